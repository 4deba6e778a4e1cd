"""Waymo and Omni3D training batches on the device — the two JSON-split datasets of the reference's 3D trainer.

Mirrors `WaymoDataset` (data/datasets/waymo.py) and `Omni3Dataset` (data/datasets/omni3d.py): `__getitem__` + `collate_fn`.  The split
JSON, the images (PIL) and the random decisions stay on the host; the images are mixed / mirrored / cropped by `kitti.augment_images`
and the labels filtered and encoded by one launch of `y3d_json3d_encode_labels` (csrc/json3d_labels.hip), in the static
50-rows-per-image layout `DDDetectionLoss.targets` and `GraphedTrainStep` already take from `kitti.build_batch`.

Predictions decode with the KITTI decoder and the dataset's own size table:
`kitti.decode_preds(..., cls_mean_size=json3d.WAYMO_CLS_MEAN_SIZE)` for Waymo, the default (KITTI's table) for Omni3D.

The compact form has the reference's collated dtypes.  One value differs within float32 rounding: the static layout
stores `size_2d` as float32, so Waymo's float64 `size_2d` carries float32-rounded values.
"""
from __future__ import annotations

import torch

from . import kitti, ops
from ._lib import Y3DError, lib
from .kitti import MAX_OBJS, PER_BOX

DATASETS = {"waymo": 0, "omni3d": 1}  # the kernel's dataset mode
RESOLUTION = (960, 640)  # W, H (waymo.py:31, omni3d.py:31)
CLASS_IDS = {"Car": 0, "Pedestrian": 1, "Cyclist": 2}  # cls2train_id of both datasets; their writelist
WAYMO_DATA_ID2CLS = {0: "unknown", 1: "Car", 2: "Pedestrian", 3: "Cyclist"}  # waymo.py:45
WAYMO_CLS2EVAL_ID = {"unknown": 0, "Car": 1, "Pedestrian": 2, "Sign": 3, "Cyclist": 4}  # waymo.py:43
# (h, w, l) per class, waymo.py:58-61
WAYMO_CLS_MEAN_SIZE = ((1.7974, 2.106, 4.8117), (1.751, 0.85498, 0.90977), (1.7697, 0.83474, 1.769))
OMNI3D_CLS_MEAN_SIZE = kitti.CLS_MEAN_SIZE  # omni3d.py:59-62
CLS_MEAN_SIZE = {"waymo": WAYMO_CLS_MEAN_SIZE, "omni3d": OMNI3D_CLS_MEAN_SIZE}
REC_W = 24
# record columns (include/y3d.h)
_CLS, _BOX, _H, _W, _L, _POS, _RY, _LIDAR, _BEHIND, _VALID, _DERR, _TRUNC, _VIS = 0, 1, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17


def _dataset_mode(dataset):
    if dataset not in DATASETS:
        raise Y3DError(f"json3d: dataset must be one of {sorted(DATASETS)}, got {dataset!r}")
    return DATASETS[dataset]


def yaw_from_matrix(R):
    """`Rotation.from_matrix(R).as_euler('xyz')[1]` (kitti_utils.py:63-64) in numpy.  As scipy does, the matrix is first replaced by
    the nearest rotation (U V^T of its singular value decomposition), so the rounded digits of a JSON give the same angle; then the
    middle angle of the extrinsic x-y-z decomposition, in [-pi/2, pi/2]."""
    import numpy as np
    m = np.asarray(R, np.float64).reshape(3, 3)
    u, _, vt = np.linalg.svd(m)
    m = u @ vt
    return float(np.arctan2(-m[2, 0], np.hypot(m[0, 0], m[1, 0])))


def object_records(anns, dataset):
    """One image's annotation dicts (each with its `category` name) -> (n, 24) float64 records of y3d_json3d_encode_labels, in the
    dtypes `Object3d.__init__` parses them to (kitti_utils.py:39-74): box float32, everything else float64."""
    import numpy as np
    mode = _dataset_mode(dataset)
    r = np.zeros((len(anns), REC_W), np.float64)
    for n, a in enumerate(anns):
        r[n, _CLS] = CLASS_IDS.get(a["category"], -1)
        if mode == 0:
            if a.get("rotation_y", None) is None:
                raise Y3DError("json3d: a Waymo annotation without rotation_y")
            box = np.array(a["bbox"])
            r[n, _BOX:_BOX + 4] = np.array([box[0], box[1], box[0] + box[2], box[1] + box[3]], dtype=np.float32)
            dim = np.array(a["dim"])
            r[n, _H], r[n, _W], r[n, _L] = dim[0], dim[1], dim[2]
            r[n, _POS:_POS + 3] = np.array(a["translation"])
            r[n, _RY] = a["rotation_y"]
            r[n, _LIDAR] = a["num_lidar"]
            r[n, _VALID], r[n, _VIS] = 1, -1
        else:
            r[n, _BOX:_BOX + 4] = np.array(np.array(a["bbox2D_proj"]), dtype=np.float32)
            dim = np.array(a["dimensions"])
            r[n, _W], r[n, _H], r[n, _L] = dim[0], dim[1], dim[2]
            r[n, _POS:_POS + 3] = np.array(a["center_cam"]) + np.array([0, r[n, _H] / 2, 0])
            r[n, _RY] = yaw_from_matrix(a["R_cam"])
            r[n, _LIDAR] = a["lidar_pts"]
            r[n, _BEHIND] = float(bool(a["behind_camera"]))
            r[n, _VALID] = float(bool(a.get("valid3D", True)))
            r[n, _DERR], r[n, _TRUNC], r[n, _VIS] = a["depth_error"], a["truncation"], a["visibility"]
    return r


class Split:
    """A split JSON as the datasets' constructors index it: `ids` (image ids, ascending; position -> id is the reference's
    idx_to_img_id), and per image id `file(id)`, `P2(id)` (3, 4) float64, `records(id)` (n, 24)."""

    def __init__(self, json_file, dataset, overfit=False):
        import json
        import os
        import numpy as np
        self.dataset, self.mode = dataset, _dataset_mode(dataset)
        self.root = os.path.dirname(json_file)
        with open(json_file) as f:
            raw = json.load(f)
        images, anns = raw["images"], raw["annotations"]
        if overfit:  # waymo.py:36-38
            images = [im for im in images if im["id"] < 50]
            anns = [a for a in anns if a["image_id"] < 50]
        self.imgs = {im["id"]: im for im in sorted(images, key=lambda im: im["id"])}
        self.ids = list(self.imgs)
        if self.mode == 0:
            self.id2cls = dict(WAYMO_DATA_ID2CLS)
        else:  # omni3d.py:47-48
            cls2id = {c["name"].title(): c["id"] for c in raw["categories"]}
            self.id2cls = {i: name for name, i in cls2id.items()}
        self.anns = {}
        for a in anns:
            a = dict(a, category=self.id2cls[a["category_id"]])
            self.anns.setdefault(a["image_id"], []).append(a)
        self._rec, self._np = {}, np

    def __len__(self):
        return len(self.ids)

    def file(self, i):
        import os
        im = self.imgs[i]
        return os.path.join(self.root, im["file_name"] if self.mode == 0 else im["file_path"].replace("waymo/images/", ""))

    def P2(self, i):
        np = self._np
        if self.mode == 0:
            return np.array(self.imgs[i]["calib"], np.float64).reshape(3, 4)
        return np.hstack((np.array(self.imgs[i]["K"], np.float64).reshape(3, 3), np.zeros((3, 1))))

    def records(self, i):
        if i not in self._rec:
            self._rec[i] = object_records(self.anns.get(i, []), self.dataset)
        return self._rec[i]


def flip_calib(P2, img_size):
    """`Calibration.flip` for the float64 calibration these datasets hold: `kitti.flip_calib`'s fit, with the eight points lifted by
    the float64 intrinsics (KITTI's text reader makes them float32 first, which `kitti.flip_calib` reproduces).  -> P2 (3, 4) float32"""
    import numpy as np
    P = np.asarray(P2, np.float64)
    cam = (P[0, 2], P[1, 2], P[0, 0], P[1, 1], P[0, 3] / -P[0, 0], P[1, 3] / -P[1, 1])
    return kitti._flip_fit(cam, float(img_size[0]), float(img_size[1]), P[2, 3])


def pack_labels(records, partners, P2s, trans, flips, scales, img_sizes, device, dataset):
    """Host side of encode_labels: B images' object records (partners[b]: the mixup partner's, or None), their P2 (float64 as read,
    or the float32 `flip_calib` result when flips[b]), crop matrices, crop scales and original (W, H) -> dict of device tensors"""
    import numpy as np
    records_of = lambda r: np.asarray(r, np.float64).reshape(-1, REC_W)
    packed = kitti._pack(records, partners, P2s, trans, flips, scales, img_sizes, device, (records_of, REC_W, "float64", CLS_MEAN_SIZE[dataset]))
    return dict(packed, dataset=dataset)


def encode_labels(packed, out_wh=RESOLUTION, min_depth=1.0, max_depth=120.0, use_camera_dis=False, max_objs=MAX_OBJS):
    """The label encoding of the dataset's `__getitem__` + `collate_fn` for a packed batch, one HIP launch, no host synchronisation
    (capturable).  -> `kitti.encode_labels`' dict: the per-box keys in the static layout, `counts`, `calib`, `ratio_pad`."""
    img_i = packed["img_i"]
    if not img_i.is_cuda or any(not packed[k].is_cuda for k in ("rec", "img_f", "mean_size")):
        raise Y3DError("encode_labels: the packed labels must live on a HIP device (no host fallback)")
    if packed["rec"].shape[-1] != REC_W:
        raise Y3DError(f"encode_labels: records of width {packed['rec'].shape[-1]}, expected {REC_W}")
    mode = _dataset_mode(packed["dataset"])
    B = img_i.shape[0]
    o = kitti._label_outputs(B, max_objs, img_i.device)
    ms = packed["mean_size"]
    lib().json3d_encode_labels(packed["rec"].data_ptr(), img_i.data_ptr(), packed["img_f"].data_ptr(), B, mode, int(out_wh[0]),
                               int(out_wh[1]), float(min_depth), float(max_depth), int(bool(use_camera_dis)), ms.data_ptr(), ms.shape[0],
                               int(max_objs), *[o[k].data_ptr() for k in PER_BOX], o["counts"].data_ptr(), o["calib"].data_ptr(),
                               o["ratio_pad"].data_ptr(), ops.stream())
    return o


def compact_labels(static, counts, use_camera_dis=False, max_objs=MAX_OBJS, dataset="waymo"):
    """`kitti.compact_labels` with these datasets' dtypes: positions and yaw are float64 here, so depth (crops = all True) and
    heading_res are float64 in every image, and Waymo's recomputed box makes its size_2d float64 (Omni3D's stays float32 unless an
    image without boxes promotes it).  heading_res is gathered again from the static float64 column, not widened from float32."""
    out = kitti.compact_labels(static, counts, [True] * len(counts), use_camera_dis, max_objs)
    rows = torch.cat([torch.arange(b * max_objs, b * max_objs + int(c)) for b, c in enumerate(counts)]).to(static["cls"].device)
    out["heading_res"] = static["heading_res"].index_select(0, rows).to(torch.float64)
    if _dataset_mode(dataset) == 0:
        out["size_2d"] = out["size_2d"].to(torch.float64)
    return out


def decode_batch_device(batch, calibs, P2=None, undo_augment=True, dataset="waymo", use_camera_dis=False, cls_mean_size=None):
    """`kitti.decode_batch_device` with the dataset's mean sizes (`CLS_MEAN_SIZE[dataset]`): waymo.py's and omni3d.py's `decode_batch`
    are copies of KITTI's.  calibs: the original images' six constants (`Validator3d._dataset` gives them from the split's P2)."""
    _dataset_mode(dataset)
    return kitti.decode_batch_device(batch, calibs, P2, undo_augment, CLS_MEAN_SIZE[dataset] if cls_mean_size is None else cls_mean_size, use_camera_dis)


def decode_batch(batch, calibs, undo_augment=True, dataset="waymo", use_camera_dis=False, cls_mean_size=None):
    """`kitti.decode_batch` with the dataset's mean sizes -> {im_file: [row lists]} after one read-back"""
    _dataset_mode(dataset)
    return kitti.decode_batch(batch, calibs, undo_augment, CLS_MEAN_SIZE[dataset] if cls_mean_size is None else cls_mean_size, use_camera_dis)


_SPLITS = {}


def read_split(json_file, dataset, overfit=False):
    """The parsed split, cached per (file, dataset, overfit, mtime)"""
    import os
    key = (os.path.abspath(json_file), dataset, bool(overfit), os.path.getmtime(json_file))
    if key not in _SPLITS:
        _SPLITS[key] = Split(json_file, dataset, overfit)
    return _SPLITS[key]


def build_batch(json_file, indices, args, device, dataset="waymo", mode="train", compact=False, img_mode="uint8"):
    """`collate_fn([dataset[i] for i in indices])` of the reference's WaymoDataset / Omni3Dataset built on `json_file`, with the image
    and label work on the device.  `indices` are dataset positions (images in ascending id order).  -> every key collate_fn returns
    except ori_img; the per-box keys in encode_labels' static layout, or with compact=True (one read-back of the counts) in
    collate_fn's ragged shapes.  img_mode "uint8": (B, H, W, 3) uint8 for the stem; "float": the reference's (B, 3, H, W) float32.
    `args.cam_dis` encodes the camera distance (the reference's datasets hard-code use_camera_dis = False)."""
    import numpy as np
    from PIL import Image
    _dataset_mode(dataset)
    if torch.device(device).type != "cuda":
        raise Y3DError("build_batch: the batch is built on a HIP device (no host fallback)")
    if mode == "test":
        raise Y3DError("build_batch: the test split has no labels")
    sp = read_split(json_file, dataset, bool(getattr(args, "overfit", False)))
    ids = sp.ids
    open_rgb = lambda i: Image.open(sp.file(i)).convert("RGB")
    frames = [open_rgb(ids[pos]) for pos in indices]
    draws = []
    for pos, im in zip(indices, frames):
        first = [True]

        def frame_info(p, _first=first, _size=im.size):
            # the partner's size is read from the primary image (waymo.py:162): only the primary reports one
            size, _first[0] = (_size if _first[0] else None), False
            P = sp.P2(ids[p])
            return (P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(sp.records(ids[p])), size

        draws += kitti.sample_augment(len(ids), [pos], frame_info, args, mode, MAX_OBJS, RESOLUTION)
    to_dev = lambda im: torch.from_numpy(np.array(im)).to(device)
    imgs = [to_dev(im) for im in frames]
    parts = [to_dev(open_rgb(ids[d["partner"]])) if d["mixed"] else None for d in draws]
    img = kitti.augment_images(imgs, parts, [d["flip"] for d in draws], [d["trans_inv"] for d in draws], RESOLUTION,
                               mode="float" if img_mode == "float" else "uint8")
    P2s = [flip_calib(sp.P2(ids[pos]), im.size) if d["flip"] else sp.P2(ids[pos]) for pos, d, im in zip(indices, draws, frames)]
    packed = pack_labels([sp.records(ids[pos]) for pos in indices], [sp.records(ids[d["partner"]]) if d["mixed"] else None for d in draws],
                         P2s, [d["trans"] for d in draws], [d["flip"] for d in draws], [d["scale"] for d in draws],
                         [im.size for im in frames], device, dataset)
    cam_dis = bool(getattr(args, "cam_dis", False))
    lab = encode_labels(packed, RESOLUTION, args.min_depth_threshold, args.max_depth_threshold, cam_dis, MAX_OBJS)
    mixed = torch.tensor([int(d["mixed"]) for d in draws], dtype=torch.uint8).to(device)
    return kitti._batch(img, lab, [ids[p] for p in indices], [im.size for im in frames], draws, packed["mean_size"], mixed,
                        compact and (lambda counts: compact_labels(lab, counts, cam_dis, MAX_OBJS, dataset)))
