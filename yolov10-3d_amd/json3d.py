"""Waymo and Omni3D training batches on the device — the two JSON-split datasets of the reference's 3D trainer.

Mirrors `WaymoDataset` (data/datasets/waymo.py) and `Omni3Dataset` (data/datasets/omni3d.py): `__getitem__` + `collate_fn`.  The split
JSON, the images (PIL) and the random decisions stay on the host; the images are mixed / mirrored / cropped by `kitti.augment_images`
and the labels filtered and encoded by one launch of `y3d_json3d_encode_labels` (csrc/json3d_labels.hip), in the static
50-rows-per-image layout `DDDetectionLoss.targets` and `GraphedTrainStep` already take from `kitti.build_batch`.

Predictions decode with the KITTI decoder and the dataset's own size table:
`kitti.decode_preds(..., cls_mean_size=json3d.WAYMO_CLS_MEAN_SIZE)` for Waymo, the default (KITTI's table) for Omni3D.

`DeviceSplit` keeps a split decoded and resident - in HBM and, behind what HBM may hold, in pinned host memory - and builds the same
batches from it without opening a file (`plan_batch`, csrc/json3d_cache.hip).

The compact form has the reference's collated dtypes.  One value differs within float32 rounding: the static layout
stores `size_2d` as float32, so Waymo's float64 `size_2d` carries float32-rounded values.
"""
from __future__ import annotations

import torch

from . import kitti, ops
from ._lib import Y3DError, lib
from .kitti import MAX_OBJS, PER_BOX
from .resident import ResidentSplit, check_plan, span_table, upload

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
    wider = {"heading_res": torch.float64, **({"size_2d": torch.float64} if _dataset_mode(dataset) == 0 else {})}
    return kitti._compact(static, counts, [True] * len(counts), use_camera_dis, max_objs, wider)


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
    `args.cam_dis` encodes the camera distance (the reference's datasets hard-code use_camera_dis = False).
    json_file may also be a `DeviceSplit`: the same batch from the resident split, without any file access."""
    import numpy as np
    from PIL import Image
    if isinstance(json_file, DeviceSplit):  # the split is resident (its own dataset): no file is touched
        json_file.check_device(device)
        return json_file.build_batch(indices, args, mode=mode, compact=compact, img_mode=img_mode)
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


# ------------------------------------------------------------------------------------------------------------------------------
# the split resident in two tiers: decoded once into HBM and, behind what HBM may hold, into pinned host memory
# ------------------------------------------------------------------------------------------------------------------------------
_DRAW_W = 18  # a row of the draw table: kitti's sixteen columns, then the staging byte offset of the primary and of the partner (-1: arena)


def draw_table(indices, draws, staged):
    """sample_augment's draws for dataset positions `indices` -> the (B, 18) float64 draw table of `y3d_json3d_plan_batch`: the rows of
    `kitti.draw_table`, then the byte offset of the primary's frame and of the partner's in the batch's staging buffer (`staged`:
    {position: offset}, the host-tier frames), or -1 for a frame of the device arena and for no partner."""
    import numpy as np
    table = np.empty((len(indices), _DRAW_W), np.float64)
    table[:, :16] = kitti.draw_table(indices, draws)
    for row, p, d in zip(table, indices, draws):
        row[16], row[17] = staged.get(p, -1), staged.get(d["partner"], -1)
    return table


def plan_batch(split, draws, draws_dev=None, out=None, spill=None):
    """The per-image tables of `y3d_kitti_image_aug` and `y3d_json3d_encode_labels` for a table of draws over a DeviceSplit, one HIP
    launch (`y3d_json3d_plan_batch`).  draws: (B, 18) float64 on the host (numpy or tensor), `draw_table`'s rows; draws_dev: the same
    table on the device (uploaded here when None); spill: the batch's staging buffer, a uint8 tensor on the split's device that holds
    the host-tier frames at the offsets the table names (None: the batch uses none).  The launcher refuses positions and partners
    outside the split and staging offsets that do not fit the frame's tier or the buffer; that each staged frame also ends inside the
    buffer is checked here, from the host sizes.  out: optionally the eight output tensors (at least B rows each; the first B are
    written).  -> `kitti.plan_batch`'s dict."""
    host, draws_dev, out = check_plan(draws, _DRAW_W, split.device, kitti.PLAN_TABLES, draws_dev, out)
    nbytes = 0
    if spill is not None:
        if not torch.is_tensor(spill) or spill.dtype != torch.uint8 or spill.device != split.device or spill.dim() != 1 or not spill.is_contiguous():
            raise Y3DError(f"plan_batch: the staging buffer must be a contiguous 1-D uint8 tensor on {split.device}")
        nbytes = spill.numel()
    N = len(split)
    for b, row in enumerate(host.tolist()):
        for what, pos, off in (("position", row[0], row[16]), ("partner", row[1], row[17])):
            if off >= 0 and 0 <= pos < N and pos == int(pos) and off + int(split._frame_bytes[int(pos)]) > nbytes:
                raise Y3DError(f"plan_batch: image {b}: {what} {pos:g} staged at {off:g} ends outside the staging buffer of {nbytes} bytes")
    lib().json3d_plan_batch(split.img_off.data_ptr(), split.frame_hw.data_ptr(), split.rec_span.data_ptr(), split.P2.data_ptr(), N, split.n_dev,
                            split.arena.data_ptr() if split.n_dev else None, spill.data_ptr() if nbytes else None, nbytes, host.data_ptr(),
                            draws_dev.data_ptr(), host.shape[0], *[out[k].data_ptr() for k, _, _ in kitti.PLAN_TABLES], ops.stream())
    return out


class DeviceSplit(ResidentSplit):
    """A Waymo / Omni3D split decoded once and kept resident: `DeviceSplit(json_file, dataset)` parses the split as `read_split` does,
    reads the frame sizes from the image headers and lays the frames out in two tiers before anything is decoded or allocated
    (`resident.tier_layout`).  Frames in dataset order go into one uint8 device arena (`arena`) while their bytes fit `max_bytes`
    (default: half of the device's free memory); every frame behind the first one that does not fit goes into `host_arena`, allocated
    pinned and written by the decoder threads directly; `n_dev` is the boundary.  A host tier of more than `host_bytes` is refused, so
    the default 0 behaves like `kitti.DeviceSplit`: all in HBM, or refused.  Frames are held as originals only (the crop reads the
    original pixels).  Device tables, indexed by dataset position: `img_off` (N) int64 (-1 in the host tier), `frame_hw` (N, 2) int32
    (H, W), `rec` (R, 24) float64 = object_records of every frame in order, `rec_span` (N, 2) int32, `P2` (N, 2, 12) float64 (as read;
    `flip_calib` of it, float32 widened), `mean_size`.  On the host: `P2_host`, `wh`, `n_lines`, `cam`, `ids`, `files`, `dataset`.

    `build_batch` returns what `build_batch(json_file, ...)` returns, bit for bit, without touching a file: the draws, one
    non-blocking copy per distinct host-tier frame of the batch from the pinned arena into a staging buffer, one non-blocking upload
    of the draw table from a ring of pinned buffers and three launches (plan_batch, the image augmentation, the label encoder)."""

    def __init__(self, json_file, dataset, mode="train", device="cuda", max_bytes=None, host_bytes=0, workers=8, overfit=False):
        import numpy as np
        from PIL import Image
        _dataset_mode(dataset)
        dev = self._accept(device, mode, workers, host_bytes)
        sp = read_split(json_file, dataset, bool(overfit))
        self.dataset, self.ids = dataset, list(sp.ids)
        self.files = [sp.file(i) for i in self.ids]
        # sizes from the image headers, the budget of both tiers before anything is decoded or allocated
        self._layout_tiers(dev, self._sizes(self.files), max_bytes, host_bytes)
        recs = [sp.records(i) for i in self.ids]
        self.P2_host = [sp.P2(i) for i in self.ids]
        self.n_lines = [len(r) for r in recs]
        self.cam = [(P[0, 2], P[1, 2], P[0, 0], P[1, 1]) for P in self.P2_host]
        self.rec = upload(np.concatenate(recs) if sum(self.n_lines) else np.zeros((1, REC_W)), dev, torch.float64)
        both = [np.stack((P.reshape(12), flip_calib(P, wh).astype(np.float64).reshape(12))) for P, wh in zip(self.P2_host, self.wh)]
        self.P2 = upload(np.stack(both), dev, torch.float64)
        self.mean_size = upload(np.asarray(CLS_MEAN_SIZE[dataset], np.float64).reshape(-1, 3), dev, torch.float64)

        def decode(pos):
            with Image.open(self.files[pos]) as im:
                return np.array(im.convert("RGB"))

        self._fill_tiers(span_table(self.n_lines), decode, lambda pos: f"frame {self.files[pos]}", workers, _DRAW_W)

    def __len__(self):
        return len(self.ids)

    def frame_info(self, pos, primary=False):
        """sample_augment's frame_info: ((cu, cv, fu, fv), objects, (W, H) or None).  The size is reported for a batch's primary
        position only and None for a partner candidate, as `build_batch(json_file, ...)` reports them: the reference reads the
        partner's size from the primary image (waymo.py:162), so a candidate is not turned down for its size."""
        return self.cam[pos], self.n_lines[pos], (self.wh[pos] if primary else None)

    def sample(self, indices, args, mode="train"):
        """The draws of `build_batch(json_file, ...)` for `indices` from the same np.random state: one `kitti.sample_augment` per image,
        whose first question is about the primary.  A drawn partner whose true size differs from the primary's is refused."""
        draws = []
        for pos in indices:
            first = [True]

            def frame_info(p, _first=first):
                primary, _first[0] = _first[0], False
                return self.frame_info(p, primary)

            draws += kitti.sample_augment(len(self), [pos], frame_info, args, mode, MAX_OBJS, RESOLUTION)
            d = draws[-1]
            if d["mixed"] and self.wh[d["partner"]] != self.wh[pos]:
                raise Y3DError(f"build_batch: mixup partner {d['partner']} of position {pos} has another size (the reference mixes "
                               f"equal-sized frames only)")
        return draws

    def build_batch(self, indices, args, mode="train", compact=False, img_mode="uint8"):
        """`build_batch(json_file, indices, args, device, dataset, ...)` from the resident split: the same dictionary, bit for bit.  With
        compact=False nothing here waits for the device (but a ring buffer still in flight) and no file is opened."""
        if mode == "test":
            raise Y3DError("build_batch: the test split has no labels")
        indices = [int(i) for i in indices]
        N, B = len(self), len(indices)
        if B < 1 or any(not 0 <= p < N for p in indices):
            raise Y3DError(f"build_batch: {B} positions, all must lie in [0, {N})")
        draws = self.sample(indices, args, mode)
        cam_dis = bool(getattr(args, "cam_dis", False))
        with torch.cuda.device(self.device):
            staged, spill = self._stage([p for pos, d in zip(indices, draws) for p in (pos, d["partner"])])
            host, dev = self._ring.upload(draw_table(indices, draws, staged))
            plan = plan_batch(self, host, dev, spill=spill)
            img, lab = kitti._resident_tail(self, plan, args, cam_dis, img_mode, RESOLUTION, encode_labels, dataset=self.dataset)
        return kitti._batch(img, lab, [self.ids[p] for p in indices], [self.wh[p] for p in indices], draws, self.mean_size, plan["mixed"],
                            compact and (lambda counts: compact_labels(lab, counts, cam_dis, MAX_OBJS, self.dataset)))
