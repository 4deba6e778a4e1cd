"""Predict: ordinary images in, boxes in original-image coordinates out — the `YOLOv10DetectionPredictor` of the reference for the six
2D (`v10`) models (engine/predictor.py preprocess / pre_transform :115-156, models/yolov10/predict.py:8-38, utils/ops.py scale_boxes
:89-124) without `Results` objects and plotting.

    predictor = predict.Predictor(model, imgsz=640, conf=0.25)
    rows = predictor([bgr0, bgr1])        # list of (n_i, 6) device tensors [x1, y1, x2, y2, conf, cls], original-image pixels

The host computes what the reference computes on the host: `LetterBox(imgsz, auto=all shapes equal, stride)`'s sizes and pads
(`yolo2d.letterbox_params`) and `scale_boxes`' gain and pad (`scale_params`).  The device does the rest: `y3d_letterbox_image` (resize,
pad, BGR -> RGB, uint8 NHWC for the stem), the model's eval forward, `v10postprocess`, and `y3d_predict_rows` (confidence / class filter,
scale back, clip, ordered compaction; csrc/letterbox.hip).  The images follow the float64 bilinear arithmetic of tests/yolo2d_ref.py, not
OpenCV's fixed point.  `Predictor` refuses 3D models: their decode needs calibrations.

The six 3D (`v10-3D`) models have `Predictor3d`: RGB images and one P2 per image in, decoded rows, the eight box corners in camera
coordinates and their projections out.

    predictor = predict.Predictor3d(model, conf=0.25)
    dets = predictor([rgb0, rgb1], [P2_0, P2_1])   # list of {"rows" (n_i, 14), "corners3d" (n_i, 8, 3), "corners_img" (n_i, 8, 2)} float64
    results = predictor.predict_split(kitti_root, [0, 1, 2], out_dir="runs")   # the KITTI test split -> runs/preds/000000.txt ...
    pictures, bev = predictor.annotate([rgb0, rgb1], [P2_0, P2_1], bev=True)    # the boxes drawn over the images, and from above (plot.py)

The host computes the reference's unaugmented sample (data/datasets/kitti.py:130-135, :192, :404): the crop matrix of the whole image,
`ratio = resolution / img_size`, the six calibration constants.  The device does `y3d_kitti_image_aug` (Pillow's affine resize), the
eval forward, `v10_3Dpostprocess` (with `use_o2m_depth=True` also the dense one-to-many head, its post-process and the depth vote
`y3d_kde_depth_fusion`), and `y3d_predict3d_rows` (KITTI decode, confidence / class filter, ordered compaction, corners and
their projection; csrc/predict3d.hip)."""
from __future__ import annotations

import torch

from . import loss as _loss
from . import kitti, ops, yolo2d
from ._lib import Y3DError, lib


def pre_transform_params(shapes, imgsz=640, stride=32):
    """`BasePredictor.pre_transform` without the pixels: LetterBox(imgsz, auto=same_shapes, stride=stride) (scaleup=True) for every
    (h, w) of `shapes` -> (list of yolo2d.letterbox_params dicts, the common canvas (H, W))"""
    shapes = [(int(s[0]), int(s[1])) for s in shapes]
    if not shapes or any(h < 1 or w < 1 for h, w in shapes):
        raise Y3DError("predict: no images, or an image without pixels")
    auto = len(set(shapes)) == 1
    lbs = [yolo2d.letterbox_params(s, imgsz, auto=auto, scaleup=True, stride=stride) for s in shapes]
    canvases = {lb["canvas"] for lb in lbs}
    if len(canvases) != 1:  # np.stack of the reference would fail
        raise Y3DError(f"predict: the letter-boxed images have different shapes {sorted(canvases)}")
    return lbs, lbs[0]["canvas"]


def scale_params(img1_shape, img0_shape):
    """gain and pad of `scale_boxes(img1_shape, boxes, img0_shape)` with ratio_pad=None (utils/ops.py:107-112) -> (gain, (padw, padh))"""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    return gain, (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))


def predict_rows(preds, meta, conf, classes=None):
    """`y3d_predict_rows`: preds (B, K, 6) float32 rows [x1, y1, x2, y2, conf, cls] in the letter-boxed frame, meta (B, 5) float32
    [h0, w0, gain, padw, padh], classes an int32 device tensor or None -> (rows (B, K, 6): the kept rows first, scaled back and clipped,
    the rest zeros; counts (B,) int32).  One launch, no host synchronisation (capturable)."""
    if preds.dim() != 3 or preds.shape[-1] != 6 or preds.dtype != torch.float32 or not preds.is_cuda:
        raise Y3DError("predict_rows: expected (B, K, 6) float32 rows on a HIP device (no host fallback)")
    B, K = int(preds.shape[0]), int(preds.shape[1])
    if tuple(meta.shape) != (B, 5) or meta.dtype != torch.float32 or not meta.is_cuda:
        raise Y3DError("predict_rows: meta must be (B, 5) float32 on the device")
    if classes is not None and (classes.dtype != torch.int32 or not classes.is_cuda or classes.dim() != 1 or not classes.numel()):
        raise Y3DError("predict_rows: classes must be a non-empty int32 device vector")
    preds, meta = preds.contiguous(), meta.contiguous()
    out = torch.empty(B, K, 6, dtype=torch.float32, device=preds.device)
    counts = torch.empty(B, dtype=torch.int32, device=preds.device)
    lib().predict_rows(preds.data_ptr(), meta.data_ptr(), float(conf), classes.data_ptr() if classes is not None else None,
                       classes.numel() if classes is not None else 0, B, K, out.data_ptr(), counts.data_ptr(), ops.stream())
    return out, counts


def raw_rows(model, img, max_det):
    """eval forward + `v10postprocess` + `xywh2xyxy` -> (B, max_det, 6) float32 [x1, y1, x2, y2, conf, cls], letter-boxed frame"""
    y = model(img)["one2one"][0]
    box, scores, labels = _loss.v10postprocess(y.permute(0, 2, 1), max_det, model.yaml["nc"])
    xy, half = box[..., :2], box[..., 2:] / 2
    return torch.cat([xy - half, xy + half, scores.unsqueeze(-1), labels.unsqueeze(-1).to(scores.dtype)], -1).float()


class Predictor:
    def __init__(self, model, imgsz=640, conf=0.25, classes=None, max_det=300, stride=32):
        from .modules import v10Detect3d
        from .tasks import YOLOv10_3DDetectionModel
        if isinstance(model, YOLOv10_3DDetectionModel) or isinstance(model.model[-1], v10Detect3d):
            raise Y3DError("predict: 3D models are not supported (their decode needs calibrations)")
        self.model = model.eval()
        self.imgsz = (int(imgsz), int(imgsz)) if isinstance(imgsz, int) else (int(imgsz[0]), int(imgsz[1]))
        self.stride = int(stride)
        if self.stride % 4 or self.imgsz[1] % 4:
            raise Y3DError(f"predict: imgsz {self.imgsz} / stride {stride}: the canvas width must be a multiple of 4")
        self.conf, self.max_det = float(conf), int(max_det)
        self.classes = None if classes is None else [int(c) for c in (classes if isinstance(classes, (list, tuple)) else [classes])]
        self._cls_dev = None

    def plan(self, shapes):
        """the host arithmetic for images of `shapes` -> (records (B, 8) int32 with source b for image b, meta (B, 5) float32, (H, W))"""
        import numpy as np
        lbs, (H, W) = pre_transform_params(shapes, self.imgsz, self.stride)
        rec, meta = np.zeros((len(lbs), 8), np.int32), np.zeros((len(lbs), 5), np.float32)
        for b, ((h0, w0), lb) in enumerate(zip(shapes, lbs)):
            rec[b] = (b, h0, w0, lb["new_unpad"][1], lb["new_unpad"][0], lb["top"], lb["left"], 1)
            gain, pad = scale_params((H, W), (h0, w0))
            meta[b] = (h0, w0, gain, pad[0], pad[1])
        return rec, meta, (H, W)

    def __call__(self, images, static=False):
        """images: list of (h, w, 3) uint8 BGR numpy arrays or uint8 tensors on a HIP device.  -> list of (n_i, 6) device tensors, or with
        static=True (rows (B, K, 6), counts (B,)) without waiting for the device."""
        import numpy as np
        if not isinstance(images, (list, tuple)) or not len(images):
            raise Y3DError("predict: a non-empty list of (h, w, 3) uint8 images is expected")
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise Y3DError("predict: the model must live on a HIP device (no host fallback)")
        imgs = []
        for im in images:
            if torch.is_tensor(im):
                if not im.is_cuda:
                    raise Y3DError("predict: an image tensor that is not on a HIP device (no host fallback); pass numpy arrays to upload")
                t = im
            else:
                t = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise Y3DError("predict: images must be (h, w, 3) uint8")
            imgs.append(t)
        rec, meta, (H, W) = self.plan([tuple(t.shape[:2]) for t in imgs])
        img = yolo2d.letterbox_images(yolo2d.pack_letterbox(imgs, rec, H, W, dev), "uint8")
        if self.classes is not None and (self._cls_dev is None or self._cls_dev.device != dev):
            self._cls_dev = torch.tensor(self.classes, dtype=torch.int32).to(dev)
        with torch.no_grad():
            raw = raw_rows(self.model, img.permute(0, 3, 1, 2), self.max_det)
        rows, counts = predict_rows(raw, torch.from_numpy(meta).to(dev), self.conf, self._cls_dev if self.classes is not None else None)
        if static:
            return rows, counts
        return [rows[b, :n] for b, n in enumerate(counts.tolist())]


# ------------------------------------------------------------------------------------------------------------------------------
# 3D: images and calibrations in, decoded rows and box corners out
# ------------------------------------------------------------------------------------------------------------------------------
def _f64_rows(x, B, width, dev, what):
    import numpy as np
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    t = t.to(dev, torch.float64)
    if t.numel() != B * width:
        raise Y3DError(f"predict3d_rows: {what} of shape {tuple(t.shape)} for {B} images ({width} values each)")
    return t.reshape(B, width).contiguous()


_MEAN_SIZES = {}


def _mean_sizes(cls_mean_size, dev):
    """the (nc, 3) float64 mean-size table on the device; a table given as nested tuples is uploaded once per device"""
    if torch.is_tensor(cls_mean_size):
        return cls_mean_size.to(dev, torch.float64).reshape(-1, 3).contiguous()
    key = (str(dev), tuple(tuple(float(v) for v in r) for r in cls_mean_size))
    if key not in _MEAN_SIZES:
        _MEAN_SIZES[key] = torch.tensor(key[1], dtype=torch.float64).reshape(-1, 3).to(dev)
    return _MEAN_SIZES[key]


def predict3d_rows(preds, calib6, P2, ratio, inv_trans, conf, classes=None, cls_mean_size=kitti.CLS_MEAN_SIZE, use_camera_dis=False):
    """`y3d_predict3d_rows`: preds (B, K, 37) float32 post-processed rows on the device; calib6 (B, 6) (cu, cv, fu, fv, tx, ty) of the
    original image (or the reference's Calibration objects), P2 (B, 3, 4) float32, ratio (B, 2) or ratio_pad (B, 2, 2), inv_trans
    (B, 2, 3) or None (the fixed 1242/1280, 375/384 rescale), as `kitti.decode_preds_device` takes them; classes an int32 device vector
    or None.  -> (rows (B, K, 14), corners3d (B, K, 8, 3), corners_img (B, K, 8, 2) float64: the kept rows first, in input order, the
    rest zeros; counts (B,) int32).  One launch, no host synchronisation; with float64 device tensors for calib6, P2, ratio and
    inv_trans nothing else is launched or copied (capturable, once the mean-size table has been uploaded by an earlier call)."""
    import numpy as np
    if preds.dim() != 3 or preds.shape[-1] != 37 or preds.dtype != torch.float32 or not preds.is_cuda:
        raise Y3DError("predict3d_rows: expected (B, K, 37) float32 rows on a HIP device (no host fallback)")
    dev, B, K = preds.device, int(preds.shape[0]), int(preds.shape[1])
    if B < 1 or K < 1:
        raise Y3DError("predict3d_rows: no rows")
    if classes is not None and (not torch.is_tensor(classes) or classes.dtype != torch.int32 or not classes.is_cuda or classes.dim() != 1
                                or not classes.numel()):
        raise Y3DError("predict3d_rows: classes must be a non-empty int32 device vector")
    preds = preds.detach().contiguous()
    calib = kitti._calib_rows(calib6, B, dev)
    if not torch.is_tensor(P2):
        P2 = torch.from_numpy(np.ascontiguousarray(np.asarray(P2, np.float32)))
    if P2.numel() != B * 12:
        raise Y3DError(f"predict3d_rows: {B} images but P2 of shape {tuple(P2.shape)} (one 3 x 4 matrix each)")
    # float32 values, promoted; a float64 device tensor is taken as it is (already promoted: nothing is launched for it)
    P = (P2.to(dev) if P2.dtype == torch.float64 else P2.to(dev, torch.float32).to(torch.float64)).reshape(B, 12).contiguous()
    rp = ratio if torch.is_tensor(ratio) else torch.from_numpy(np.ascontiguousarray(np.asarray(ratio, np.float64)))
    rp = rp[:, 0] if rp.dim() == 3 else rp
    rt = _f64_rows(rp, B, 2, dev, "ratio")
    inv = None
    if inv_trans is not None:
        inv = _f64_rows(inv_trans if torch.is_tensor(inv_trans) else np.stack([np.asarray(t, np.float64).reshape(2, 3) for t in inv_trans]),
                        B, 6, dev, "inverse transforms")
    ms = _mean_sizes(cls_mean_size, dev)
    rows = torch.empty(B, K, 14, dtype=torch.float64, device=dev)
    c3 = torch.empty(B, K, 8, 3, dtype=torch.float64, device=dev)
    ci = torch.empty(B, K, 8, 2, dtype=torch.float64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    lib().predict3d_rows(preds.data_ptr(), B, K, calib.data_ptr(), P.data_ptr(), rt.data_ptr(), inv.data_ptr() if inv is not None else None,
                         ms.data_ptr(), ms.shape[0], int(bool(use_camera_dis)), float(conf), classes.data_ptr() if classes is not None else None,
                         classes.numel() if classes is not None else 0, rows.data_ptr(), c3.data_ptr(), ci.data_ptr(), counts.data_ptr(),
                         ops.stream())
    return rows, c3, ci, counts


O2M_FACTOR = 5      # the one-to-many post-process keeps max_det * 5 rows (val.py:52)
O2M_ROWS_MAX = 3902  # the most one-to-many rows `y3d_kde_depth_fusion` holds in LDS


def rows3d(y, max_det, nc):
    """`v10_3Dpostprocess` + the cat of models/yolov10_3D/val.py:46-47: y (B, nc + 35, A) decoded head output -> (B, max_det, 37) float32"""
    reg, scores, labels = _loss.v10_3Dpostprocess(y.permute(0, 2, 1), max_det, nc)
    return torch.cat((reg, scores.unsqueeze(-1), labels.unsqueeze(-1)), -1).float()


def check_o2m(max_det, A):
    """the refusals of the one-to-many depth vote, before anything is launched: the one-to-many post-process needs max_det * 5 anchors,
    the fusion kernel keeps max_det * 5 rows in LDS"""
    km = int(max_det) * O2M_FACTOR
    if km > O2M_ROWS_MAX:
        raise Y3DError(f"use_o2m_depth: max_det = {max_det} asks for {km} one-to-many rows, the depth fusion holds at most {O2M_ROWS_MAX} "
                       f"(max_det <= {O2M_ROWS_MAX // O2M_FACTOR})")
    if km > int(A):
        raise Y3DError(f"use_o2m_depth: max_det = {max_det} asks for {km} one-to-many rows, the head has {A} anchors "
                       f"(max_det <= {int(A) // O2M_FACTOR} at this image size)")


def o2m_rows3d(yO, yM, max_det, nc):
    """the validator's `postprocess` with use_o2m_depth (val.py:44-55) on the decoded outputs of the two head sets, (B, nc + 35, A) each:
    `v10_3Dpostprocess(yO, max_det)`, `v10_3Dpostprocess(yM, max_det * 5)`, the two cats, `kitti.aggregate_o2m_preds` at its defaults
    -> (fused rows (B, max_det, 37), rowsO, rowsM (B, max_det * 5, 37)).  Three launches, capturable."""
    if yO.shape != yM.shape:
        raise Y3DError(f"use_o2m_depth: one-to-one output {tuple(yO.shape)} but one-to-many output {tuple(yM.shape)}")
    check_o2m(max_det, yO.shape[-1])
    rowsO, rowsM = rows3d(yO, max_det, nc), rows3d(yM, max_det * O2M_FACTOR, nc)
    return kitti.aggregate_o2m_preds(rowsO, rowsM), rowsO, rowsM


def anchors_of(model, img):
    """the number of anchors of the 3D head for the (B, 3, H, W) image: one per cell of every level"""
    H, W = int(img.shape[-2]), int(img.shape[-1])
    return sum((-(-H // int(s))) * (-(-W // int(s))) for s in model.model[-1].stride.tolist())


def raw_rows3d(model, img, max_det, use_o2m_depth=False, depth_maps=None):
    """eval forward + `v10_3Dpostprocess` + the cat of models/yolov10_3D/val.py:46-47 -> (B, max_det, 37) float32.
    use_o2m_depth: the head also runs its dense one-to-many set (`v10Detect3d.eval_one2many`, set for this call) and the depths become
    the vote of `o2m_rows3d`; refused before any launch when max_det * 5 exceeds the anchors or the fusion kernel's 3902 rows.
    depth_maps (B, Hm, Wm): the reference's `elif use_dino_depth` - the depths are read from the maps (`kitti.depth_from_map`); with
    both, one-to-many wins and the maps are not read, as in the reference."""
    nc = model.yaml["nc"]
    if not use_o2m_depth:
        rows = rows3d(model(img)["one2one"][0], max_det, nc)
        return rows if depth_maps is None else kitti.depth_from_map(rows, depth_maps)
    check_o2m(max_det, anchors_of(model, img))
    head = model.model[-1]
    was, head.eval_one2many = head.eval_one2many, True
    try:
        out = model(img)
    finally:
        head.eval_one2many = was
    return o2m_rows3d(out["one2one"][0], out["one2many"][0], max_det, nc)[0]


def kitti_results(rows, counts, im_files):
    """the rows of `predict3d_rows` / `Predictor3d` -> {im_file: [[cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], ...]}, the
    dict `kitti.decode_preds` returns (so `kitti_eval.get_stats` and `kitti.save_results` take it).  rows: (B, K, 14) with counts (B,),
    or a list of (n_i, 14) with counts None."""
    if counts is None:
        per = [torch.as_tensor(r).reshape(-1, 14) for r in rows]
    else:
        n = counts.tolist() if torch.is_tensor(counts) else [int(c) for c in counts]
        host = torch.as_tensor(rows).cpu()
        if host.dim() != 3 or host.shape[-1] != 14 or len(n) != host.shape[0] or any(c < 0 or c > host.shape[1] for c in n):
            raise Y3DError(f"kitti_results: rows {tuple(host.shape)} do not match {len(n)} counts")
        per = [host[b, :c] for b, c in enumerate(n)]
    if len(per) != len(im_files):
        raise Y3DError(f"kitti_results: {len(per)} images but {len(im_files)} file names")
    return {f: r.cpu().tolist() for f, r in zip(im_files, per)}


class Predictor3d:
    def __init__(self, model, conf=0.25, classes=None, max_det=50, resolution=kitti.RESOLUTION, cls_mean_size=kitti.CLS_MEAN_SIZE,
                 use_camera_dis=False, use_o2m_depth=False):
        from .modules import v10Detect3d
        if not isinstance(model.model[-1], v10Detect3d):
            raise Y3DError("predict3d: a 3D model is expected (predict.Predictor takes the 2D models)")
        self.model = model.eval()
        self.resolution = (int(resolution[0]), int(resolution[1]))  # (W, H)
        stride = int(model.stride.max())
        if min(self.resolution) < 1 or self.resolution[0] % stride or self.resolution[1] % stride:
            raise Y3DError(f"predict3d: resolution {self.resolution} must be a multiple of the model's stride {stride}")
        self.conf, self.max_det = float(conf), int(max_det)
        self.classes = None if classes is None else [int(c) for c in (classes if isinstance(classes, (list, tuple)) else [classes])]
        self.cls_mean_size, self.use_camera_dis = cls_mean_size, bool(use_camera_dis)
        self.use_o2m_depth = bool(use_o2m_depth)  # the depths become the vote of the one-to-many proposals (raw_rows3d)
        self._cls_dev = None

    def plan(self, shapes, P2s):
        """the host arithmetic of the reference's unaugmented sample for images of `shapes` (h, w) with projections `P2s` ->
        {"trans_inv" (B, 2, 3), "ratio" (B, 2), "calib6" (B, 6) float64, "P2" (B, 3, 4) float32}"""
        import numpy as np
        shapes = [(int(s[0]), int(s[1])) for s in shapes]
        if not shapes or any(h < 1 or w < 1 for h, w in shapes):
            raise Y3DError("predict3d: no images, or an image without pixels")
        if len(P2s) != len(shapes):
            raise Y3DError(f"predict3d: {len(shapes)} images but {len(P2s)} P2 matrices")
        P = [np.asarray(p.cpu() if torch.is_tensor(p) else p, np.float32) for p in P2s]
        if any(p.shape != (3, 4) for p in P):
            raise Y3DError("predict3d: every P2 must be a (3, 4) matrix")
        res = np.array(self.resolution)
        inv, ratio = [], []
        for h, w in shapes:
            img_size = np.array([w, h])
            inv.append(kitti.get_affine_transform(img_size / 2, img_size, self.resolution, inv=True)[1])
            ratio.append(res / img_size)
        return {"trans_inv": np.stack(inv), "ratio": np.stack(ratio).astype(np.float64),
                "calib6": np.array([kitti.calib_params(p) for p in P], np.float64), "P2": np.stack(P)}

    def __call__(self, images, P2s, static=False):
        """images: list of (h, w, 3) uint8 RGB numpy arrays or uint8 tensors on a HIP device; P2s: one (3, 4) matrix per image.
        -> list of {"rows" (n_i, 14), "corners3d" (n_i, 8, 3), "corners_img" (n_i, 8, 2)} device tensors (one read-back of the counts),
        or with static=True (rows (B, K, 14), corners3d (B, K, 8, 3), corners_img (B, K, 8, 2), counts (B,)) without waiting."""
        import numpy as np
        if not isinstance(images, (list, tuple)) or not len(images):
            raise Y3DError("predict3d: a non-empty list of (h, w, 3) uint8 images is expected")
        if not isinstance(P2s, (list, tuple)) and not (torch.is_tensor(P2s) or isinstance(P2s, np.ndarray)):
            raise Y3DError("predict3d: one (3, 4) P2 matrix per image is expected")
        if len(P2s) != len(images):
            raise Y3DError(f"predict3d: {len(images)} images but {len(P2s)} P2 matrices")
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise Y3DError("predict3d: the model must live on a HIP device (no host fallback)")
        imgs = []
        for im in images:
            if torch.is_tensor(im):
                if not im.is_cuda:
                    raise Y3DError("predict3d: an image tensor that is not on a HIP device (no host fallback); pass numpy arrays to upload")
                t = im
            else:
                t = torch.from_numpy(np.ascontiguousarray(im)).to(dev)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise Y3DError("predict3d: images must be (h, w, 3) uint8")
            imgs.append(t)
        B = len(imgs)
        p = self.plan([tuple(t.shape[:2]) for t in imgs], list(P2s))
        img = kitti.augment_images(imgs, [None] * B, [False] * B, list(p["trans_inv"]), self.resolution, "uint8")
        return self._rows(img, p, static)

    def _rows(self, img, p, static):
        """img (B, H, W, 3) uint8 at the resolution, p = plan(..) -> the eval forward, the post-process and the row pass"""
        import numpy as np
        dev = img.device
        if self.classes is not None and (self._cls_dev is None or self._cls_dev.device != dev):
            self._cls_dev = torch.tensor(self.classes, dtype=torch.int32).to(dev)
        with torch.no_grad():
            raw = raw_rows3d(self.model, img.permute(0, 3, 1, 2), self.max_det, use_o2m_depth=self.use_o2m_depth)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        rows, c3, ci, counts = predict3d_rows(raw, up(p["calib6"]), up(p["P2"]), up(p["ratio"]), up(p["trans_inv"]), self.conf,
                                              self._cls_dev if self.classes is not None else None, self.cls_mean_size, self.use_camera_dis)
        if static:
            return rows, c3, ci, counts
        return [{"rows": rows[b, :n], "corners3d": c3[b, :n], "corners_img": ci[b, :n]} for b, n in enumerate(counts.tolist())]

    def annotate(self, images, P2s, results=None, bev=False, thickness=2):
        """the box wireframes over the original images (plot.draw_boxes3d): images and P2s as `__call__` takes them,
        results what `__call__` returned for them, in either form (None: the predictor runs).  The images are grouped by shape and
        every group is uploaded, drawn and read back once; the caller's arrays and tensors are left as they are.
        -> a list of (h, w, 3) uint8 numpy arrays, and with bev=True (that list, the BEV maps (B, 600, 1200, 3) uint8 numpy)."""
        import numpy as np
        from . import plot
        if results is None:
            results = self(images, P2s, static=True)
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise Y3DError("predict3d: the model must live on a HIP device (no host fallback)")
        B = len(images)
        if isinstance(results, (list, tuple)) and len(results) == 4 and torch.is_tensor(results[0]):
            rows, c3, _, counts = results
        else:  # the list form: pad to the longest image
            if len(results) != B:
                raise Y3DError(f"annotate: {B} images but results for {len(results)}")
            K = max([int(d["rows"].shape[0]) for d in results] + [1])
            rows, c3 = torch.zeros(B, K, 14, dtype=torch.float64, device=dev), torch.zeros(B, K, 8, 3, dtype=torch.float64, device=dev)
            for b, d in enumerate(results):
                n = int(d["rows"].shape[0])
                rows[b, :n], c3[b, :n] = d["rows"].to(dev), d["corners3d"].to(dev)
            counts = torch.tensor([int(d["rows"].shape[0]) for d in results], dtype=torch.int32).to(dev)
        if rows.shape[0] != B or len(P2s) != B:
            raise Y3DError(f"annotate: {B} images, {len(P2s)} P2 matrices and results for {rows.shape[0]} images")
        P = np.stack([np.asarray(p.cpu() if torch.is_tensor(p) else p, np.float32).reshape(3, 4) for p in P2s]).astype(np.float64)
        P = torch.from_numpy(P).to(dev)
        groups = {}
        for b, im in enumerate(images):
            groups.setdefault(tuple(int(v) for v in im.shape), []).append(b)
        out = [None] * B
        for shape, idx in groups.items():
            u8 = lambda im: im.dtype == (torch.uint8 if torch.is_tensor(im) else np.uint8)
            if len(shape) != 3 or shape[2] != 3 or not all(u8(images[b]) for b in idx):
                raise Y3DError("annotate: images must be (h, w, 3) uint8")
            if torch.is_tensor(images[idx[0]]):
                canvas = torch.stack([images[b].to(dev) for b in idx]).contiguous()
            else:
                canvas = torch.from_numpy(np.ascontiguousarray(np.stack([images[b] for b in idx]))).to(dev)
            sel = torch.tensor(idx, dtype=torch.int64).to(dev)
            plot.draw_boxes3d(canvas, c3.index_select(0, sel), rows.index_select(0, sel), counts.index_select(0, sel), P.index_select(0, sel),
                              thickness=thickness)
            for b, pic in zip(idx, canvas.cpu().numpy()):
                out[b] = pic
        if not bev:
            return out
        return out, plot.draw_bev(c3, rows, counts).cpu().numpy()

    def predict_split(self, root_or_split_file, indices, out_dir=None):
        """the KITTI test split: `kitti.build_test_batch` -> the predictor -> `kitti_results`; with out_dir, `kitti.save_results` writes
        out_dir/preds/<id>.txt as the reference's `save_results`.  -> {im_file: rows}"""
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise Y3DError("predict3d: the model must live on a HIP device (no host fallback)")
        batch = kitti.build_test_batch(root_or_split_file, indices, dev, img_mode="uint8", resolution=self.resolution)
        # the batch's image is the predictor's own (the same crop matrices); its calib is scaled by the ratio, the decode wants the original's
        p = self.plan([tuple(s) for s in batch["ori_shape"]], list(batch["P2"].cpu().numpy()))
        rows, _, _, counts = self._rows(batch["img"], p, True)
        results = kitti_results(rows, counts, batch["im_file"])
        if out_dir is not None:
            kitti.save_results(results, out_dir)
        return results
