"""Predict: ordinary images in, boxes in original-image coordinates out — the `YOLOv10DetectionPredictor` of the reference for the six
2D (`v10`) models (engine/predictor.py preprocess / pre_transform :115-156, models/yolov10/predict.py:8-38, utils/ops.py scale_boxes
:89-124) without `Results` objects and plotting.

    predictor = predict.Predictor(model, imgsz=640, conf=0.25)
    rows = predictor([bgr0, bgr1])        # list of (n_i, 6) device tensors [x1, y1, x2, y2, conf, cls], original-image pixels

The host computes what the reference computes on the host: `LetterBox(imgsz, auto=all shapes equal, stride)`'s sizes and pads
(`yolo2d.letterbox_params`) and `scale_boxes`' gain and pad (`scale_params`).  The device does the rest: `y3d_letterbox_image` (resize,
pad, BGR -> RGB, uint8 NHWC for the stem), the model's eval forward, `v10postprocess`, and `y3d_predict_rows` (confidence / class filter,
scale back, clip, ordered compaction; csrc/letterbox.hip).  The images follow the float64 bilinear arithmetic of tests/yolo2d_ref.py, not
OpenCV's fixed point.  3D models are refused: their decode needs calibrations."""
from __future__ import annotations

import torch

from . import loss as _loss
from . import ops, yolo2d
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
