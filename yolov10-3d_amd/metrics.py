"""Validator box metrics on the device: precision, recall, mAP50 and mAP50-95 — named after the reference's utils/metrics.py.

Drop-ins for `box_iou` (utils/metrics.py:53), the validator's `match_predictions` (engine/validator.py:229-273, use_scipy = False) and
`_process_batch` (models/yolo/detect/val.py:197-209), `ap_per_class` (:532), `Metric` / `DetMetrics` / `Det3dMetrics` (:623, :795,
:896), and `BoxStats`, the accumulator behind both validators' `update_metrics` / `get_stats` (models/yolo/detect/val.py:97-175,
models/yolov10_3D/val.py:114-187).  The reference matches and scores on the host with per-image numpy loops; here one HIP launch per
validation batch matches every image (csrc/det_metrics.hip) and appends to device accumulators without a host synchronisation, and
one launch per `get_stats` computes every class's AP and recall / precision curves.  The host only smooths the mean F1 curve.

Deliberate tie rules where the reference is implementation-defined (its argsorts are unstable quicksorts): an IoU tie between two
class-matched labels of one detection goes to the higher gt index; detections of equal confidence keep accumulation order (image,
then row).  Limits: `max_gts()` gts and `max_dets()` detections per image.

`ConfusionMatrix` (utils/metrics.py:281) is what both validators feed when `plots` is on (the default): one launch per validation
batch adds into an int32 matrix on the device; its tie rules are in the class docstring.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import ops
from ._lib import Y3DError, lib

IOUV = torch.linspace(0.5, 0.95, 10)  # models/yolo/detect/val.py:40, fp32
_X_AP = np.linspace(0, 1, 101)        # compute_ap's COCO grid
_X_CURVE = np.linspace(0, 1, 1000)    # ap_per_class's curve grid
_CONST = {}


def max_gts() -> int:
    return lib().det_metrics_max_gts()


def max_dets() -> int:
    return lib().det_metrics_max_dets()


def _on_device(who, *ts):
    for t in ts:
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise Y3DError(f"{who} runs on a HIP device: pass device tensors (there is no CPU fallback)")


def _const(dev):
    """iouv, the 101- and 1000-point grids on `dev` (uploaded once)"""
    key = str(dev)
    if key not in _CONST:
        _CONST[key] = (IOUV.to(dev), torch.from_numpy(_X_AP).to(dev), torch.from_numpy(_X_CURVE).to(dev))
    return _CONST[key]


def _unpack(mask, n_thr):
    return ((mask.unsqueeze(1) >> torch.arange(n_thr, device=mask.device, dtype=mask.dtype)) & 1).bool()


def _pack(tp):
    tp = tp.reshape(tp.shape[0], -1)
    return (tp.to(torch.int32) << torch.arange(tp.shape[1], device=tp.device, dtype=torch.int32)).sum(1, dtype=torch.int32)


def box_iou(box1, box2, eps=1e-7):
    """utils/metrics.py:53: (N, M) fp32 IoU of xyxy boxes, bit for bit"""
    _on_device("box_iou", box1, box2)
    a = box1.detach().reshape(-1, 4).float().contiguous()
    b = box2.detach().reshape(-1, 4).float().contiguous()
    out = torch.empty(a.shape[0], b.shape[0], dtype=torch.float32, device=a.device)
    lib().box_iou(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], float(eps), out.data_ptr(), ops.stream())
    return out


def match_predictions(pred_classes, true_classes, iou):
    """engine/validator.py:229-273 (use_scipy = False): iou (labels, detections) -> (detections, 10) bool correct matrix"""
    n_gt, n_det = int(iou.shape[0]), int(iou.shape[1])
    if n_gt > max_gts() or n_det > max_dets():
        raise Y3DError(f"match_predictions: {n_gt} labels / {n_det} detections; at most {max_gts()} / {max_dets()} per image")
    _on_device("match_predictions", pred_classes, true_classes, iou)
    thr = _const(iou.device)[0]
    tp = torch.zeros(n_det, dtype=torch.int32, device=iou.device)
    if n_det:  # the converted tensors stay referenced until the launch is queued
        v = iou.detach().float().contiguous()
        gc = true_classes.reshape(-1).to(torch.int32).contiguous()
        dc = pred_classes.reshape(-1).to(torch.int32).contiguous()
        lib().match_predictions(v.data_ptr(), gc.data_ptr(), n_gt, dc.data_ptr(), n_det, thr.data_ptr(), thr.numel(), tp.data_ptr(), ops.stream())
    return _unpack(tp, thr.numel())


def process_batch(detections, gt_bboxes, gt_cls):
    """DetectionValidator._process_batch (models/yolo/detect/val.py:197-209): detections (N, 6) xyxy, conf, cls"""
    return match_predictions(detections[:, 5], gt_cls, box_iou(gt_bboxes, detections[:, :4]))


def smooth(y, f=0.05):
    """utils/metrics.py:441: a box filter over round(2 f len) // 2 * 2 + 1 points, the ends padded with the end values"""
    w = round(len(y) * f * 2) // 2 + 1
    pad = w // 2
    yp = np.concatenate((np.full(pad, y[0]), y, np.full(pad, y[-1])))
    return np.convolve(yp, np.ones(w) / w, mode="valid")


def _ap_device(mask, conf, cls, unique_classes, nt, n_thr, eps):
    """AP (nc, n_thr), p_curve, r_curve (nc, 1000) for the classes with targets; mask / conf / cls in accumulation order on the device"""
    dev = mask.device
    nc = len(unique_classes)
    if nc == 0:
        return np.zeros((0, n_thr)), np.zeros((0, 1000)), np.zeros((0, 1000))
    o = torch.sort(conf, descending=True, stable=True).indices
    o = o[torch.sort(cls[o], stable=True).indices]
    tp_s, conf_s, cls_s = mask[o].contiguous(), conf[o].contiguous(), cls[o].contiguous()
    ucls = torch.from_numpy(np.asarray(unique_classes, dtype=np.int32)).to(dev)
    nl = torch.from_numpy(np.asarray(nt, dtype=np.int64) + eps).to(dev)
    _, x_ap, x_cv = _const(dev)
    out = torch.empty(nc * (n_thr + 2 * x_cv.numel()), dtype=torch.float64, device=dev)
    ap = out[:nc * n_thr]
    pc = out[nc * n_thr:nc * (n_thr + x_cv.numel())]
    rc = out[nc * (n_thr + x_cv.numel()):]
    lib().ap_per_class(tp_s.data_ptr(), conf_s.data_ptr(), cls_s.data_ptr(), tp_s.numel(), ucls.data_ptr(), nl.data_ptr(), nc, n_thr,
                       x_ap.data_ptr(), x_ap.numel(), x_cv.data_ptr(), x_cv.numel(), ap.data_ptr(), pc.data_ptr(), rc.data_ptr(), ops.stream())
    h = out.cpu().numpy()
    m = x_cv.numel()
    return h[:nc * n_thr].reshape(nc, n_thr), h[nc * n_thr:nc * (n_thr + m)].reshape(nc, m), h[nc * (n_thr + m):].reshape(nc, m)


def _operating_point(ap, p_curve, r_curve, unique_classes, nt, eps):
    """the host tail of ap_per_class: F1 curves, the smoothed-mean-F1 operating point, the 12-tuple"""
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    i = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    tp = (r * nt).round()
    fp = (tp / (p + eps) - tp).round()
    return tp, fp, p, r, f1, ap, np.asarray(unique_classes).astype(int), p_curve, r_curve, f1_curve, _X_CURVE.copy(), np.array([])


def _classes(target_cls_host):
    return np.unique(np.asarray(target_cls_host).astype(np.int64), return_counts=True)


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, on_plot=None, save_dir=Path(), names=(), eps=1e-16, prefix=""):
    """utils/metrics.py:532 on device tensors: (tp, fp, p, r, f1, ap, unique_classes, p_curve, r_curve, f1_curve, x, prec_values) as
    numpy arrays; prec_values is empty (the reference fills it only for plots).  Classes are integers."""
    if plot:
        raise Y3DError("ap_per_class: plotting is not supported (plot=False only)")
    _on_device("ap_per_class", tp, conf, pred_cls, target_cls)
    tp = tp.reshape(tp.shape[0], -1)
    n_thr = tp.shape[1]
    unique_classes, nt = _classes(target_cls.cpu().numpy())
    ap, pc, rc = _ap_device(_pack(tp), conf.reshape(-1).to(torch.float64), pred_cls.reshape(-1).to(torch.int32), unique_classes, nt, n_thr, eps)
    return _operating_point(ap, pc, rc, unique_classes, nt, eps)


class Metric:
    """utils/metrics.py:623: per-class P, R, F1, AP (nc, 10) and their means"""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = [], [], [], [], []
        self.nc = 0

    @property
    def ap50(self):
        return self.all_ap[:, 0] if len(self.all_ap) else []

    @property
    def ap(self):
        return self.all_ap.mean(1) if len(self.all_ap) else []

    @property
    def mp(self):
        return self.p.mean() if len(self.p) else 0.0

    @property
    def mr(self):
        return self.r.mean() if len(self.r) else 0.0

    @property
    def map50(self):
        return self.all_ap[:, 0].mean() if len(self.all_ap) else 0.0

    @property
    def map75(self):
        return self.all_ap[:, 5].mean() if len(self.all_ap) else 0.0

    @property
    def map(self):
        return self.all_ap.mean() if len(self.all_ap) else 0.0

    def mean_results(self):
        return [self.mp, self.mr, self.map50, self.map]

    def class_result(self, i):
        return self.p[i], self.r[i], self.ap50[i], self.ap[i]

    @property
    def maps(self):
        maps = np.zeros(self.nc) + self.map
        for i, c in enumerate(self.ap_class_index):
            maps[c] = self.ap[i]
        return maps

    def fitness(self):
        return (np.array(self.mean_results()) * [0.0, 0.0, 0.1, 0.9]).sum()

    def update(self, results):
        (self.p, self.r, self.f1, self.all_ap, self.ap_class_index, self.p_curve, self.r_curve, self.f1_curve, self.px,
         self.prec_values) = results

    @property
    def curves(self):
        return []

    @property
    def curves_results(self):
        return [[self.px, self.prec_values, "Recall", "Precision"], [self.px, self.f1_curve, "Confidence", "F1"],
                [self.px, self.p_curve, "Confidence", "Precision"], [self.px, self.r_curve, "Confidence", "Recall"]]


class DetMetrics:
    """utils/metrics.py:795: box metrics with fitness 0.1 mAP50 + 0.9 mAP50-95 (upstream YOLO)"""

    def __init__(self, save_dir=Path("."), plot=False, on_plot=None, names=()):
        self.save_dir, self.plot, self.on_plot, self.names = save_dir, plot, on_plot, names
        self.box = Metric()
        self.speed = {"preprocess": 0.0, "inference": 0.0, "loss": 0.0, "postprocess": 0.0}
        self.task = "detect"

    def process(self, tp, conf, pred_cls, target_cls):
        self._update(ap_per_class(tp, conf, pred_cls, target_cls, plot=self.plot, names=self.names))

    def _update(self, results):
        self.box.nc = len(self.names)
        self.box.update(results[2:])

    @property
    def keys(self):
        return ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"]

    def mean_results(self):
        return self.box.mean_results()

    def class_result(self, i):
        return self.box.class_result(i)

    @property
    def maps(self):
        return self.box.maps

    @property
    def fitness(self):
        return self.box.fitness()

    @property
    def ap_class_index(self):
        return self.box.ap_class_index

    @property
    def results_dict(self):
        return dict(zip(self.keys + ["fitness"], self.mean_results() + [self.fitness]))

    @property
    def curves(self):
        return ["Precision-Recall(B)", "F1-Confidence(B)", "Precision-Confidence(B)", "Recall-Confidence(B)"]

    @property
    def curves_results(self):
        return self.box.curves_results


class Det3dMetrics(DetMetrics):
    """utils/metrics.py:896, what both validators of this fork construct: the box metrics plus `metrics/3D`, which is also the fitness"""

    def __init__(self, save_dir=Path("."), plot=False, on_plot=None, names=()):
        super().__init__(save_dir, plot, on_plot, names)
        self.metric3d = 0

    @property
    def keys(self):
        return super().keys + ["metrics/3D"]

    @property
    def fitness(self):
        return self.metric3d

    def class_result(self, i):
        return self.box.class_result(i) + ((self.metric3d,) if i == 1 else (-1,))

    def mean_results(self):
        return self.box.mean_results() + [self.metric3d]


def _host_rows(v, B, who):
    """per-image sequences (as collated) -> (B, w) float64 numpy"""
    if torch.is_tensor(v):
        v = v.detach().cpu()
    rows = np.stack([np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float64).reshape(-1) for x in v]) if len(v) else np.zeros((0, 1))
    if rows.shape[0] != B:
        raise Y3DError(f"{who}: {B} images but {rows.shape[0]} rows")
    return rows


def _upload(a, dev):
    """host array -> device without waiting for the queue (pinned, non-blocking)"""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


class BoxStats:
    """The validators' box statistics on the device.

        stats = BoxStats(nc=80)
        for batch in loader:
            stats.update_2d(preds, batch)             # DetectionValidator.update_metrics (v10postprocess + xywh2xyxy rows)
            # or stats.update_3d(rows, keep, batch)   # YOLOv10_3DDetectionValidator.update_metrics (kitti.decode_preds_device)
        results = stats.get_stats(metrics)            # metrics: Det3dMetrics (both validators of this fork) or DetMetrics

    `update_*` launch one kernel per batch and never wait for the device.  A batch with more than `max_dets()` rows per image is
    refused at once; an image with more than `max_gts()` gts is refused by `get_stats` (the count is only known on the device).
    """

    def __init__(self, nc, single_cls=False, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise Y3DError(f"BoxStats accumulates on a HIP device, not {self.device}")
        self.nc, self.single_cls = int(nc), bool(single_cls)
        self.iouv = IOUV.to(self.device)
        self.niou = self.iouv.numel()
        self.reset()

    def reset(self):
        dev = self.device
        self.seen, self.nt_per_class = 0, None
        self._n = self._ng = 0
        self._tp = torch.empty(0, dtype=torch.int32, device=dev)
        self._conf = torch.empty(0, dtype=torch.float64, device=dev)
        self._cls = torch.empty(0, dtype=torch.int32, device=dev)
        self._tcls = torch.empty(0, dtype=torch.int32, device=dev)
        self._status = torch.zeros(1, dtype=torch.int32, device=dev)

    @staticmethod
    def _grow(buf, used, need):
        if used + need <= buf.numel():
            return buf
        out = torch.empty(max(2 * buf.numel(), used + need, 4096), dtype=buf.dtype, device=buf.device)
        out[:used] = buf[:used]
        return out

    def _targets(self, batch, B, who):
        idx = batch["batch_idx"].detach().reshape(-1)
        cls = batch["cls"].detach().reshape(-1)
        box = batch["bboxes"].detach().reshape(-1, 4)
        _on_device(who, idx, cls, box)
        if not (idx.numel() == cls.numel() == box.shape[0]):
            raise Y3DError(f"{who}: batch_idx / cls / bboxes disagree ({idx.numel()}, {cls.numel()}, {box.shape[0]})")
        return idx.float().contiguous(), cls.float().contiguous(), box.float().contiguous()

    def _launch(self, mode, preds, keep, meta, imgsz, tgt, who):
        B, K = int(preds.shape[0]), int(preds.shape[1])
        idx, cls, box = tgt
        n = B * K
        self._tp = self._grow(self._tp, self._n, n)
        self._conf = self._grow(self._conf, self._n, n)
        self._cls = self._grow(self._cls, self._n, n)
        self._tcls = self._grow(self._tcls, self._ng, cls.numel())
        o = self._n
        lib().box_match_batch(mode, preds.data_ptr(), keep.data_ptr() if keep is not None else None, B, K, meta.data_ptr(), int(imgsz[0]),
                              int(imgsz[1]), int(self.single_cls), idx.data_ptr(), cls.data_ptr(), box.data_ptr(), idx.numel(),
                              self.iouv.data_ptr(), self.niou, self._tp[o:].data_ptr(), self._conf[o:].data_ptr(), self._cls[o:].data_ptr(),
                              self._status.data_ptr(), ops.stream())
        self._tcls[self._ng:self._ng + cls.numel()] = cls
        self._n += n
        self._ng += cls.numel()
        self.seen += B

    @staticmethod
    def _check_k(preds, who):
        if preds.shape[1] > max_dets():
            raise Y3DError(f"{who}: {preds.shape[1]} detections per image; at most {max_dets()} are supported")

    def update_2d(self, preds, batch):
        """DetectionValidator.update_metrics (models/yolo/detect/val.py:128-164): preds (B, K, 6) [x1, y1, x2, y2, conf, cls] in the
        letterboxed frame (the YOLOv10 validator's v10postprocess + xywh2xyxy output); batch with batch_idx, cls, bboxes (normalised
        xywh), ori_shape and ratio_pad per image, and img (or imgsz = (H, W))."""
        who = "BoxStats.update_2d"
        if preds.dim() != 3 or preds.shape[-1] != 6:
            raise Y3DError(f"{who}: expected (B, K, 6) predictions, got {tuple(preds.shape)}")
        self._check_k(preds, who)
        _on_device(who, preds)
        B = int(preds.shape[0])
        tgt = self._targets(batch, B, who)
        imgsz = tuple(batch["img"].shape[2:]) if "img" in batch else tuple(batch["imgsz"])
        ori = _host_rows(batch["ori_shape"], B, who)[:, :2]
        rp = _host_rows(batch["ratio_pad"], B, who)  # ((gain, gain), (padw, padh)) -> gain, gain, padw, padh
        meta = _upload(np.concatenate((ori, rp[:, [0, 2, 3]]), 1), self.device)
        self._launch(0, preds.detach().float().contiguous(), None, meta, imgsz, tgt, who)

    def update_3d(self, rows, keep, batch):
        """YOLOv10_3DDetectionValidator.update_metrics (models/yolov10_3D/val.py:114-164) box part: rows (B, K, 14) float64 and keep
        (B, K) from kitti.decode_preds_device (the decode_preds_eval rows, never copied to the host); batch with batch_idx, cls, bboxes
        (normalised xywh) and ori_shape (h, w) per image."""
        who = "BoxStats.update_3d"
        if rows.dim() != 3 or rows.shape[-1] != 14 or keep is None or tuple(keep.shape) != tuple(rows.shape[:2]):
            raise Y3DError(f"{who}: expected (B, K, 14) rows and a (B, K) keep mask, got {tuple(rows.shape)} / "
                           f"{None if keep is None else tuple(keep.shape)}")
        self._check_k(rows, who)
        _on_device(who, rows, keep)
        B = int(rows.shape[0])
        tgt = self._targets(batch, B, who)
        meta = _upload(_host_rows(batch["ori_shape"], B, who)[:, :2], self.device)
        self._launch(1, rows.detach().to(torch.float64).contiguous(), keep.detach().to(torch.bool).contiguous().view(torch.uint8), meta,
                     (0, 0), tgt, who)

    def get_stats(self, metrics, metric3d=0.0):
        """get_stats of the validators: runs ap_per_class when any detection is a true positive, sets `nt_per_class`, sets
        `metrics.metric3d` (Det3dMetrics; the 3D validator's KITTI AP, kitti_eval.get_stats) and returns `metrics.results_dict`."""
        if getattr(metrics, "plot", False):
            raise Y3DError("BoxStats.get_stats: plotting is not supported (metrics.plot = False only)")
        n = self._n
        tp, conf, cls = self._tp[:n], self._conf[:n], self._cls[:n]
        head = torch.cat((self._status, (tp != 0).any().reshape(1).to(torch.int32), self._tcls[:self._ng])).cpu().numpy()
        if head[0] > 0:
            raise Y3DError(f"BoxStats: an image has {int(head[0])} gts; at most {max_gts()} are supported")
        tcls = head[2:]
        self.nt_per_class = np.bincount(tcls.astype(int), minlength=self.nc)
        if head[1]:
            unique_classes, nt = _classes(tcls)
            ap, pc, rc = _ap_device(tp, conf, cls, unique_classes, nt, self.niou, 1e-16)
            metrics._update(_operating_point(ap, pc, rc, unique_classes, nt, 1e-16))
        if isinstance(metrics, Det3dMetrics):
            metrics.metric3d = metric3d
        return metrics.results_dict


def _targets(batch, who):
    """batch_idx (n), cls (n), bboxes (n, 4) of a collated batch as contiguous float32 device tensors"""
    idx = batch["batch_idx"].detach().reshape(-1)
    cls = batch["cls"].detach().reshape(-1)
    box = batch["bboxes"].detach().reshape(-1, 4)
    _on_device(who, idx, cls, box)
    if not (idx.numel() == cls.numel() == box.shape[0]):
        raise Y3DError(f"{who}: batch_idx / cls / bboxes disagree ({idx.numel()}, {cls.numel()}, {box.shape[0]})")
    return idx.float().contiguous(), cls.float().contiguous(), box.float().contiguous()


class ConfusionMatrix:
    """utils/metrics.py:281 for detection, accumulated on the device (csrc/det_metrics.hip, `y3d_confusion_batch`).

        cm = ConfusionMatrix(nc=80, conf=args.conf)
        for batch in loader:
            cm.update_2d(preds, batch)              # what DetectionValidator.update_metrics feeds it (models/yolo/detect/val.py:137, :151)
            # or cm.update_3d(rows, keep, batch)    # YOLOv10_3DDetectionValidator.update_metrics (models/yolov10_3D/val.py:138, :156)
        cm.matrix                                   # (nc + 1, nc + 1) float64 numpy [predicted, true], index nc = background

    `update_*` take exactly what `BoxStats.update_*` take, launch one kernel per batch and never wait for the device; like the
    validators they skip an image without gts.  `process_batch(detections, gt_bboxes, gt_cls)` is the reference's method on device
    tensors (prepared xyxy boxes, one image).  Reading `matrix` is the only read-back; it raises when an image had more than
    `max_gts()` gts or a class lay outside [0, nc).

    A detection takes part iff its confidence > conf (strict; float32 for 2D rows and float32 drop-in detections, float64 for 3D rows
    and float64 drop-in detections); pairs with IoU > float32(iou_thres) are matched whatever their classes: each detection keeps its
    best gt, then each gt keeps the best of the detections that chose it.  An image without a single match does not count its
    detections (the reference's `if n:`).  Deliberate tie rules where the reference is implementation-defined (its argsort is an
    unstable quicksort), what a stable sort, reversed, gives: an IoU tie between two gts of one detection goes to the higher gt index,
    an IoU tie between two detections on one gt goes to the higher detection index.  `plot()` and task="classify" are not supported."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, task="detect", device=None):
        if task != "detect":
            raise Y3DError(f"ConfusionMatrix: task {task!r} is not supported (detect only)")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise Y3DError(f"ConfusionMatrix accumulates on a HIP device, not {self.device}")
        self.task, self.nc = task, int(nc)
        if self.nc < 1:
            raise Y3DError(f"ConfusionMatrix: nc = {nc}")
        self.conf = 0.25 if conf in (None, 0.001) else conf  # apply 0.25 if default val conf is passed (utils/metrics.py:304)
        self.iou_thres = iou_thres
        if not float(self.iou_thres) >= 0.0:
            raise Y3DError(f"ConfusionMatrix: iou_thres = {iou_thres} (must not be negative)")
        self._m = self._status = None

    def _buffers(self):
        if self._m is None:
            self._m = torch.zeros(self.nc + 1, self.nc + 1, dtype=torch.int32, device=self.device)
            self._status = torch.zeros(2, dtype=torch.int32, device=self.device)
        return self._m, self._status

    def reset(self):
        if self._m is not None:
            self._m.zero_()
            self._status.zero_()

    @property
    def matrix(self):
        """(nc + 1, nc + 1) float64 numpy, the reference's dtype; the one read-back"""
        m, status = self._buffers()
        h = torch.cat((status, m.reshape(-1))).cpu().numpy()
        if h[0] > 0:
            raise Y3DError(f"ConfusionMatrix: an image has {int(h[0])} gts; at most {max_gts()} are supported")
        if h[1]:
            raise Y3DError(f"ConfusionMatrix: a class outside [0, {self.nc}) was met")
        return h[2:].reshape(self.nc + 1, self.nc + 1).astype(np.float64)

    def tp_fp(self):
        """utils/metrics.py:382: true and false positives per class, background removed"""
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]

    def plot(self, *a, **k):
        raise Y3DError("ConfusionMatrix.plot: plotting is not supported; read .matrix")

    def print(self):
        for row in self.matrix:
            print(" ".join(map(str, row)))

    def process_batch(self, detections, gt_bboxes, gt_cls):
        """utils/metrics.py:319: detections (N, 6) [x1, y1, x2, y2, conf, cls] or None, gt_bboxes (M, 4) xyxy, gt_cls (M); one image"""
        who = "ConfusionMatrix.process_batch"
        _on_device(who, gt_cls)
        n_gt = int(gt_cls.shape[0])
        det, n_det, f64 = None, 0, 0
        if detections is not None:
            _on_device(who, detections)
            if detections.dim() != 2 or detections.shape[1] != 6:
                raise Y3DError(f"{who}: expected (N, 6) detections, got {tuple(detections.shape)} (oriented boxes are not supported)")
            f64 = int(detections.dtype == torch.float64)
            det = detections.detach().contiguous() if f64 else detections.detach().float().contiguous()
            n_det = int(det.shape[0])
        if n_gt > max_gts() or n_det > max_dets():
            raise Y3DError(f"{who}: {n_gt} labels / {n_det} detections; at most {max_gts()} / {max_dets()} per image")
        gb = gc = None
        if n_gt:
            _on_device(who, gt_bboxes)
            gb = gt_bboxes.detach().reshape(-1, 4).float().contiguous()
            gc = gt_cls.detach().reshape(-1).to(torch.int32).contiguous()
            if gb.shape[0] != n_gt:
                raise Y3DError(f"{who}: {n_gt} classes but {gb.shape[0]} boxes")
        m, status = self._buffers()
        lib().confusion_image(gb.data_ptr() if n_gt else None, gc.data_ptr() if n_gt else None, n_gt, det.data_ptr() if det is not None and n_det else None,
                              f64, n_det, self.nc, float(self.conf), float(self.iou_thres), m.data_ptr(), status.data_ptr(), ops.stream())

    def _launch(self, mode, preds, keep, meta, imgsz, tgt, single_cls):
        idx, cls, box = tgt
        m, status = self._buffers()
        B, K = int(preds.shape[0]), int(preds.shape[1])
        lib().confusion_batch(mode, preds.data_ptr() if K else None, keep.data_ptr() if keep is not None and K else None, B, K, meta.data_ptr(),
                              int(imgsz[0]), int(imgsz[1]), int(bool(single_cls)), idx.data_ptr(), cls.data_ptr(), box.data_ptr(), idx.numel(),
                              self.nc, float(self.conf), float(self.iou_thres), m.data_ptr(), status.data_ptr(), ops.stream())

    def update_2d(self, preds, batch, single_cls=False):
        """the confusion-matrix part of DetectionValidator.update_metrics; arguments as `BoxStats.update_2d`"""
        who = "ConfusionMatrix.update_2d"
        if preds.dim() != 3 or preds.shape[-1] != 6:
            raise Y3DError(f"{who}: expected (B, K, 6) predictions, got {tuple(preds.shape)}")
        BoxStats._check_k(preds, who)
        _on_device(who, preds)
        B = int(preds.shape[0])
        tgt = _targets(batch, who)
        imgsz = tuple(batch["img"].shape[2:]) if "img" in batch else tuple(batch["imgsz"])
        ori = _host_rows(batch["ori_shape"], B, who)[:, :2]
        rp = _host_rows(batch["ratio_pad"], B, who)
        meta = _upload(np.concatenate((ori, rp[:, [0, 2, 3]]), 1), self.device)
        self._launch(0, preds.detach().float().contiguous(), None, meta, imgsz, tgt, single_cls)

    def update_3d(self, rows, keep, batch, single_cls=False):
        """the confusion-matrix part of YOLOv10_3DDetectionValidator.update_metrics; arguments as `BoxStats.update_3d`"""
        who = "ConfusionMatrix.update_3d"
        if rows.dim() != 3 or rows.shape[-1] != 14 or keep is None or tuple(keep.shape) != tuple(rows.shape[:2]):
            raise Y3DError(f"{who}: expected (B, K, 14) rows and a (B, K) keep mask, got {tuple(rows.shape)} / "
                           f"{None if keep is None else tuple(keep.shape)}")
        BoxStats._check_k(rows, who)
        _on_device(who, rows, keep)
        B = int(rows.shape[0])
        tgt = _targets(batch, who)
        meta = _upload(_host_rows(batch["ori_shape"], B, who)[:, :2], self.device)
        self._launch(1, rows.detach().to(torch.float64).contiguous(), keep.detach().to(torch.bool).contiguous().view(torch.uint8), meta,
                     (0, 0), tgt, single_cls)
