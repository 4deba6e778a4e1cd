"""One-call validators: a model and a split in, the reference validators' results out.

    results = val.Validator3d(model, kitti_root)()                      # YOLOv10_3DDetectionValidator (models/yolov10_3D/val.py)
    results = val.Validator2d(model, yolo2d.RectSplit(img_dir, 640))()  # DetectionValidator with the YOLOv10 post-process

Both run the stages the library already has, in the reference's order, per batch: the validation batch builder (`kitti.build_batch` /
`json3d.build_batch` / `yolo2d.build_batch`, mode="val"), the eval forward (through `graph.GraphedForward` with graph=True), the
NMS-free post-process, `metrics.BoxStats.update_*` and, with `plots` (the reference's default), `metrics.ConfusionMatrix.update_*`.
The batches are built with compact=True (the builders' one read-back of the per-image label counts): `BoxStats` counts every row of
`batch["cls"]` as a target, so the padding rows of the static layout must not reach it.  Beyond that nothing is copied to the host
inside the loop and no stage waits for the device; the 3D rows are read back once after the last batch.  After the call: `metrics` (a `Det3dMetrics`, which both validators of this fork build, with
`speed` and `confusion_matrix` set as `finalize_metrics` sets them), `confusion_matrix`, `seen`, `nt_per_class`, `speed` (ms per
image under the reference's keys, from device events read once after the loop; `loss` stays 0.0) and, for 3D, `results`.
There is no host fallback: the model must live on a HIP device."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import json3d, kitti, kitti_eval, metrics, plot, yolo2d
from . import loss as _loss
from ._lib import Y3DError
from .graph import GraphedForward
from .predict import _mean_sizes, predict3d_rows, raw_rows, raw_rows3d


def _is_3d(model):
    from .modules import v10Detect3d
    return isinstance(model.model[-1], v10Detect3d)


class _Validator:
    def __init__(self, model, want_3d, conf, max_det, single_cls, plots, graph):
        who = type(self).__name__
        if not hasattr(model, "model") or _is_3d(model) != want_3d:
            raise Y3DError(f"{who}: a {'3D' if want_3d else '2D'} model is expected ({'Validator2d' if want_3d else 'Validator3d'} takes the "
                           f"{'2D' if want_3d else '3D'} models)")
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise Y3DError(f"{who}: the model must live on a HIP device, not {self.device} (no host fallback)")
        self.model, self.nc = model, int(model.yaml["nc"])
        self.conf, self.max_det, self.single_cls, self.plots, self.graph = float(conf), int(max_det), bool(single_cls), bool(plots), bool(graph)
        self._graphs = {}
        self.metrics = self.confusion_matrix = self.nt_per_class = None
        self.seen = 0
        self.speed = {"preprocess": 0.0, "inference": 0.0, "loss": 0.0, "postprocess": 0.0}

    def _graph_key(self, img):
        return tuple(img.shape)

    def _raw(self, img):
        """img (B, H, W, 3) uint8 -> the post-processed rows of the eval forward, eagerly or replayed from one hipGraph per shape"""
        if not self.graph:
            with torch.no_grad():
                return self._rows(img)
        key = self._graph_key(img)
        if key not in self._graphs:
            self._graphs[key] = GraphedForward(self._rows, img)
        return self._graphs[key](img)

    def _start(self):
        self.stats = metrics.BoxStats(self.nc, single_cls=self.single_cls, device=self.device)
        self.confusion_matrix = metrics.ConfusionMatrix(self.nc, conf=self.conf, device=self.device)
        self.seen = 0
        self._events = []

    def _mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _finish(self, metric3d):
        self.metrics = metrics.Det3dMetrics(names=self.model.names)
        res = self.stats.get_stats(self.metrics, metric3d)  # the first wait for the device
        self.seen, self.nt_per_class = self.stats.seen, self.stats.nt_per_class
        ms = np.zeros(3)
        for ev in self._events:
            ms += [a.elapsed_time(b) for a, b in zip(ev[:-1], ev[1:])]
        per = ms / max(self.seen, 1)
        self.speed = {"preprocess": float(per[0]), "inference": float(per[1]), "loss": 0.0, "postprocess": float(per[2])}
        self.metrics.speed = self.speed  # finalize_metrics (models/yolo/detect/val.py:162-165)
        self.metrics.confusion_matrix = self.confusion_matrix
        return res

    def __call__(self):
        was_training = self.model.training
        self.model.eval()
        try:
            return self._run()
        finally:
            self.model.train(was_training)


class Validator3d(_Validator):
    """`YOLOv10_3DDetectionValidator` for a KITTI root or split file (dataset="kitti") or a Waymo / Omni3D split JSON.  A KITTI split
    may also be passed as a `kitti.DeviceSplit`: its frames are validated in its own order, batches are built without file access.
    So may a Waymo / Omni3D split as a `json3d.DeviceSplit`, with `dataset` = the split's own.

    Per batch of `batch` consecutive dataset positions: the val batch, the eval forward, `v10_3Dpostprocess`,
    `kitti.decode_preds_device` with the dataset's mean sizes and threshold = conf, `BoxStats.update_3d`, and
    `ConfusionMatrix.update_3d` when `plots`.  The kept rows become `self.results` ({im_file: rows}) with one read-back after the loop.
    KITTI: `metrics/3D` = `kitti_eval.get_stats(results, label_dir or <root>/training/label_2)`.  Waymo and Omni3D: the reference's
    metric shells out to a TensorFlow environment, so `metrics/3D` keeps `Det3dMetrics`' initial value, 0.
    `resolution` applies to KITTI; the other two datasets have the fixed `json3d.RESOLUTION`.  `speed`: preprocess = the batch builder,
    inference = the eval forward (with graph=True the replay, which includes `v10_3Dpostprocess`), postprocess = the rest.

    `pictures` = n > 0 (the reference's `plot_val_samples` / `plot_predictions` take the first 3 batches): for the first n batches, up to
    nine images each of the label picture (`plot.label_pictures`), the prediction picture (predictions at threshold 0.1, decoded with
    undo_augment=False, under the labels' wireframes, as `plot_preds` draws them) and the BEV map with the decoded labels as `gt`, all
    made on the device after the batch's metrics and read back once after the loop into `self.pictures`, a list of {"labels", "preds",
    "bev"} uint8 arrays.  With pictures=0 (the default) nothing more is launched than before.

    The depth refinements of the reference's `postprocess` (val.py:33-59), both off by default (the defaults fall back
    to `args.use_o2m_depth` / `args.use_dino_depth`) and off meaning the launches above, call for call:
    `use_o2m_depth`: the head's `eval_one2many` is set for the run, and the depth of every row becomes the vote of the one-to-many
    proposals (`predict.o2m_rows3d`: both post-processes and `kitti.aggregate_o2m_preds`; with graph=True all of it is replayed).
    `use_dino_depth`: `depth_fn`, or the callable registered with `loss.set_teacher`, is called on the batch image (a (B, 3, H, W) uint8 view) under
    no_grad, `(depth_maps, embeddings) = fn(img)`, outside the graph and after the replay, and the depths are read from its maps
    (`kitti.depth_from_map`, launched eagerly).  With both switches one-to-many wins, as in the reference.  Decode, `BoxStats`,
    confusion matrix, pictures and `results` take the refined rows."""

    PICTURE_CONF, PICTURE_IMGS = 0.1, 9  # plot_preds' threshold, KITTIVisualizer.max_imgs

    def __init__(self, model, root_or_split, args=None, dataset="kitti", batch=16, conf=0.001, max_det=50, single_cls=False, plots=True,
                 resolution=kitti.RESOLUTION, label_dir=None, graph=False, pictures=0, use_o2m_depth=None, use_dino_depth=None, depth_fn=None):
        if int(pictures) != pictures or int(pictures) < 0:
            raise Y3DError(f"Validator3d: pictures = {pictures!r} (the number of leading batches to draw, 0 for none)")
        super().__init__(model, True, conf, max_det, single_cls, plots, graph)
        if dataset not in ("kitti", "waymo", "omni3d"):
            raise Y3DError(f"Validator3d: dataset {dataset!r} (kitti, waymo or omni3d)")
        if int(batch) < 1:
            raise Y3DError(f"Validator3d: batch = {batch}")
        if isinstance(root_or_split, kitti.DeviceSplit) and dataset != "kitti":
            raise Y3DError(f"Validator3d: a kitti.DeviceSplit holds a KITTI split, not dataset {dataset!r}")
        if isinstance(root_or_split, json3d.DeviceSplit) and dataset != root_or_split.dataset:
            raise Y3DError(f"Validator3d: this json3d.DeviceSplit holds a {root_or_split.dataset} split, not dataset {dataset!r}")
        self.source, self.dataset, self.batch = root_or_split, dataset, int(batch)
        self.args = args if args is not None else kitti.data_args()
        self.resolution = (int(resolution[0]), int(resolution[1])) if dataset == "kitti" else json3d.RESOLUTION
        self.label_dir = label_dir
        self.mean_sizes = kitti.CLS_MEAN_SIZE if dataset == "kitti" else json3d.CLS_MEAN_SIZE[dataset]
        self.results = {}
        self.n_pictures, self.pictures = int(pictures), []
        self.use_o2m_depth = bool(getattr(self.args, "use_o2m_depth", False) if use_o2m_depth is None else use_o2m_depth)
        self.use_dino_depth = bool(getattr(self.args, "use_dino_depth", False) if use_dino_depth is None else use_dino_depth)
        if depth_fn is not None and not callable(depth_fn):
            raise Y3DError("Validator3d: depth_fn must be a callable, (depth_maps, embeddings) = depth_fn(img)")
        self.depth_fn = depth_fn

    def _rows(self, img):
        return raw_rows3d(self.model, img.permute(0, 3, 1, 2), self.max_det, use_o2m_depth=self.use_o2m_depth)

    def _graph_key(self, img):
        # one hipGraph per shape and state of the switch (off: the shape alone, as before)
        return (tuple(img.shape), "o2m") if self.use_o2m_depth else tuple(img.shape)

    def _depth_callable(self):
        """the depth network of `use_dino_depth`: `depth_fn`, else the callable registered with `loss.set_teacher`"""
        fn = self.depth_fn if self.depth_fn is not None else _loss.get_teacher()
        if fn is None:
            raise Y3DError("use_dino_depth needs a depth map: pass depth_fn to Validator3d or register a callable with "
                           "loss.set_teacher(fn), (depth_maps, embeddings) = fn(img); the DINOv2 teacher itself is not part of this package")
        return fn

    def _dino_depth(self, raw, img, fn):
        """the reference's `elif use_dino_depth` (val.py:57-58, :61-76): eagerly, after the forward (or its replay)"""
        with torch.no_grad():
            depth_maps = fn(img.permute(0, 3, 1, 2))[0]
        return kitti.depth_from_map(raw, depth_maps)

    def _projection(self):
        """-> position -> the original image's P2 (3, 4), next to `_dataset`'s six constants"""
        if isinstance(self.source, (kitti.DeviceSplit, json3d.DeviceSplit)):
            return lambda pos: self.source.P2_host[pos]
        if self.dataset == "kitti":
            data, ids = kitti._split(self.source, "val")
            return lambda pos: kitti.read_calib(os.path.join(data, "calib", f"{ids[pos]:06d}.txt"))
        sp = json3d.read_split(self.source, self.dataset, bool(getattr(self.args, "overfit", False)))
        return lambda pos: sp.P2(sp.ids[pos])

    def _draw(self, b, raw, c6, P2s, ms):
        """the three pictures of one batch, device tensors (nothing is read back here)"""
        n = min(int(b["img"].shape[0]), self.PICTURE_IMGS)
        cam_dis = bool(getattr(self.args, "cam_dis", False))
        P = kitti.p2_device(P2s, int(b["img"].shape[0]), self.device)
        labels = plot.label_pictures(b, c6, P, self.PICTURE_IMGS, ms, cam_dis)
        lrows, lc3, _, lcounts = kitti.decode_batch_device(b, c6, None, False, ms, cam_dis)
        prow, pc3, _, pcounts = predict3d_rows(raw, c6, P, b["ratio_pad"], None, self.PICTURE_CONF, None, ms, cam_dis)
        first = lambda *ts: [t[:n].contiguous() for t in ts]
        affine = plot.ratio_affine(b["ratio_pad"].to(torch.float64), n)
        preds = plot.draw_boxes3d(b["img"][:n].clone(), *first(pc3, prow, pcounts, P), affine)
        plot.draw_labels3d(preds, *first(lrows, lc3, lcounts, P), affine, box2d=False)
        pc3, prow, pcounts, lc3, lcounts = first(pc3, prow, pcounts, lc3, lcounts)
        return {"labels": labels, "preds": preds, "bev": plot.draw_bev(pc3, prow, pcounts, gt=(lc3, lcounts))}

    def _dataset(self):
        """-> (number of images, position -> the original image's (cu, cv, fu, fv, tx, ty), as the reference's get_calib holds them)"""
        if isinstance(self.source, kitti.DeviceSplit):  # resident on the device: ids, calibrations and the label directory from it
            sp = self.source
            return len(sp), lambda pos: kitti.calib_params(sp.P2_host[pos]), sp.data
        if self.dataset == "kitti":
            data, ids = kitti._split(self.source, "val")
            return len(ids), lambda pos: kitti.calib_params(kitti.read_calib(os.path.join(data, "calib", f"{ids[pos]:06d}.txt"))), data
        resident = isinstance(self.source, json3d.DeviceSplit)  # its host tables: the float64 projections as read
        sp = self.source if resident else json3d.read_split(self.source, self.dataset, bool(getattr(self.args, "overfit", False)))

        def calib(pos):
            P = sp.P2_host[pos] if resident else sp.P2(sp.ids[pos])
            return (P[0, 2], P[1, 2], P[0, 0], P[1, 1], P[0, 3] / -P[0, 0], P[1, 3] / -P[1, 1])

        return len(sp), calib, None

    def _batch(self, idx):
        if self.dataset == "kitti":
            return kitti.build_batch(self.source, idx, self.args, self.device, mode="val", compact=True, resolution=self.resolution)
        return json3d.build_batch(self.source, idx, self.args, self.device, dataset=self.dataset, mode="val", compact=True)

    def _run(self):
        dino = self._depth_callable() if self.use_dino_depth and not self.use_o2m_depth else None
        head = self.model.model[-1]
        was, head.eval_one2many = head.eval_one2many, self.use_o2m_depth
        try:
            return self._run_batches(dino)
        finally:
            head.eval_one2many = was

    def _run_batches(self, dino):
        n, calib, data = self._dataset()
        self._start()
        ms = _mean_sizes(self.mean_sizes, self.device)
        files, kept, drawn = [], [], []
        P2_of = self._projection() if self.n_pictures else None
        for s in range(0, n, self.batch):
            idx = list(range(s, min(s + self.batch, n)))
            t0 = self._mark()
            b = self._batch(idx)
            t1 = self._mark()
            raw = self._raw(b["img"])
            if dino is not None:
                raw = self._dino_depth(raw, b["img"], dino)
            t2 = self._mark()
            c6 = metrics._upload(np.array([calib(p) for p in idx], np.float64), self.device)
            inv = metrics._upload(np.stack([np.asarray(i["trans_inv"], np.float64).reshape(2, 3) for i in b["info"]]), self.device)
            rows, keep = kitti.decode_preds_device(raw, c6, b["ratio_pad"], inv, threshold=self.conf, cls_mean_size=ms)
            self.stats.update_3d(rows, keep, b)
            if self.plots:
                self.confusion_matrix.update_3d(rows, keep, b, single_cls=self.single_cls)
            self._events.append((t0, t1, t2, self._mark()))
            files += list(b["im_file"])
            kept.append(torch.cat((rows, keep.unsqueeze(-1).to(rows.dtype)), -1))
            if len(drawn) < self.n_pictures:
                drawn.append(self._draw(b, raw, c6, [P2_of(p) for p in idx], ms))
        self.pictures = [{k: v.cpu().numpy() for k, v in d.items()} for d in drawn]  # the one read-back of the pictures
        self.results = {}
        if kept:  # the one read-back of the rows
            host = torch.cat(kept).cpu()
            self.results = {f: host[i, host[i, :, 14] != 0, :14].tolist() for i, f in enumerate(files)}
        metric3d = 0
        if self.dataset == "kitti":
            metric3d = kitti_eval.get_stats(self.results, self.label_dir or os.path.join(data, "label_2"))
        return self._finish(metric3d)


class Validator2d(_Validator):
    """`DetectionValidator` as the YOLOv10 validator runs it, on a `yolo2d.RectSplit`.

    Per rect batch of `rect_split.batches()`: `yolo2d.build_batch(mode="val")`, the eval forward, `v10postprocess` + `xywh2xyxy`
    (`predict.raw_rows`), `BoxStats.update_2d`, and `ConfusionMatrix.update_2d` when `plots`.  Returns `get_stats(Det3dMetrics(...))`:
    the fork's own validator builds `Det3dMetrics` for the 2D models too, so `metrics/3D` is 0.  `speed` as `Validator3d`."""

    def __init__(self, model, rect_split, args=None, conf=0.001, max_det=300, single_cls=False, plots=True, graph=False):
        super().__init__(model, False, conf, max_det, single_cls, plots, graph)
        if not isinstance(rect_split, yolo2d.RectSplit):
            raise Y3DError("Validator2d: a yolo2d.RectSplit is expected")
        self.split = rect_split
        self.args = args if args is not None else yolo2d.data_args()

    def _rows(self, img):
        return raw_rows(self.model, img.permute(0, 3, 1, 2), self.max_det)

    def _run(self):
        self._start()
        for items in self.split.batches():
            t0 = self._mark()
            b = yolo2d.build_batch(self.split, items, self.args, self.device, mode="val", compact=True)
            t1 = self._mark()
            preds = self._raw(b["img"])
            t2 = self._mark()
            view = {k: v for k, v in b.items() if k != "img"}  # the image is (B, H, W, 3) uint8 here: BoxStats reads the canvas from imgsz
            view["imgsz"] = tuple(int(v) for v in b["resized_shape"][0])
            self.stats.update_2d(preds, view)
            if self.plots:
                self.confusion_matrix.update_2d(preds, view, single_cls=self.single_cls)
            self._events.append((t0, t1, t2, self._mark()))
        return self._finish(0)
