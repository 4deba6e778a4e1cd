"""Mints tests/golden/det_metrics.npz from the REFERENCE's own box metrics, run on the CPU.

    python tools/make_golden_det_metrics.py        # needs the reference checkout (oracle.ref_shim.import_reference)

Importing the reference runs `is_online()` (ultralytics/utils/__init__.py), which opens sockets; this script makes every socket connect
raise OSError BEFORE the import, so nothing leaves the machine.

The inputs are the seeded synthetic sets of tests/det_metrics_sets.py (the tests rebuild them bit for bit), so the fixture holds only
the reference's outputs: tp masks, AP tables, P / R / F1, the recall / precision curves of k3, e3 and every 16th class of c2, and the
results dicts.  The sets, each scored by the reference's validators on stub instances (`object.__new__`, the attributes `update_metrics` /
`get_stats` read):
  * "k3": KITTI-like, 200 images in batches of 8, K = 50 decode rows per image (fp64, a keep mask), 3 classes, through
    YOLOv10_3DDetectionValidator.update_metrics / get_stats (its _prepare_preds / _prepare_batch return dicts built from the rows, the
    targets as decode_batch_eval builds them) with Det3dMetrics and a fixed metrics/3D;
  * "c2": COCO-like, 150 letterboxed 640x640 images of varied ori_shape / ratio_pad in batches of 16, K = 300 rows [xyxy, conf, cls],
    80 classes, through DetectionValidator.update_metrics / get_stats with Det3dMetrics (what the fork's validator builds) and again
    with upstream DetMetrics; "c2s" is the same with single_cls;
  * "e3": hand-made edge cases in the 3D layout: no gts, no kept dets, a class only in gts, a class only in dets, duplicate dets on
    one gt, a det losing its label to a lower-index det; "n3": no true positive anywhere.
Also the reference's box_iou / match_predictions / ap_per_class outputs on the "c2" statistics.

The reference's argsorts are unstable quicksorts, so the script asserts that (1) no two detections of one class share a confidence,
(2) no detection has two class-matched labels with the same IoU >= 0.5, and (3) the smoothed-mean-F1 maximum beats every other index by
more than 1e-9.
"""
from __future__ import annotations

import os
import socket
import sys
import types

import numpy as np
import torch


def _no_network(*a, **k):
    raise OSError("network disabled while minting fixtures")


socket.create_connection = _no_network
socket.socket.connect = _no_network
socket.socket.connect_ex = _no_network

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from det_metrics_sets import input_sets  # noqa: E402
from oracle import ref_shim as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "det_metrics.npz")
META3D = 0.4321  # the fixed metrics/3D the stub dataset reports
CURVES = {"k3": slice(None), "e3": slice(None), "c2": slice(None, None, 16)}  # rows of the p / r curves stored (c2: every 16th)


def load_reference():
    R.import_reference()
    try:
        import sklearn.neighbors  # noqa: F401
    except Exception:
        sk = types.ModuleType("sklearn")
        sk.neighbors = types.ModuleType("sklearn.neighbors")
        sk.neighbors.KernelDensity = object
        sys.modules["sklearn"], sys.modules["sklearn.neighbors"] = sk, sk.neighbors
    from ultralytics.models.yolo.detect.val import DetectionValidator
    from ultralytics.models.yolov10_3D.val import YOLOv10_3DDetectionValidator
    from ultralytics.utils import metrics as M
    from ultralytics.utils import ops
    return DetectionValidator, YOLOv10_3DDetectionValidator, M, ops


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's validators on stub instances
# ------------------------------------------------------------------------------------------------------------------------------
def stub_common(v, M, nc, single_cls, metrics_cls):
    v.args = types.SimpleNamespace(single_cls=single_cls, plots=False, save_json=False, save_txt=False, conf=0.001)
    v.device = torch.device("cpu")
    v.iouv = torch.linspace(0.5, 0.95, 10)
    v.niou = v.iouv.numel()
    v.nc = nc
    v.names = {i: f"c{i}" for i in range(nc)}
    v.metrics = metrics_cls()
    v.metrics.names = v.names
    v.metrics.plot = False
    v.seen = 0
    v.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
    v.confusion_matrix = None


def run_3d(V3, M, ops, batches, nc, single_cls=False):
    v = object.__new__(V3)
    stub_common(v, M, nc, single_cls, M.Det3dMetrics)
    v.results = {}
    v.dataloader = types.SimpleNamespace(dataset=types.SimpleNamespace(get_stats=lambda results, save_dir: META3D))
    v.save_dir = None
    for bi, b in enumerate(batches):
        names = [f"{bi}_{i}.png" for i in range(b["rows"].shape[0])]

        def prep_preds(preds, batch, b=b, names=names):
            return {f: b["rows"][i][b["keep"][i]].tolist() for i, f in enumerate(names)}

        def prep_batch(batch, b=b, names=names):
            out = {}
            for i, f in enumerate(names):
                m = b["batch_idx"] == i
                t = []
                for j in np.flatnonzero(m):
                    bbox = (ops.xywh2xyxy(b["bboxes"][j].copy()) * b["ori_shape"][i][[1, 0, 1, 0]]).tolist()
                    t.append([float(b["cls"][j]), 0.0] + bbox + [0.0] * 7 + [1])
                out[f] = t
            return out

        v._prepare_preds, v._prepare_batch = prep_preds, prep_batch
        v.update_metrics(None, {"im_file": names})
    stats = {k: torch.cat(x, 0).cpu().numpy() for k, x in v.stats.items()}
    res = v.get_stats()
    return v, stats, res


def run_2d(VD, M, batches, nc, single_cls=False, metrics_cls=None):
    v = object.__new__(VD)
    stub_common(v, M, nc, single_cls, metrics_cls or M.Det3dMetrics)
    for b in batches:
        S = int(b["imgsz"][0])
        batch = {"batch_idx": torch.from_numpy(b["batch_idx"]), "cls": torch.from_numpy(b["cls"]), "bboxes": torch.from_numpy(b["bboxes"]),
                 "ori_shape": [tuple(int(x) for x in o) for o in b["ori_shape"]],
                 "ratio_pad": [((float(r[0, 0]), float(r[0, 1])), (float(r[1, 0]), float(r[1, 1]))) for r in b["ratio_pad"]],
                 "img": torch.zeros(1, 1, 1, 1).expand(len(b["preds"]), 3, S, S), "im_file": [""] * len(b["preds"])}
        v.update_metrics(torch.from_numpy(b["preds"].copy()), batch)
    stats = {k: torch.cat(x, 0).cpu().numpy() for k, x in v.stats.items()}
    res = v.get_stats()
    return v, stats, res


# ------------------------------------------------------------------------------------------------------------------------------
def check_ties(stats, M, tag):
    conf, pc = stats["conf"], stats["pred_cls"]
    for c in np.unique(pc):
        s = conf[pc == c]
        assert np.unique(s).size == s.size, f"{tag}: a confidence tie in class {c}"
    if stats["tp"].any():
        f1 = M.ap_per_class(stats["tp"], conf, pc, stats["target_cls"], names={})[9]
        sm = M.smooth(f1.mean(0), 0.1)
        i = sm.argmax()
        rest = np.delete(sm, i)
        assert sm[i] - rest.max() > 1e-9, f"{tag}: the smoothed-F1 maximum is not unique ({sm[i] - rest.max():.3g})"


def check_iou_ties(M, gt_boxes, gt_cls, det_boxes, det_cls, tag):
    iou = M.box_iou(torch.as_tensor(gt_boxes), torch.as_tensor(det_boxes)).numpy()
    iou = iou * (np.asarray(gt_cls)[:, None] == np.asarray(det_cls)[None, :])
    for d in range(iou.shape[1]):
        col = iou[:, d][iou[:, d] >= 0.5]
        assert np.unique(col).size == col.size, f"{tag}: an IoU tie >= 0.5 for det {d}"


def save_result(out, prefix, v, stats, res, tp=True, curves=None):
    m = v.metrics
    if tp:  # (c2d's equal c2's)
        out[f"{prefix}/tp"] = (stats["tp"].astype(np.int16) << np.arange(10, dtype=np.int16)).sum(1).astype(np.int16)  # bit t: iouv[t]
    out[f"{prefix}/results"] = np.array([float(res[k]) for k in m.keys + ["fitness"]])
    out[f"{prefix}/nt_per_class"] = v.nt_per_class
    out[f"{prefix}/seen"] = np.array(v.seen)
    out[f"{prefix}/ap_class_index"] = np.asarray(m.ap_class_index, np.int64)
    if len(m.box.all_ap):
        out[f"{prefix}/all_ap"] = m.box.all_ap
        out[f"{prefix}/p"], out[f"{prefix}/r"], out[f"{prefix}/f1"] = m.box.p, m.box.r, m.box.f1
        out[f"{prefix}/maps"] = m.maps
        if curves is not None:  # rows `curves` of the (nc, 1000) curves (all of them: slice(None))
            out[f"{prefix}/p_curve"], out[f"{prefix}/r_curve"] = m.box.p_curve[curves], m.box.r_curve[curves]


def main():
    VD, V3, M, ops = load_reference()
    out = {}
    inputs = input_sets()
    k3, c2, c2s, e3, n3 = (inputs[k] for k in ("k3", "c2", "c2s", "e3", "n3"))
    # tie-freedom of the inputs (the reference's quicksorts decide nothing)
    for b in k3 + e3 + n3:
        for i in range(b["rows"].shape[0]):
            m = b["batch_idx"] == i
            g = ops.xywh2xyxy(b["bboxes"][m].copy()) * b["ori_shape"][i][[1, 0, 1, 0]]
            d = b["rows"][i][b["keep"][i]]
            check_iou_ties(M, g.astype(np.float32), b["cls"][m], d[:, 2:6].astype(np.float32), d[:, 0], "3d")
    for b in c2:
        for i in range(b["preds"].shape[0]):
            m = b["batch_idx"] == i
            rp = ((b["ratio_pad"][i, 0, 0], b["ratio_pad"][i, 0, 1]), tuple(b["ratio_pad"][i, 1]))
            g = ops.xywh2xyxy(torch.from_numpy(b["bboxes"][m])) * 640.0
            ops.scale_boxes((640, 640), g, tuple(b["ori_shape"][i]), ratio_pad=rp)
            d = torch.from_numpy(b["preds"][i].copy())
            ops.scale_boxes((640, 640), d[:, :4], tuple(b["ori_shape"][i]), ratio_pad=rp)
            check_iou_ties(M, g, b["cls"][m].reshape(-1), d[:, :4], d[:, 5].numpy(), "2d")
            check_iou_ties(M, g, np.zeros(int(m.sum())), d[:, :4], np.zeros(len(d)), "2d single_cls")
    for name, sets, fn in (("k3", k3, lambda s: run_3d(V3, M, ops, s, 3)), ("e3", e3, lambda s: run_3d(V3, M, ops, s, 4)),
                           ("n3", n3, lambda s: run_3d(V3, M, ops, s, 3)), ("c2", c2, lambda s: run_2d(VD, M, s, 80)),
                           ("c2s", c2s, lambda s: run_2d(VD, M, s, 80, single_cls=True)),
                           ("c2d", c2, lambda s: run_2d(VD, M, s, 80, metrics_cls=M.DetMetrics))):
        v, stats, res = fn(sets)
        check_ties(stats, M, name)
        if name == "c2":
            c2_stats = stats
        save_result(out, name, v, stats, res, tp=name != "c2d", curves=CURVES.get(name))
        print(name, {k: round(float(x), 6) for k, x in res.items()})
    assert not out["n3/tp"].any() and out["e3/tp"].any()
    # the drop-ins on the c2 statistics and on the first c2 image
    st = c2_stats
    r = M.ap_per_class(st["tp"], st["conf"], st["pred_cls"], st["target_cls"], names={})
    for i, k in enumerate(("tp", "fp", "p", "r", "f1", "ap", "unique_classes")):
        out[f"apc/{k}"] = np.asarray(r[i])
    b = c2[0]
    m = b["batch_idx"] == 0
    S = 640
    gt = ops.xywh2xyxy(torch.from_numpy(b["bboxes"][m])) * torch.tensor([S, S, S, S])
    ops.scale_boxes((S, S), gt, tuple(b["ori_shape"][0]), ratio_pad=((b["ratio_pad"][0, 0, 0], b["ratio_pad"][0, 0, 1]), tuple(b["ratio_pad"][0, 1])))
    det = torch.from_numpy(b["preds"][0].copy())
    ops.scale_boxes((S, S), det[:, :4], tuple(b["ori_shape"][0]), ratio_pad=((b["ratio_pad"][0, 0, 0], b["ratio_pad"][0, 0, 1]), tuple(b["ratio_pad"][0, 1])))
    out["one/gt"], out["one/gt_cls"], out["one/det"] = gt.numpy(), b["cls"][m].reshape(-1), det.numpy()
    out["one/iou"] = M.box_iou(gt, det[:, :4]).numpy()
    v = object.__new__(VD)
    v.iouv = torch.linspace(0.5, 0.95, 10)
    out["one/tp"] = v.match_predictions(det[:, 5], torch.from_numpy(b["cls"][m].reshape(-1)), M.box_iou(gt, det[:, :4])).numpy()
    # small boxes (normalised coordinates), where the place of the 1e-7 in box_iou's denominator shows in the rounding
    a, b = inputs["tiny"]
    out["tiny/iou"] = M.box_iou(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
