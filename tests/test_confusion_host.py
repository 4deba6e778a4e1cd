"""Host: the confusion matrix's two-argmax rule (tests/confusion_ref.py) against the reference's own matrices
(tests/golden/confusion.npz, minted by tools/make_golden_confusion.py), against the reference's statements with stable sorts where ties
occur, against the reference itself where its checkout exists; the ABI prototypes; the argument checks of `metrics.ConfusionMatrix` and
the validators."""
import os

import numpy as np
import pytest
import torch

import confusion_ref as CR
from conftest import GOLDEN
from det_metrics_sets import SplitMix64, jitter

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib, metrics, val, yolo2d


def golden():
    return np.load(os.path.join(GOLDEN, "confusion.npz"))


@pytest.mark.parametrize("name", list(CR.SETS))
def test_restatement_reproduces_the_reference_matrices(name):
    src, nc, single_cls = CR.SETS[name]
    want = golden()[name]
    assert want.shape == (nc + 1, nc + 1) and want.dtype == np.int32
    np.testing.assert_array_equal(CR.validator_matrix(CR.batches_of(src), nc, single_cls), want)


def test_fixture_covers_the_edges():
    z = golden()
    x3, n3 = z["x3"], z["n3"]
    assert n3[:3].sum() == 0 and n3[3].tolist() == [1, 1, 1, 0]  # no match anywhere: the gts are missed, the detections not counted
    assert x3[1, 1] == 1 and x3[2, 4] == 1 and x3[4, 2] == 1     # image 2: the loser is predicted background, its second gt missed
    assert x3[2, 0] == 1                                         # image 3: a wrong-class match is off the diagonal
    assert z["k3"][:3, :3].sum() > 0 and z["c2"].sum() == z["c2s"].sum()


def random_image(rng, nc, grid=None):
    """one image: gts and jittered / random detections; with `grid`, coordinates snapped to it so that IoU ties occur"""
    g, gc = [], []
    for _ in range(rng.integers(1, 7)):
        x1, y1 = rng.uniform(0, 500), rng.uniform(0, 300)
        g.append([x1, y1, x1 + rng.uniform(20, 150), y1 + rng.uniform(20, 90)])
        gc.append(rng.integers(0, nc))
    g = np.array(g)
    d = [jitter(rng, g[rng.integers(0, len(g))], rng.uniform(0.01, 0.3)) for _ in range(rng.integers(0, 12))]
    d += [[x, y, x + rng.uniform(15, 100), y + rng.uniform(15, 60)] for x, y in ((rng.uniform(0, 550), rng.uniform(0, 330)) for _ in range(rng.integers(0, 4)))]
    d = np.array(d, np.float64).reshape(-1, 4)
    if grid:
        g, d = np.round(g / grid) * grid, np.round(d / grid) * grid
        d[:, 2:] = np.maximum(d[:, 2:], d[:, :2] + grid)
    cf = rng.uniform(0.0, 1.0, len(d)).astype(np.float32).reshape(-1)
    dc = np.array([rng.integers(0, nc) for _ in range(len(d))], np.int64)
    return g.astype(np.float32), np.array(gc, np.int64), d.astype(np.float32), cf, dc


def test_two_argmax_equals_the_stable_sorted_statements_with_ties():
    rng = SplitMix64(99)
    ties = 0
    for n in range(300):
        g, gc, d, cf, dc = random_image(rng, 3, grid=25.0)
        if not len(d):
            continue
        a, b = np.zeros((4, 4), np.int64), np.zeros((4, 4), np.int64)
        CR.process_batch(a, d, cf, dc, g, gc)
        CR.literal(b, d, cf, dc, g, gc)
        np.testing.assert_array_equal(a, b, err_msg=f"image {n}")
        iou = CR.iou_f32(g, d[cf > np.float32(CR.CONF)])
        iou = iou[iou > np.float32(CR.IOU_THRES)]
        ties += int(np.unique(iou).size < iou.size)
    assert ties > 20  # the tie rules were exercised


def test_restatement_equals_the_reference_on_seeded_images(monkeypatch):
    from oracle import ref_shim as R
    if not R.available():
        pytest.skip("the reference checkout is not on this machine")
    import socket

    def no_network(*a, **k):
        raise OSError("network disabled")

    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setattr(socket.socket, "connect_ex", no_network)
    monkeypatch.setenv("YOLO_OFFLINE", "1")
    import sys
    modules, path = set(sys.modules), list(sys.path)
    try:
        R.import_reference()
        from ultralytics.utils.metrics import ConfusionMatrix
        _compare_with(ConfusionMatrix)
    finally:  # leave the session as it was: the reference package and the shim's inert stand-ins for its optional imports go again
        for k in set(sys.modules) - modules:
            m = sys.modules[k]
            if k.split(".")[0] == "ultralytics" or (getattr(m, "__file__", None) is None and getattr(m, "__path__", None) == []):
                del sys.modules[k]
        sys.path[:] = path
        R._IMPORTED = None


def _compare_with(ConfusionMatrix):
    rng = SplitMix64(4242)
    nc, counted = 5, 0
    for n in range(200):
        g, gc, d, cf, dc = random_image(rng, nc)
        if n % 17 == 0:
            g, gc = g[:0], gc[:0]
        iou = CR.iou_f32(g, d[cf > np.float32(CR.CONF)])
        above = iou[iou > np.float32(CR.IOU_THRES)]
        assert np.unique(above).size == above.size  # the reference's unstable sorts decide nothing
        ref = ConfusionMatrix(nc=nc, conf=0.001)
        det = torch.from_numpy(np.concatenate((d, cf[:, None], dc[:, None].astype(np.float32)), 1)) if (len(d) or n % 2) else None
        ref.process_batch(det, torch.from_numpy(g), torch.from_numpy(gc))
        mine = np.zeros((nc + 1, nc + 1), np.int64)
        CR.process_batch(mine, None if det is None else d, None if det is None else cf, None if det is None else dc, g, gc)
        np.testing.assert_array_equal(mine, ref.matrix.astype(np.int64), err_msg=f"image {n}")
        counted += int(mine.sum())
    assert counted > 500


def test_prototypes_declared():
    protos = _lib.parse_header()
    import ctypes
    for name, nargs in (("y3d_confusion_batch", 19), ("y3d_confusion_image", 12)):
        ret, args = protos[name]
        assert ret is ctypes.c_int and len(args) == nargs
    b = protos["y3d_confusion_batch"][1]
    assert b[0] is ctypes.c_int and b[1] is ctypes.c_void_p and b[13] is ctypes.c_int and b[14] is ctypes.c_double and b[15] is ctypes.c_double
    i = protos["y3d_confusion_image"][1]
    assert i[2] is ctypes.c_int and i[3] is ctypes.c_void_p and i[7] is ctypes.c_double and i[8] is ctypes.c_double
    assert hasattr(y3d.lib()._dll, "y3d_confusion_batch") and hasattr(y3d.lib()._dll, "y3d_confusion_image")


def test_confusion_matrix_arguments():
    assert metrics.ConfusionMatrix(3, conf=0.001).conf == 0.25 and metrics.ConfusionMatrix(3, conf=None).conf == 0.25
    assert metrics.ConfusionMatrix(3, conf=0.5).conf == 0.5 and metrics.ConfusionMatrix(3).iou_thres == 0.45
    with pytest.raises(y3d.Y3DError, match="classify"):
        metrics.ConfusionMatrix(3, task="classify")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        metrics.ConfusionMatrix(3, device="cpu")
    with pytest.raises(y3d.Y3DError, match="plot"):
        metrics.ConfusionMatrix(3).plot()
    with pytest.raises(y3d.Y3DError, match="negative"):
        metrics.ConfusionMatrix(3, iou_thres=-0.1)
    cm = metrics.ConfusionMatrix(3)
    with pytest.raises(y3d.Y3DError, match="device tensors"):
        cm.process_batch(torch.zeros(2, 6), torch.zeros(1, 4), torch.zeros(1))
    with pytest.raises(y3d.Y3DError, match=r"\(B, K, 6\)"):
        cm.update_2d(torch.zeros(1, 4, 5), {})
    with pytest.raises(y3d.Y3DError, match="at most"):
        cm.update_3d(torch.zeros(1, metrics.max_dets() + 1, 14), torch.ones(1, metrics.max_dets() + 1, dtype=torch.bool), {})


def _tiny(kind):
    if kind == "3d":
        return y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml"))
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=4, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    return y3d.YOLOv10DetectionModel(cfg)


def test_validators_refuse_the_wrong_model_and_the_host():
    m3, m2 = _tiny("3d"), _tiny("2d")
    with pytest.raises(y3d.Y3DError, match="3D model is expected"):
        val.Validator3d(m2, "/nowhere")
    with pytest.raises(y3d.Y3DError, match="2D model is expected"):
        val.Validator2d(m3, None)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        val.Validator3d(m3, "/nowhere")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        val.Validator2d(m2, None)
    assert m3.training and m2.training
    assert issubclass(yolo2d.RectSplit, yolo2d.Split)
