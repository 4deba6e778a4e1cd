"""GPU: the one-call validators (val.py) against a hand-stitched loop of the calls they are made of, bit for bit: `Validator3d` on the
synthetic KITTI tree of tests/kitti_labels_tree.py with a tiny 3D model (320 x 256: 80 cells on the coarsest level for max_det = 50;
five frames in batches of two, so the last batch is short), eagerly and replayed from a hipGraph; `Validator2d` on the rect tree of
tests/yolo2d_tree.py with a tiny v10 model."""
import os

import numpy as np
import pytest
import torch

import yolo2d_tree as T2
from kitti_labels_tree import fixture as tree_fixture, write_tree

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, kitti_eval, metrics, predict, val, yolo2d
from yolov10_3d_amd import loss as PL
from yolov10_3d_amd import ops as P_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = (320, 256)
FRAMES = [0, 2, 6, 7, 9]  # 1242 x 375, 1224 x 370 and 1238 x 374
KEYS = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "metrics/3D", "fitness"]


@pytest.fixture(autouse=True)
def _float32_compute():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    yield
    y3d.set_compute_dtype(before)


def _prime(m, shape, branches):
    """as tests/test_hip_letterbox.py: BatchNorm statistics of a random batch and wider random score projections, so that the scores
    of the random model differ"""
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    keep = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m.train()(torch.rand(*shape, device=DEV))
        for branch in branches(m.model[-1]):
            for level in branch:
                level[-1].weight.normal_(0.0, 0.05)
                level[-1].bias.add_(torch.randn_like(level[-1].bias))
    for b, mom in zip(bns, keep):
        b.momentum = mom
    P_ops.bump_param_epoch()
    return m


# ---------------------------------------------------------------------------------------------------------------- 3D
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = write_tree(str(tmp_path_factory.mktemp("kitti_val")), tree_fixture(), images=True)
    open(os.path.join(r, "ImageSets", "val.txt"), "w").write("".join(f"{i:06d}\n" for i in FRAMES))
    return r


@pytest.fixture(scope="module")
def model3d():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml")).to(DEV)
    _prime(m, (2, 3, RES[1], RES[0]), lambda head: (head.cls, head.dep_un))
    y3d.set_compute_dtype(before)
    return m.train()  # left in training mode: the validators must restore it


def _raw3d(model, img):
    with torch.no_grad():
        y = model(img.permute(0, 3, 1, 2))["one2one"][0]
        reg, sc, lab = PL.v10_3Dpostprocess(y.permute(0, 2, 1), 50, 3)
    return torch.cat((reg, sc.unsqueeze(-1), lab.unsqueeze(-1)), -1).float()


@pytest.fixture(scope="module")
def conf3d(root, model3d):
    """a threshold inside the scores of the random model, so that the keep mask does something"""
    y3d.set_compute_dtype(torch.float32)
    b = kitti.build_batch(root, [0, 1], kitti.data_args(), DEV, mode="val", resolution=RES)
    raw = _raw3d(model3d.eval(), b["img"])
    model3d.train()
    sc = raw[..., 35].reshape(-1)
    rows, _ = kitti.decode_preds_device(raw, b["calib"], b["ratio_pad"], [i["trans_inv"] for i in b["info"]], threshold=0.0)
    conf = float(rows[..., 13].reshape(-1).median())
    print(f"decoded scores {float(rows[..., 13].min()):.6g} .. {float(rows[..., 13].max()):.6g}, threshold {conf:.6g}, class scores to {float(sc.max()):.6g}")
    return conf


@pytest.fixture(scope="module")
def stitched3d(root, model3d, conf3d):
    """the existing calls, by hand"""
    y3d.set_compute_dtype(torch.float32)
    model3d.eval()
    stats, cm, results = metrics.BoxStats(3, device=DEV), metrics.ConfusionMatrix(3, conf=conf3d, device=DEV), {}
    for s in range(0, len(FRAMES), 2):
        idx = list(range(s, min(s + 2, len(FRAMES))))
        b = kitti.build_batch(root, idx, kitti.data_args(), DEV, mode="val", compact=True, resolution=RES)
        raw = _raw3d(model3d, b["img"])
        calib = torch.tensor([kitti.calib_params(kitti.read_calib(os.path.join(root, "training/calib", f"{FRAMES[p]:06d}.txt"))) for p in idx],
                             dtype=torch.float64)
        inv = [i["trans_inv"] for i in b["info"]]
        rows, keep = kitti.decode_preds_device(raw, calib, b["ratio_pad"], inv, threshold=conf3d)
        stats.update_3d(rows, keep, b)
        cm.update_3d(rows, keep, b)
        results.update(kitti.decode_preds(raw, calib, b["im_file"], b["ratio_pad"], inv, threshold=conf3d))
    model3d.train()
    ap3d = kitti_eval.get_stats(results, os.path.join(root, "training", "label_2"))
    m = metrics.Det3dMetrics(names=model3d.names)
    res = stats.get_stats(m, ap3d)
    return dict(res=res, results=results, seen=stats.seen, nt=stats.nt_per_class, matrix=cm.matrix, ap3d=ap3d)


def _same(v, res, want):
    assert list(res) == KEYS and list(want["res"]) == KEYS
    assert [float(res[k]) for k in KEYS] == [float(want["res"][k]) for k in KEYS]
    assert v.seen == want["seen"] and np.array_equal(v.nt_per_class, want["nt"])
    assert v.confusion_matrix.matrix.tobytes() == want["matrix"].tobytes()
    assert v.metrics.confusion_matrix is v.confusion_matrix and v.metrics.speed is v.speed
    assert list(v.speed) == ["preprocess", "inference", "loss", "postprocess"] and v.speed["loss"] == 0.0
    assert all(v.speed[k] > 0 for k in ("preprocess", "inference", "postprocess"))


def test_validator3d_equals_the_hand_stitched_loop(root, model3d, conf3d, stitched3d):
    v = val.Validator3d(model3d, root, batch=2, conf=conf3d, resolution=RES)
    assert model3d.training
    res = v()
    assert model3d.training  # the mode is restored
    _same(v, res, stitched3d)
    assert list(v.results) == [f"{i:06d}.txt" for i in FRAMES] and v.results == stitched3d["results"]
    n = sum(len(r) for r in v.results.values())
    assert 0 < n < 50 * len(FRAMES) and v.seen == len(FRAMES) and v.nt_per_class.sum() > 0
    assert float(res["metrics/3D"]) == float(stitched3d["ap3d"]) == float(kitti_eval.get_stats(v.results, os.path.join(root, "training", "label_2")))
    assert v.confusion_matrix.matrix[3].sum() + v.confusion_matrix.matrix[:3, :3].sum() == v.nt_per_class.sum()  # every gt is counted once
    # a split file instead of the root, an explicit label directory, eval mode kept, no confusion matrix
    model3d.eval()
    w = val.Validator3d(model3d, os.path.join(root, "ImageSets", "val.txt"), batch=5, conf=conf3d, resolution=RES, plots=False,
                        label_dir=os.path.join(root, "training", "label_2"))
    res5 = w()
    assert not model3d.training
    model3d.train()
    assert w.results == v.results and float(res5["metrics/3D"]) == float(res["metrics/3D"]) and w.confusion_matrix.matrix.sum() == 0
    np.testing.assert_array_equal(w.nt_per_class, v.nt_per_class)


def test_validator3d_graph_equals_eager(root, model3d, conf3d, stitched3d):
    v = val.Validator3d(model3d, root, batch=2, conf=conf3d, resolution=RES, graph=True)
    res = v()
    assert model3d.training
    _same(v, res, stitched3d)
    assert v.results == stitched3d["results"]
    assert sorted(v._graphs) == [(1, RES[1], RES[0], 3), (2, RES[1], RES[0], 3)] and all(g.captures == 1 for g in v._graphs.values())


# ---------------------------------------------------------------------------------------------------------------- 2D
NC2, IMGSZ, STRIDE, PAD = 20, 64, 32, 0.5


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    img_dir = T2.write_tree(str(tmp_path_factory.mktemp("rect_val")), T2.fixture()["label_text"])
    return yolo2d.RectSplit(img_dir, IMGSZ, 5, STRIDE, PAD)  # 12 images: batches of 5, 5 and 2


@pytest.fixture(scope="module")
def model2d():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=NC2, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    torch.manual_seed(3)
    m = y3d.YOLOv10DetectionModel(cfg).to(DEV)
    _prime(m, (4, 3, IMGSZ, IMGSZ), lambda head: (head.one2one_cv3,))
    y3d.set_compute_dtype(before)
    return m.train()


def test_validator2d_equals_the_hand_stitched_loop(split, model2d):
    model2d.eval()
    stats, cm = metrics.BoxStats(NC2, device=DEV), metrics.ConfusionMatrix(NC2, conf=0.001, device=DEV)
    shapes = set()
    for items in split.batches():
        b = yolo2d.build_batch(split, items, yolo2d.data_args(), DEV, mode="val", compact=True)
        with torch.no_grad():
            preds = predict.raw_rows(model2d, b["img"].permute(0, 3, 1, 2), 40)
        one = {k: b[k] for k in ("cls", "bboxes", "batch_idx", "ori_shape", "ratio_pad")}
        one["imgsz"] = b["resized_shape"][0]
        shapes.add(tuple(one["imgsz"]))
        stats.update_2d(preds, one)
        cm.update_2d(preds, one)
    model2d.train()
    m = metrics.Det3dMetrics(names=model2d.names)
    want = dict(res=stats.get_stats(m), seen=stats.seen, nt=stats.nt_per_class, matrix=cm.matrix)
    assert len(shapes) > 1 and want["seen"] == 12 and want["nt"].sum() > 0
    assert want["matrix"][NC2].sum() + want["matrix"][:NC2, :NC2].sum() == want["nt"].sum()  # every gt is counted once
    for graph in (False, True):
        v = val.Validator2d(model2d, split, max_det=40, graph=graph)
        res = v()
        assert model2d.training
        _same(v, res, want)
        assert float(res["metrics/3D"]) == 0.0 and v.confusion_matrix.conf == 0.25
    with pytest.raises(y3d.Y3DError, match="RectSplit"):
        val.Validator2d(model2d, os.path.dirname(split.im_files[0]))  # a directory is not a split
