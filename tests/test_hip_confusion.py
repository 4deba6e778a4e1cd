"""GPU: the confusion matrix (csrc/det_metrics.hip `y3d_confusion_batch` / `y3d_confusion_image`, metrics.ConfusionMatrix) against the
reference's own matrices (tests/golden/confusion.npz) and, at the smallest shapes where the kernel can go wrong, against the numpy
restatement of tests/confusion_ref.py.  Every comparison is exact integer equality."""
import functools

import numpy as np
import pytest
import torch

import confusion_ref as CR
from test_confusion_host import golden

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import metrics as DM  # noqa: E402

DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def feed(cm, batches, single_cls=False):
    """the set through update_3d / update_2d as a validator would"""
    for b in batches:
        batch = {"batch_idx": t(b["batch_idx"]), "cls": t(b["cls"].reshape(-1, 1)), "bboxes": t(b["bboxes"]),
                 "ori_shape": [tuple(int(v) for v in o) for o in b["ori_shape"]]}
        if "rows" in b:
            cm.update_3d(t(b["rows"]), t(b["keep"]), batch, single_cls=single_cls)
        else:
            batch["ratio_pad"] = [((float(r[0, 0]), float(r[0, 1])), (float(r[1, 0]), float(r[1, 1]))) for r in b["ratio_pad"]]
            batch["imgsz"] = tuple(int(v) for v in b["imgsz"])
            cm.update_2d(t(b["preds"]), batch, single_cls=single_cls)
    return cm


@functools.lru_cache(maxsize=None)
def device_matrix(name):
    src, nc, single_cls = CR.SETS[name]
    m = feed(DM.ConfusionMatrix(nc, conf=0.001), CR.batches_of(src), single_cls).matrix
    assert m.dtype == np.float64 and m.shape == (nc + 1, nc + 1)
    return m


def exact(got, want):
    assert np.array_equal(got, np.round(got))
    np.testing.assert_array_equal(got.astype(np.int64), np.asarray(want).astype(np.int64))


@pytest.mark.parametrize("name", ["k3", "x3", "n3", "c2", "c2s"])
def test_batched_updates_equal_the_reference(name):
    exact(device_matrix(name), golden()[name])
    if name == "n3":  # no match anywhere: the detections are not counted
        assert device_matrix(name)[:3].sum() == 0


@pytest.mark.parametrize("name", ["k3", "c2"])
def test_drop_in_image_by_image_equals_the_batched_path(name):
    src, nc, single_cls = CR.SETS[name]
    cm = DM.ConfusionMatrix(nc, conf=0.001)
    for b in CR.batches_of(src):
        n = len(b["rows"]) if "rows" in b else len(b["preds"])
        for i in range(n):
            g, gc, box, cf, dc = (CR.prep_3d if "rows" in b else CR.prep_2d)(b, i)
            if not len(gc):
                continue  # `if nl:` of both validators
            if "rows" in b:  # float64 rows: the confidence is compared in float64
                d = b["rows"][i][b["keep"][i]]
                det = np.concatenate((d[:, 2:6], d[:, 13:14], d[:, 0:1]), 1)
            else:
                det = np.concatenate((box, cf[:, None], dc[:, None].astype(np.float32)), 1)
            cm.process_batch(t(det) if len(det) else None, t(g), t(gc))
    exact(cm.matrix, device_matrix(name))
    tp, fp = cm.tp_fp()
    exact(tp, np.diag(golden()[name])[:-1])
    exact(fp, golden()[name].sum(1)[:-1] - np.diag(golden()[name])[:-1])


# ---------------------------------------------------------------------------------------------------------------- small shapes
H0, W0 = 512, 1024  # powers of two: integer pixel coordinates survive the normalised xywh round trip exactly


def mk3(images, K=None):
    """images: [(gts [(cls, x1, y1, x2, y2)], dets [(cls, box, score, kept)])] -> one batch in the 3D layout of det_metrics_sets"""
    K = K if K is not None else max([len(d) for _, d in images] + [1])
    rows, keep = np.zeros((len(images), K, 14)), np.zeros((len(images), K), bool)
    bidx, cls, boxes = [], [], []
    for i, (gts, dets) in enumerate(images):
        for c, x1, y1, x2, y2 in gts:
            bidx.append(i)
            cls.append(c)
            boxes.append([(x1 + x2) / 2 / W0, (y1 + y2) / 2 / H0, (x2 - x1) / W0, (y2 - y1) / H0])
        for k, (c, box, score, kept) in enumerate(dets):
            rows[i, k, 0], rows[i, k, 2:6], rows[i, k, 13], keep[i, k] = c, box, score, kept
    return dict(rows=rows, keep=keep, batch_idx=np.array(bidx, np.float32), cls=np.array(cls, np.float32),
                bboxes=np.array(boxes, np.float32).reshape(-1, 4), ori_shape=np.array([[H0, W0]] * len(images), np.int64))


def both(batches, nc, conf=0.001, iou_thres=0.45):
    cm = feed(DM.ConfusionMatrix(nc, conf=conf, iou_thres=iou_thres), batches)
    want = CR.validator_matrix(batches, nc, conf=cm.conf, iou_thres=iou_thres)
    got = cm.matrix
    exact(got, want)
    return got.astype(np.int64)


A, B_ = (128, 128, 256, 256), (160, 128, 288, 256)


def test_one_class_and_empty_images():
    m = both([mk3([([(0,) + A], [(0, [130, 128, 258, 256], 0.9, True), (0, [600, 300, 700, 400], 0.8, True)]),   # a match and a background
                   ([(0,) + A, (0,) + B_], [(0, list(A), 0.9, False), (0, list(B_), 0.9, False)]),                # gts, K rows, none kept
                   ([], [(0, list(A), 0.9, True)]),                                                                # no gts: skipped
                   ([], [])])], nc=1)
    assert m.tolist() == [[1, 1], [2, 0]]
    # K = 0: every gt is missed
    b = mk3([([(0,) + A], [])])
    b["rows"], b["keep"] = b["rows"][:, :0], b["keep"][:, :0]
    assert both([b], nc=1).tolist() == [[0, 0], [1, 0]]


def test_strict_thresholds():
    one = mk3([([(1,) + A], [(2, [136, 128, 264, 256], 0.9, True)])])
    g, _, box, _, _ = CR.prep_3d(one, 0)
    v = CR.iou_f32(g, box)[0, 0]
    assert v.dtype == np.float32 and 0.8 < v < 0.95
    assert both([one], 3, iou_thres=float(v)).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]  # IoU == threshold: no match
    below = float(np.nextafter(v, np.float32(0)))  # the IoU is one ulp above the threshold
    assert both([one], 3, iou_thres=below).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    # confidence: a row at the threshold is excluded; float64 rows are compared in float64
    dets = [(0, list(A), 0.25, True), (1, [600, 300, 700, 400], np.nextafter(0.25, 1.0), True), (2, [700, 300, 800, 400], 0.2, True)]
    m = both([mk3([([(0,) + A, (1, 600, 300, 700, 400)], dets)])], 3)
    assert m[1, 1] == 1 and m[3, 0] == 1 and m.sum() == 2
    m = both([mk3([([(0,) + A], dets[:1] + dets[2:])])], 3, conf=0.2)  # an explicit threshold is taken as given: 0.25 > 0.2, 0.2 is not
    assert m[0, 0] == 1 and m.sum() == 1
    # 2D rows: float32 confidences against float32(conf)
    preds = np.zeros((1, 3, 6), np.float32)
    preds[0, :, :4] = [list(A), [600, 300, 700, 400], [10, 10, 50, 50]]
    preds[0, :, 4] = [0.25, np.nextafter(np.float32(0.25), np.float32(1)), 0.9]
    preds[0, :, 5] = [0, 1, 2]
    b2 = dict(preds=preds, batch_idx=np.zeros(2, np.float32), cls=np.array([[0], [1]], np.float32),
              bboxes=np.array([[192 / W0, 192 / H0, 128 / W0, 128 / H0], [650 / W0, 350 / H0, 100 / W0, 100 / H0]], np.float32),
              ori_shape=np.array([[H0, W0]], np.int64), ratio_pad=np.array([[[1.0, 1.0], [0.0, 0.0]]]), imgsz=np.array([H0, W0], np.int64))
    m = both([b2], 3)
    assert m[1, 1] == 1 and m[3, 0] == 1 and m[2, 3] == 1 and m.sum() == 3


def test_the_loser_does_not_fall_back():
    # both dets prefer A; det 1 loses A and is predicted background although it overlaps B above the threshold; B is missed
    m = both([mk3([([(1,) + A, (2,) + B_], [(1, [130, 128, 258, 256], 0.9, True), (0, [140, 128, 268, 256], 0.8, True)])])], 3)
    assert m[1, 1] == 1 and m[0, 3] == 1 and m[3, 2] == 1 and m.sum() == 3


def test_documented_tie_rules():
    # a detection midway between two gts: equal IoU, the higher gt index wins
    img = ([(0,) + A, (1,) + B_], [(2, [144, 128, 272, 256], 0.9, True)])
    g, _, box, _, _ = CR.prep_3d(mk3([img]), 0)
    iou = CR.iou_f32(g, box)
    assert iou[0, 0] == iou[1, 0] > 0.45
    m = both([mk3([img])], 3)
    assert m[2, 1] == 1 and m[3, 0] == 1 and m.sum() == 2
    # two detections with equal IoU on one gt: the higher detection index wins, the other is predicted background
    img = ([(0,) + A], [(1, [144, 128, 272, 256], 0.9, True), (2, [112, 128, 240, 256], 0.8, True)])
    g, _, box, _, _ = CR.prep_3d(mk3([img]), 0)
    iou = CR.iou_f32(g, box)
    assert iou[0, 0] == iou[0, 1] > 0.45
    m = both([mk3([img])], 3)
    assert m[2, 0] == 1 and m[1, 3] == 1 and m.sum() == 2
    # the same two through the drop-in
    cm = DM.ConfusionMatrix(3)
    cm.process_batch(t(np.array([[144, 128, 272, 256, 0.9, 2]], np.float32)), t(np.array([A, B_], np.float32)), t(np.array([0, 1])))
    cm.process_batch(t(np.array([[144, 128, 272, 256, 0.9, 1], [112, 128, 240, 256, 0.8, 2]], np.float32)), t(np.array([A], np.float32)), t(np.array([0])))
    m = cm.matrix
    assert m[2, 1] == 1 and m[3, 0] == 1 and m[2, 0] == 1 and m[1, 3] == 1 and m.sum() == 4


def test_drop_in_edges():
    cm = DM.ConfusionMatrix(2, conf=0.3)
    none = torch.zeros(0, device=DEV)
    cm.process_batch(t(np.array([[1, 1, 9, 9, 0.9, 1], [1, 1, 9, 9, 0.3, 0]], np.float32)), torch.zeros(0, 4, device=DEV), none)  # no gts: false positives
    cm.process_batch(None, torch.zeros(0, 4, device=DEV), none)                                                                  # nothing
    cm.process_batch(None, t(np.array([A], np.float32)), t(np.array([1.0])))                                                     # detections=None
    cm.process_batch(torch.zeros(0, 6, device=DEV), t(np.array([A], np.float32)), t(np.array([0.0])))                            # no rows
    assert cm.matrix.tolist() == [[0, 0, 0], [0, 0, 1], [1, 1, 0]]
    cm.reset()
    assert cm.matrix.sum() == 0
    cm.process_batch(t(np.array([[1, 1, 9, 9, 0.9, 2]], np.float32)), t(np.array([A], np.float32)), t(np.array([0])))  # class 2 of 2
    with pytest.raises(y3d.Y3DError, match="outside"):
        cm.matrix


@functools.lru_cache(maxsize=None)
def full_image():
    """K = max_dets() rows and max_gts() gts in one image, and a second ordinary image"""
    from det_metrics_sets import SplitMix64, jitter
    rng = SplitMix64(5)
    G, K = DM.max_gts(), DM.max_dets()
    gts, dets = [], []
    for _ in range(G):
        x1, y1 = rng.uniform(0, 900), rng.uniform(0, 440)
        gts.append((rng.integers(0, 3), x1, y1, x1 + rng.uniform(20, 120), y1 + rng.uniform(20, 70)))
    for k in range(K):
        box = jitter(rng, np.array(gts[rng.integers(0, G)][1:]), rng.uniform(0.01, 0.2))
        dets.append((rng.integers(0, 3), list(box), rng.uniform(0.0, 1.0), rng.random() < 0.9))
    other = ([(1,) + A], [(1, [130, 128, 258, 256], 0.9, True)])
    return gts, dets, other


def test_limits():
    gts, dets, other = full_image()
    m = both([mk3([(gts, dets), other])], 3)
    assert m[:3, :3].sum() > 100 and m[:3, 3].sum() > 100
    # one gt too many: that image adds nothing, the matrix refuses to be read, the other image is counted
    cm = feed(DM.ConfusionMatrix(3), [mk3([(gts + [gts[0]], dets), other])])
    with pytest.raises(y3d.Y3DError, match=f"{DM.max_gts() + 1} gts"):
        cm.matrix
    assert cm._m.cpu().numpy().tolist() == CR.validator_matrix([mk3([other])], 3).tolist()


def merge(a, b):
    n = len(a["rows"])
    return dict(rows=np.concatenate((a["rows"], b["rows"])), keep=np.concatenate((a["keep"], b["keep"])),
                batch_idx=np.concatenate((a["batch_idx"], b["batch_idx"] + n)), cls=np.concatenate((a["cls"], b["cls"])),
                bboxes=np.concatenate((a["bboxes"], b["bboxes"])), ori_shape=np.concatenate((a["ori_shape"], b["ori_shape"])))


def test_accumulation_and_determinism():
    k3 = CR.batches_of("k3")
    two = feed(DM.ConfusionMatrix(3, conf=0.001), k3[:2]).matrix
    one = feed(DM.ConfusionMatrix(3, conf=0.001), [merge(k3[0], k3[1])]).matrix
    assert two.sum() > 100
    exact(two, one)
    again = feed(DM.ConfusionMatrix(3, conf=0.001), CR.batches_of("k3")).matrix
    assert again.tobytes() == device_matrix("k3").tobytes()
