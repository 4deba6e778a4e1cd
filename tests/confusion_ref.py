"""A numpy restatement of the reference's detection `ConfusionMatrix` (utils/metrics.py:319-376) as the two-argmax rule the kernel
implements (csrc/det_metrics.hip), of the way both validators feed it, and the edge images of tests/golden/confusion.npz.

    each participating detection (confidence > conf) keeps its best gt among those with IoU > float32(iou_thres), whatever the classes
    (ties -> the higher gt index); each gt keeps the best of the detections that chose it (ties -> the higher detection index);
    matched gt -> matrix[cls(d), cls(i)], unmatched gt -> matrix[nc, cls(i)], and, only when the image has a match, every
    participating detection left unmatched -> matrix[cls(d), nc].
"""
import numpy as np

from test_det_metrics_host import iou_f32, scale_f32

CONF, IOU_THRES = 0.25, 0.45  # ConfusionMatrix(nc, conf=args.conf = 0.001) -> 0.25; iou_thres default


def match(iou, iou_thres=IOU_THRES):
    """iou (M, N) float32 of the participating detections -> gdet (M,): each gt's detection or -1"""
    M, N = iou.shape
    gdet = np.full(M, -1, np.int64)
    if M == 0 or N == 0:
        return gdet
    cand = iou > np.float32(iou_thres)
    v = np.where(cand, iou, np.float32(-1))
    best = M - 1 - np.argmax(v[::-1], axis=0)  # the last maximum: the higher gt index
    has = cand.any(0)
    for g in range(M):
        ds = [d for d in range(N) if has[d] and best[d] == g]
        if ds:
            top = max(iou[g, d] for d in ds)
            gdet[g] = max(d for d in ds if iou[g, d] == top)
    return gdet


def process_batch(matrix, det_box, det_conf, det_cls, gt_box, gt_cls, conf=CONF, iou_thres=IOU_THRES):
    """the drop-in: det_* None for `detections=None`; det_conf in the row's own precision (float32 or float64); adds into matrix"""
    nc = matrix.shape[0] - 1
    gt_cls = np.asarray(gt_cls).astype(np.int64)
    if det_box is not None:
        thr = np.float32(conf) if np.asarray(det_conf).dtype == np.float32 else np.float64(conf)
        part = np.asarray(det_conf) > thr
        det_box, det_cls = np.asarray(det_box, np.float32)[part], np.asarray(det_cls).astype(np.int64)[part]
    if len(gt_cls) == 0:
        if det_box is not None:
            for c in det_cls:
                matrix[c, nc] += 1
        return
    if det_box is None:
        for c in gt_cls:
            matrix[nc, c] += 1
        return
    gdet = match(iou_f32(np.asarray(gt_box, np.float32).reshape(-1, 4), det_box.reshape(-1, 4)), iou_thres)
    for g, d in enumerate(gdet):
        matrix[det_cls[d] if d >= 0 else nc, gt_cls[g]] += 1
    if (gdet >= 0).any():
        for d in range(len(det_cls)):
            if d not in gdet:
                matrix[det_cls[d], nc] += 1


def literal(matrix, det_box, det_conf, det_cls, gt_box, gt_cls, conf=CONF, iou_thres=IOU_THRES):
    """the reference's own statements with its unstable argsorts made stable (one image, gts and detections present)"""
    nc = matrix.shape[0] - 1
    part = np.asarray(det_conf) > conf
    det_box, det_cls = np.asarray(det_box, np.float32)[part], np.asarray(det_cls).astype(np.int64)[part]
    gt_cls = np.asarray(gt_cls).astype(np.int64)
    iou = iou_f32(np.asarray(gt_box, np.float32), det_box)
    x = np.nonzero(iou > np.float32(iou_thres))
    if x[0].shape[0]:
        matches = np.concatenate((np.stack(x, 1).astype(np.float32), iou[x[0], x[1]][:, None]), 1)
        if x[0].shape[0] > 1:
            matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
            matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
            matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
            matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
    else:
        matches = np.zeros((0, 3))
    n = matches.shape[0] > 0
    m0, m1, _ = matches.transpose().astype(int)
    for i, gc in enumerate(gt_cls):
        j = m0 == i
        if n and sum(j) == 1:
            matrix[det_cls[m1[j]], gc] += 1
        else:
            matrix[nc, gc] += 1
    if n:
        for i, dc in enumerate(det_cls):
            if not any(m1 == i):
                matrix[dc, nc] += 1


# ------------------------------------------------------------------------------------------------------------------------------
# the validators' calls on the batch dicts of tests/det_metrics_sets.py
# ------------------------------------------------------------------------------------------------------------------------------
def prep_3d(b, i, single_cls=False):
    """-> gt xyxy float32, gt classes, detection boxes float32 / confidences float64 / classes of the kept rows"""
    m = b["batch_idx"] == i
    q = b["bboxes"][m].astype(np.float32)
    dw, dh = q[:, 2] / np.float32(2), q[:, 3] / np.float32(2)
    g = np.stack((q[:, 0] - dw, q[:, 1] - dh, q[:, 0] + dw, q[:, 1] + dh), 1) * np.float32(b["ori_shape"][i][[1, 0, 1, 0]]).astype(np.float32)
    d = b["rows"][i][b["keep"][i]]
    return g, b["cls"][m].reshape(-1), d[:, 2:6].astype(np.float32), d[:, 13], (0 * d[:, 0] if single_cls else d[:, 0])


def prep_2d(b, i, single_cls=False):
    m = b["batch_idx"] == i
    q = b["bboxes"][m].astype(np.float32)
    H, W = (np.float32(v) for v in b["imgsz"])
    dw, dh = q[:, 2] / np.float32(2), q[:, 3] / np.float32(2)
    g = np.stack((q[:, 0] - dw, q[:, 1] - dh, q[:, 0] + dw, q[:, 1] + dh), 1) * np.array([W, H, W, H], np.float32)
    rp, (h0, w0) = b["ratio_pad"][i], b["ori_shape"][i]
    g = scale_f32(g, rp[0, 0], rp[1, 0], rp[1, 1], h0, w0)
    d = b["preds"][i]
    return (g, b["cls"][m].reshape(-1), scale_f32(d[:, :4], rp[0, 0], rp[1, 0], rp[1, 1], h0, w0), d[:, 4].astype(np.float32),
            (0 * d[:, 5] if single_cls else d[:, 5]))


def images(batches, single_cls=False):
    """every image of a set, prepared: (gt_box, gt_cls, det_box, det_conf, det_cls)"""
    for b in batches:
        n = len(b["rows"]) if "rows" in b else len(b["preds"])
        for i in range(n):
            yield (prep_3d if "rows" in b else prep_2d)(b, i, single_cls)


def update(matrix, image, conf=CONF, iou_thres=IOU_THRES):
    """what both validators' update_metrics do with one prepared image: nothing without gts, `detections=None` without rows"""
    g, gc, box, cf, dc = image
    if len(gc) == 0:
        return
    if len(dc) == 0:
        process_batch(matrix, None, None, None, g, gc, conf, iou_thres)
    else:
        process_batch(matrix, box, cf, dc, g, gc, conf, iou_thres)


def validator_matrix(batches, nc, single_cls=False, conf=CONF, iou_thres=IOU_THRES):
    matrix = np.zeros((nc + 1, nc + 1), np.int64)
    for im in images(batches, single_cls):
        update(matrix, im, conf, iou_thres)
    return matrix


# ------------------------------------------------------------------------------------------------------------------------------
# the edge images of the fixture ("x3": the 3D layout, classes 0..3), free of IoU ties above the threshold
# ------------------------------------------------------------------------------------------------------------------------------
X3_NC = 4


def make_x3():
    K = 6
    n_img = 8
    rows = np.zeros((n_img, K, 14))
    keep = np.zeros((n_img, K), bool)
    bidx, cls, boxes = [], [], []
    ori = np.array([[400, 1000]] * n_img, np.int64)

    def gt(i, c, x1, y1, x2, y2):
        bidx.append(i)
        cls.append(c)
        boxes.append([(x1 + x2) / 2 / 1000, (y1 + y2) / 2 / 400, (x2 - x1) / 1000, (y2 - y1) / 400])

    def det(i, k, c, box, score, kept=True):
        rows[i, k, 0], rows[i, k, 2:6], rows[i, k, 13], keep[i, k] = c, box, score, kept

    # image 0: no gts, two confident dets: the validators do not call process_batch
    det(0, 0, 0, [10, 10, 60, 60], 0.91)
    det(0, 3, 1, [100, 10, 160, 60], 0.42)
    # image 1: gts, rows present but none kept: `detections=None`
    gt(1, 0, 100, 100, 200, 200)
    gt(1, 3, 300, 100, 400, 200)
    det(1, 0, 0, [100, 100, 200, 200], 0.99, kept=False)
    det(1, 1, 3, [300, 100, 400, 200], 0.98, kept=False)
    # image 2: two dets choose gt A; the loser overlaps gt B above the threshold and is still predicted background, B is missed
    gt(2, 1, 100, 100, 200, 200)
    gt(2, 2, 130, 100, 230, 200)
    det(2, 0, 1, [102, 100, 202, 200], 0.61)
    det(2, 1, 2, [105, 100, 205, 200], 0.74)
    # image 3: kept rows at and below the confidence threshold are excluded (0.25 is not > 0.25); one wrong-class match
    gt(3, 0, 10, 10, 110, 90)
    gt(3, 3, 500, 200, 560, 260)
    det(3, 0, 0, [10, 10, 110, 90], 0.25)
    det(3, 1, 2, [12, 11, 108, 92], 0.66)
    det(3, 2, 3, [500, 200, 560, 260], 0.2)
    det(3, 4, 1, [700, 300, 760, 360], 0.8)
    # image 4: confident dets, gts, no pair above the threshold: the dets are NOT counted (`if n:`), the gts are missed
    gt(4, 0, 100, 100, 200, 200)
    gt(4, 1, 600, 100, 700, 200)
    det(4, 0, 0, [150, 150, 250, 250], 0.9)
    det(4, 2, 1, [800, 300, 900, 380], 0.7)
    # image 5: a det overlapping two gts picks the better one; a second det takes the other
    gt(5, 0, 300, 100, 400, 200)
    gt(5, 0, 320, 100, 420, 200)
    det(5, 0, 0, [316, 100, 416, 200], 0.5)
    det(5, 5, 3, [297, 100, 397, 200], 0.3)
    # image 6: a class-3 gt alone, a far det
    gt(6, 3, 50, 50, 90, 90)
    det(6, 1, 0, [500, 50, 590, 90], 0.95)
    # image 7: nothing at all
    return [dict(rows=rows, keep=keep, batch_idx=np.array(bidx, np.float32), cls=np.array(cls, np.float32),
                 bboxes=np.array(boxes, np.float32).reshape(-1, 4), ori_shape=ori)]


SETS = {"k3": ("k3", 3, False), "c2": ("c2", 80, False), "c2s": ("c2s", 80, True), "n3": ("n3", 3, False), "x3": ("x3", X3_NC, False)}


def batches_of(name):
    from det_metrics_sets import input_sets
    return make_x3() if name == "x3" else input_sets()[name]
