"""A plain sequential restatement of the KITTI AP matching (csrc/kitti_eval.hip, kitti_eval.py), written from include/y3d.h, DESIGN
§3.10 and the kernel's comments: name codes, clean_data's ignore flags, both passes of the per-image statistics, the recall threshold
scan, precision with its suffix max and mAP.  NumPy and python loops only (no torch), so both the host pin
(tests/test_kitti_eval_ref_host.py) and the device tests (tests/test_hip_kitti_eval*.py) can use it.

Rounding, as the kernel states it: box heights are fp32 differences; an overlap is an fp32 value compared with the min-overlap in
double; truncation is an fp32 value compared with 0.15 / 0.3 / 0.5 in double; a detection's DontCare overlap is
float32(iw * ih / ua) with iw, ih in double and ua the fp32 area of the detection; the alpha difference is fp32 and its cosine double.
fp32 values are held as python floats (exact), so `<` and `>` between two of them decide as the fp32 comparison does.

The fp64 geometry at the end (rectangle corners, Sutherland-Hodgman clipping, shoelace area) is the independent reference of the
rotated overlaps."""
import math
from bisect import bisect_left

import numpy as np

N_SAMPLE_PTS = 41
NAMES = ("car", "pedestrian", "cyclist", "van", "person_sitting", "tractor", "trailer")   # codes 0..6; 7 = any other name
MIN_HEIGHT = (40.0, 25.0, 25.0)
MAX_OCCLUSION = (0.0, 1.0, 2.0)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
NO_DETECTION = -10000000.0
NEG_INF = float("-inf")

# get_official_eval_result's min-overlap tables: [k][metric (bbox, bev, 3d)][class id 0..7]
MIN_OVERLAPS = np.array([[[0.7, 0.5, 0.5, 0.7, 0.5, 0.7, 0.7, 0.7]] * 3,
                         [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5],
                          [0.5, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5]],
                         [[0.7, 0.5, 0.5, 0.7, 0.5, 0.5, 0.5, 0.5], [0.3, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5],
                          [0.3, 0.25, 0.25, 0.5, 0.25, 0.5, 0.5, 0.5]]])
CLASS_IDS = {"Car": 0, "Pedestrian": 1, "Cyclist": 2}


def name_codes(names):
    """y3d.h's name codes: 0 car .. 6 trailer, 7 other (case-insensitive), + 8 for a name that is exactly "DontCare" """
    out = []
    for n in names:
        n = str(n)
        low = n.lower()
        out.append((NAMES.index(low) if low in NAMES else 7) + (8 if n == "DontCare" else 0))
    return np.array(out, dtype=np.int32)


def _f32(a, k, width=None, default=None):
    n = len(a["name"])
    v = np.asarray(a[k], dtype=np.float32) if k in a else np.full(n, default, np.float32)
    return v.reshape(n, width) if width else v.reshape(n)


def flags(gt, dt, cls, diff):
    """clean_data for class code `cls` and difficulty `diff`: (ignored_gt, ignored_dt) as int lists and the DontCare boxes (n, 4) fp32.
    ignored_gt: 0 counted, 1 matched but not counted (neighbour class, or too occluded / truncated / small), -1 another class.
    ignored_dt: 1 lower than the minimum height, else 0 for the class and -1 for any other."""
    gcode = name_codes(gt["name"])
    gb = _f32(gt, "bbox", 4)
    gh = (gb[:, 3] - gb[:, 1]).tolist()                       # fp32 difference
    occ = _f32(gt, "occluded", default=0.0).tolist()
    trunc = _f32(gt, "truncated", default=0.0).tolist()       # fp32 value as a double
    ignored_gt = []
    for i in range(len(gcode)):
        c = int(gcode[i]) & 7
        if c == cls:
            valid = 1
        elif (cls == 1 and c == 4) or (cls == 0 and c == 3):   # Person_sitting next to Pedestrian, Van next to Car
            valid = 0
        else:
            valid = -1
        ignore = occ[i] > MAX_OCCLUSION[diff] or trunc[i] > MAX_TRUNCATION[diff] or gh[i] <= MIN_HEIGHT[diff]
        if valid == 1 and not ignore:
            ignored_gt.append(0)
        elif valid == 0 or (ignore and valid == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
    dcode = name_codes(dt["name"])
    db = _f32(dt, "bbox", 4)
    dh = np.abs(db[:, 3] - db[:, 1]).tolist()
    ignored_dt = []
    for j in range(len(dcode)):
        if dh[j] < MIN_HEIGHT[diff]:
            ignored_dt.append(1)
        elif (int(dcode[j]) & 7) == cls:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return ignored_gt, ignored_dt, gb[(gcode & 8) != 0]


def dontcare_overlaps(dt_bbox, dc_boxes):
    """per detection, the list of its overlaps with the DontCare boxes, intersection over the detection's own area"""
    db = np.asarray(dt_bbox, np.float32).reshape(-1, 4)
    ua = ((db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])).astype(np.float64)   # fp32 product, then widened
    d, c = db.astype(np.float64), np.asarray(dc_boxes, np.float32).reshape(-1, 4).astype(np.float64)
    out = []
    for j in range(d.shape[0]):
        row = []
        for i in range(c.shape[0]):
            o = 0.0
            iw = min(d[j, 2], c[i, 2]) - max(d[j, 0], c[i, 0])
            if iw > 0:
                ih = min(d[j, 3], c[i, 3]) - max(d[j, 1], c[i, 1])
                if ih > 0:
                    o = float(np.float32(iw * ih / ua[j]))
            row.append(o)
        out.append(row)
    return out


def _note(trace, key, what):
    trace.setdefault(key, []).append(what)


def image_stats(ov, ignored_gt, ignored_dt, scores, min_overlap, metric=0, thresh=0.0, count=False, aos=False, gt_alpha=None,
                dt_alpha=None, dc=None, trace=None):
    """compute_statistics_jit on one image.  ov[j][i]: overlap of det j with gt i.  count = False (threshold pass): the score of the det
    each gt is a true positive of, -inf for the others.  count = True: (tp, fp, fn, similarity) at score threshold `thresh`; dc[j] lists
    det j's DontCare overlaps (metric 0 only).  `trace`, a dict, collects what the walk met: lists keyed 'assigned' (gt, det),
    'denied' (gt, det: above the min-overlap but taken), 'score_tie', 'ov_tie', 'aid_taken', 'aid_replaced', 'at_min' (an overlap equal
    to float32(min_overlap), gt, det), 'suppressed' / 'kept' (det), 'at_thresh' (det)."""
    ng, nd = len(ignored_gt), len(ignored_dt)
    mo = float(min_overlap)
    mo32 = float(np.float32(mo))
    assigned = [False] * nd
    tp = fp = fn = 0
    sim = 0.0
    tp_score = [NEG_INF] * ng
    for i in range(ng):
        ig = ignored_gt[i]
        if ig == -1:
            continue
        det, valid, aid, vscore, maxov = -1, False, False, NO_DETECTION, 0.0
        for j in range(nd):
            idj = ignored_dt[j]
            if idj == -1:
                continue
            if assigned[j]:
                if trace is not None and ov[j][i] > mo:
                    _note(trace, "denied", (i, j))
                continue
            sc = scores[j]
            if count and sc < thresh:
                continue
            o = ov[j][i]
            above = o > mo
            if trace is not None:
                if o == mo32:
                    _note(trace, "at_min", (i, j, above))
                if count and sc == thresh:
                    _note(trace, "at_thresh", j)
                if above and valid and not count and sc == vscore:
                    _note(trace, "score_tie", (i, det, j))
                if above and valid and count and idj == 0 and not aid and o == maxov:
                    _note(trace, "ov_tie", (i, det, j))
            if not count:
                if above and sc > vscore:
                    det, vscore, valid = j, sc, True
            elif above and (o > maxov or aid) and idj == 0:
                if trace is not None and aid:
                    _note(trace, "aid_replaced", (i, det, j))
                maxov, det, valid, aid = o, j, True, False
            elif above and not valid and idj == 1:
                det, valid, aid = j, True, True
                if trace is not None:
                    _note(trace, "aid_taken", (i, j))
        if not valid:
            if ig == 0:
                fn += 1
            continue
        if not (ig == 1 or ignored_dt[det] == 1):
            tp += 1
            tp_score[i] = scores[det]
            if count and aos:
                delta = float(np.float32(gt_alpha[i]) - np.float32(dt_alpha[det]))
                sim += (1.0 + math.cos(delta)) / 2.0
        assigned[det] = True
        if trace is not None:
            _note(trace, "assigned", (i, det))
    if not count:
        return tp_score
    for j in range(nd):
        if ignored_dt[j] != 0 or assigned[j] or scores[j] < thresh:
            continue
        if metric == 0 and dc is not None and any(o > mo for o in dc[j]):   # inside a DontCare box: counted, then taken off
            if trace is not None:
                _note(trace, "suppressed", j)
            continue
        if trace is not None and dc is not None and len(dc[j]):
            _note(trace, "kept", j)
        fp += 1
    if not aos:
        return tp, fp, fn, 0.0
    return tp, fp, fn, (sim if (tp > 0 or fp > 0) else -1.0)


def thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """get_thresholds: the scores (descending) at which recall first reaches each of the 41 sample points"""
    scores = sorted((float(s) for s in scores), reverse=True)
    cur, out = 0, []
    for i, s in enumerate(scores):
        lr = (i + 1) / num_gt
        rr = (i + 2) / num_gt if i < len(scores) - 1 else lr
        if (rr - cur) < (cur - lr) and i < len(scores) - 1:
            continue
        out.append(s)
        cur += 1 / (num_sample_pts - 1.0)
    return out


class Scene:
    """gt / dt annos of all images with their fields cast to fp32 once, as the packed records hold them"""

    def __init__(self, gts, dts):
        assert len(gts) == len(dts)
        self.gts, self.dts = gts, dts
        self.n_img = len(gts)
        self.ng = [len(a["name"]) for a in gts]
        self.nd = [len(a["name"]) for a in dts]
        self.gt_off = np.concatenate(([0], np.cumsum(self.ng))).astype(np.int64)
        self.ov_off = np.concatenate(([0], np.cumsum(np.asarray(self.ng, np.int64) * np.asarray(self.nd, np.int64))))
        self.total_gt = int(self.gt_off[-1])
        self.scores = [_f32(a, "score").tolist() for a in dts]
        self.gt_alpha = [_f32(a, "alpha", default=-10.0).tolist() for a in gts]
        self.dt_alpha = [_f32(a, "alpha", default=-10.0).tolist() for a in dts]
        self._flags, self._dc = {}, {}

    def flags(self, cls, diff):
        if (cls, diff) not in self._flags:
            self._flags[cls, diff] = [flags(g, d, cls, diff) for g, d in zip(self.gts, self.dts)]
        return self._flags[cls, diff]

    def dontcare(self, img):
        if img not in self._dc:
            self._dc[img] = dontcare_overlaps(self.dts[img]["bbox"], self.flags(0, 0)[img][2])
        return self._dc[img]

    def split(self, flat):
        """flat fp32 overlaps (image i's (n_dt, n_gt) block at ov_off[i]) -> per-image nested lists ov[j][i]"""
        flat = np.asarray(flat, np.float32)
        assert flat.shape[0] >= self.ov_off[-1]
        return [flat[self.ov_off[i]:self.ov_off[i + 1]].reshape(self.nd[i], self.ng[i]).tolist() for i in range(self.n_img)]


def eval_setting(scene, ov, cls, diff, metric, min_overlap, aos=False, trace=None):
    """One (class code, difficulty, metric, min-overlap) setting over all images.  ov: scene.split(...) of the metric's overlaps.
    -> dict: tp_score (total_gt) fp32, nvalid (n_img), thresholds (n <= 41) fp32, cnt (41, n_img, 3) and sim (41, n_img) with zero rows
    from n on, pr (41, 4), precision and orientation (41) after the suffix max.  trace: see image_stats (one dict per image is kept
    under trace[img])."""
    n_img = scene.n_img
    fl = scene.flags(cls, diff)
    tp_score = np.full(max(scene.total_gt, 1), NEG_INF, np.float32)
    nvalid = np.zeros(n_img, np.int64)
    sub = []   # per image: the gts / dets the class looks at (flags != -1), which is all the walk ever touches
    for img in range(n_img):
        igt, idt, _ = fl[img]
        rg = [i for i, f in enumerate(igt) if f != -1 or trace is not None]   # a trace keeps the image's own indices
        rd = [j for j, f in enumerate(idt) if f != -1 or trace is not None]
        o = ov[img]
        s = {"rg": rg, "rd": rd, "igt": [igt[i] for i in rg], "idt": [idt[j] for j in rd], "ov": [[o[j][i] for i in rg] for j in rd],
             "sc": [scene.scores[img][j] for j in rd], "ga": [scene.gt_alpha[img][i] for i in rg],
             "da": [scene.dt_alpha[img][j] for j in rd], "dc": None}
        if metric == 0:
            dc = scene.dontcare(img)
            s["dc"] = [dc[j] for j in rd]
        sub.append(s)
        nvalid[img] = sum(1 for f in igt if f == 0)
        tr = None if trace is None else trace.setdefault(img, {}).setdefault("thresholds", {})
        got = image_stats(s["ov"], s["igt"], s["idt"], s["sc"], min_overlap, metric, trace=tr)
        for a, i in enumerate(rg):
            tp_score[scene.gt_off[img] + i] = got[a]
    thr = np.array(thresholds(tp_score[tp_score > NEG_INF].tolist(), int(nvalid.sum())), dtype=np.float32)
    n = thr.shape[0]
    assert n <= N_SAMPLE_PTS
    cnt = np.zeros((N_SAMPLE_PTS, n_img, 3), np.int64)
    sim = np.zeros((N_SAMPLE_PTS, n_img), np.float64)
    pr = np.zeros((N_SAMPLE_PTS, 4), np.float64)
    tl = thr.tolist()
    for img in range(n_img):
        s = sub[img]
        memo = {}   # the walk depends on the threshold only through which dets fall below it
        order = sorted(s["sc"])
        for t in range(n):
            key = bisect_left(order, tl[t])   # how many scores are below the threshold
            if key not in memo or trace is not None:
                tr = None if trace is None else trace.setdefault(img, {}).setdefault(t, {})
                memo[key] = image_stats(s["ov"], s["igt"], s["idt"], s["sc"], min_overlap, metric, tl[t], True, aos, s["ga"], s["da"],
                                        s["dc"], tr)
            cnt[t, img] = memo[key][:3]
            sim[t, img] = memo[key][3]
    for t in range(n):
        pr[t, :3] = cnt[t].sum(0)
        acc = 0.0
        for img in range(n_img):
            if sim[t, img] != -1.0:
                acc += sim[t, img]
        pr[t, 3] = acc
    precision, orientation = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision[:n] = pr[:n, 0] / (pr[:n, 0] + pr[:n, 1])   # 0 / 0 = NaN
        if aos:
            orientation[:n] = pr[:n, 3] / (pr[:n, 0] + pr[:n, 1])
    for i in range(n):
        precision[i] = np.max(precision[i:])
        if aos:
            orientation[i] = np.max(orientation[i:])
    return {"tp_score": tp_score, "nvalid": nvalid, "thresholds": thr, "cnt": cnt, "sim": sim, "pr": pr, "precision": precision,
            "orientation": orientation}


def mAP(prec, mode=40):
    prec = np.asarray(prec, np.float64)
    if mode == 40:
        return prec[..., 1:].sum(-1) / 40 * 100
    assert mode == 11
    return prec[..., ::4].sum(-1) / 11 * 100


def wants_aos(dts):
    """get_official_eval_result's rule: the first image with detections decides, by its first alpha"""
    for a in dts:
        al = np.asarray(a["alpha"]) if "alpha" in a else np.zeros(0)
        if al.shape[0] != 0:
            return bool(al[0] != -10)
    return False


def official_detail(scene, ovs, cls_name, mode=40, difficulties=(0, 1, 2)):
    """the detail dict of get_official_eval_result for one class; ovs[metric] = scene.split(overlaps of the metric).  Later
    min-overlap rows overwrite equal keys, as the dict they are written into does."""
    c = CLASS_IDS[cls_name]
    aos = wants_aos(scene.dts)
    detail, done = {}, {}
    for k in range(MIN_OVERLAPS.shape[0]):
        for metric, tag in enumerate(("bbox", "bev", "3d")):
            mo = MIN_OVERLAPS[k, metric, c]
            if (metric, mo) not in done:   # the table repeats min-overlaps across k; a setting is evaluated once
                done[metric, mo] = [eval_setting(scene, ovs[metric], c, d, metric, mo, aos and metric == 0) for d in difficulties]
            res = done[metric, mo]
            detail[f"{tag}@{mo:.2f}"] = [float(mAP(r["precision"], mode)) for r in res]
            if aos and metric == 0:
                detail["aos"] = [float(mAP(r["orientation"], mode)) for r in res]
    return detail


# ---------------------------------------------------------------------------------------------------------------------------------
# independent fp64 geometry: rectangle corners, Sutherland-Hodgman clipping, shoelace area
# ---------------------------------------------------------------------------------------------------------------------------------
def corners(x, z, l, w, ry):
    c, s = math.cos(ry), math.sin(ry)
    local = [(-l / 2, -w / 2), (-l / 2, w / 2), (l / 2, w / 2), (l / 2, -w / 2)]
    return [(c * u + s * v + x, -s * u + c * v + z) for u, v in local]


def shoelace(p):
    return 0.5 * sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p)))


def clip(subject, clipper):
    if shoelace(clipper) < 0:
        clipper = clipper[::-1]
    out = subject
    for i in range(len(clipper)):
        a, b = clipper[i], clipper[(i + 1) % len(clipper)]
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        inp, out = out, []
        for j in range(len(inp)):
            p, q = inp[j], inp[(j + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return []
    return out


def inter_fp64(a, b):
    p = clip(corners(*a), corners(*b))
    return abs(shoelace(p)) if len(p) >= 3 else 0.0


def bev_iou(a, b):
    i = inter_fp64(a, b)
    return i / (a[2] * a[3] + b[2] * b[3] - i)


def iou3d(g, d):
    """g, d = (x, y, z, l, h, w, ry), y the bottom face (camera frame)"""
    i = inter_fp64((g[0], g[2], g[3], g[5], g[6]), (d[0], d[2], d[3], d[5], d[6]))
    iy = min(g[1], d[1]) - max(g[1] - g[4], d[1] - d[4])
    if iy <= 0 or i <= 0:
        return 0.0
    v = i * iy
    return v / (g[3] * g[4] * g[5] + d[3] * d[4] * d[5] - v)
