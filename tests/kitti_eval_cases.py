"""The synthetic case lists of tests/test_hip_kitti_eval_edges.py (NumPy only).  tests/test_kitti_eval_ref_host.py walks the same lists
with the restatement alone and asserts that they reach the edges they are named for, so a case cannot quietly stop testing its edge.

A case holds annos, an overlap table crafted by the test (both statistics entry points take the table as an input), the
(class code, difficulty) rows, the (rows, nk) min-overlaps, the metric and the AOS switch.  Crafted overlaps are multiples of 1/64 unless
a boundary is the point."""
import numpy as np

from kitti_eval_ref import MIN_OVERLAPS

F = np.float32
UP = lambda v: np.nextafter(F(v), F(np.inf))      # noqa: E731
DOWN = lambda v: np.nextafter(F(v), F(-np.inf))   # noqa: E731
ALL_CD = [(c, d) for c in range(3) for d in range(3)]


def anno(names, bbox=None, score=None, alpha=None, occ=None, trunc=None):
    n = len(names)
    a = {"name": np.array(list(names), dtype="<U16").reshape(n),
         "bbox": np.tile(F([0, 0, 50, 50]), (n, 1)) if bbox is None else np.asarray(bbox, F).reshape(n, 4),
         "alpha": np.zeros(n, F) if alpha is None else np.asarray(alpha, F).reshape(n),
         "occluded": np.zeros(n, F) if occ is None else np.asarray(occ, F).reshape(n),
         "truncated": np.zeros(n, F) if trunc is None else np.asarray(trunc, F).reshape(n),
         "location": np.ones((n, 3), F), "dimensions": np.ones((n, 3), F), "rotation_y": np.zeros(n, F)}
    if score is not None:
        a["score"] = np.asarray(score, F).reshape(n)
    return a


class Case:
    def __init__(self, name, gts, dts, ovs, cd, mo, metric, aos=False):
        self.name, self.gts, self.dts, self.cd, self.metric, self.aos = name, gts, dts, list(cd), metric, aos
        self.mo = np.asarray(mo, np.float64).reshape(len(self.cd), -1)
        self.nk = self.mo.shape[1]
        for o, g, d in zip(ovs, gts, dts):
            assert o.shape == (len(d["name"]), len(g["name"])), name
        self.ov = np.concatenate([np.asarray(o, F).reshape(-1) for o in ovs] + [np.zeros(0, F)])

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------------------
# crowded image: the assigned-detection bitmask past its first word, the strided flag loads past 64 and past the block
# ---------------------------------------------------------------------------------------------------------------------------------
CROWDED_SHAPES = [(31, 5), (32, 5), (33, 34), (64, 65), (65, 64), (255, 3), (256, 256)]


def crowded(nd, ng, nk):
    """One image of Cars.  gts 2m and 2m + 1 both overlap det nd - 1 - m above every min-overlap (the even one takes it, the odd one is
    denied); odd gts of odd m fall back on det m.  Low overlaps are sprinkled so the lanes of the lower min-overlaps walk other matches;
    scores come from 13 values, so they tie."""
    rng = np.random.default_rng(1000 * nd + ng)
    ov = np.where(rng.random((nd, ng)) < 0.06, rng.integers(1, 41, (nd, ng)), 0).astype(np.float64)
    for m in range((ng + 1) // 2):
        q = nd - 1 - m
        if q < 0:
            break
        ov[q, 2 * m] = 60
        if 2 * m + 1 < ng:
            ov[q, 2 * m + 1] = 58
            if m % 2 == 1 and m < nd:
                ov[m, 2 * m + 1] = max(ov[m, 2 * m + 1], 50)
    gn = ["Van" if i % 11 == 10 else "Car" for i in range(ng)]
    dn = ["Pedestrian" if j % 17 == 5 else "Car" for j in range(nd)]
    score = [((j * 7) % 13 + 1) / 16 for j in range(nd)]
    alpha = rng.integers(-3, 4, nd) / 2
    mo = [[0.7, 0.5, 0.3][:nk]]
    return Case(f"crowded-{nd}x{ng}-nk{nk}", [anno(gn, alpha=rng.integers(-3, 4, ng) / 2)], [anno(dn, score=score, alpha=alpha)],
                [ov / 64], [(0, 0)], mo, 2, aos=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# random mixed images (lanes, image counts)
# ---------------------------------------------------------------------------------------------------------------------------------
GT_NAMES = ["Car"] * 5 + ["Pedestrian"] * 3 + ["Cyclist"] * 3 + ["Van", "Person_sitting", "Truck", "DontCare", "DontCare"]
DT_NAMES = ["Car"] * 4 + ["Pedestrian"] * 3 + ["Cyclist"] * 3 + ["Van"]


def random_image(rng, ng, nd):
    """boxes on an 8-pixel grid with heights around both minimum heights; overlaps are multiples of 1/64, mostly zero"""
    def boxes(n, lo):
        x1, y1 = rng.integers(0, 120, n) * 8.0, rng.integers(10, 30, n) * 8.0
        h = rng.choice([24.0, 25.0, 32.0, 40.0, 48.0, 56.0, 64.0, 96.0, 120.0], n)
        return np.stack([x1, y1, x1 + rng.integers(lo, 12, n) * 8.0, y1 + h], 1)
    gt = anno(rng.choice(GT_NAMES, ng), bbox=boxes(ng, 2), alpha=rng.integers(-6, 7, ng) / 4, occ=rng.choice([0, 0, 0, 1, 2, 3], ng),
              trunc=rng.choice([0.0, 0.0, 0.125, 0.25, 0.375, 0.625], ng))
    dt = anno(rng.choice(DT_NAMES, nd), bbox=boxes(nd, 1), alpha=rng.integers(-6, 7, nd) / 4, score=rng.integers(1, 33, nd) / 32)
    ov = np.where(rng.random((nd, ng)) < 0.3, rng.integers(1, 65, (nd, ng)), 0) / 64
    for i in range(min(ng, nd)):   # most gts have a detection of their own class on them
        if rng.random() < 0.7 and gt["name"][i] in ("Car", "Pedestrian", "Cyclist"):
            dt["name"][i] = gt["name"][i]
            ov[i, i] = rng.integers(40, 65) / 64
    return gt, dt, ov


LANE_ROWS = np.array([[0.7, 0.5, 0.45], [0.5, 0.25, 0.3], [0.3, 0.125, 0.15], [0.625, 0.375, 0.35], [0.4, 0.2, 0.25], [0.8, 0.6, 0.75]])


def lanes(nk, official=False):
    """9 (class, difficulty) rows in one launch over 10 mixed images; min-overlaps differ per k and per class"""
    rng = np.random.default_rng(77)
    imgs = [random_image(rng, int(rng.integers(6, 14)), int(rng.integers(8, 22))) for _ in range(10)]
    rows = MIN_OVERLAPS[:, 0, :3] if official else LANE_ROWS[:nk]   # (k, class)
    mo = [[rows[k][c] for k in range(nk)] for c, _ in ALL_CD]
    return Case(f"lanes-nk{nk}" + ("-official" if official else ""), [g for g, _, _ in imgs], [d for _, d, _ in imgs],
                [o for _, _, o in imgs], ALL_CD, mo, 0, aos=True)


LANE_CASES = [(1, False), (2, False), (3, False), (6, False), (3, True)]
IMAGE_COUNTS = [1, 255, 256, 257, 600]


def images(n_img):
    """a few boxes per image; images without gts, without dets and without either are interleaved"""
    rng = np.random.default_rng(5)
    gts, dts, ovs = [], [], []
    for i in range(n_img):
        ng, nd = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        if n_img > 1:
            ng, nd = (0 if i % 7 in (1, 3) else ng), (0 if i % 7 in (2, 3) else nd)
        g, d, o = random_image(rng, ng, nd)
        if i == 256:   # the first image past one stride of the reduce has a tp, a fn and two fps of its own
            g = anno(["Car", "Car", "Pedestrian"], alpha=[0.5, 1, -1])
            d = anno(["Car", "Car", "Pedestrian", "Car"], score=[0.5, 0.75, 0.5, 0.25], alpha=[1, 0, 1, 2])
            o = np.array([[0.75, 0, 0], [0, 0, 0], [0, 0, 0.75], [0, 0, 0]])
        gts.append(g), dts.append(d), ovs.append(o)
    return Case(f"images-{n_img}", gts, dts, ovs, [(0, 1), (1, 2)], [[0.7, 0.5], [0.5, 0.25]], 0, aos=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# ties and boundaries
# ---------------------------------------------------------------------------------------------------------------------------------
BOUNDARY_MO = [0.5, 0.25, 0.7, 0.3]
BOUNDARY_OV = [F(0.5), F(0.25), F(0.7), UP(0.7), DOWN(0.7), F(0.3), UP(0.3), DOWN(0.3), F(33 / 64), F(31 / 64), F(17 / 64), F(15 / 64)]


def ties():
    """image 0: dets 0 and 1 tie in score and in overlap with gt 0, gt 1 overlaps det 1 alone; so whichever pass resolves a tie to the
    later det leaves gt 1 without one.  image 1: det 0 is too low (ignored_dt = 1) and precedes same-class dets with an equal and a better
    overlap (gt 0), stands alone (gt 1), and follows a same-class det (gt 2).  image 2: gt g meets det g alone at BOUNDARY_OV[g].
    image 3: three dets of equal score on three gts, so the recall thresholds equal scores."""
    o0 = np.array([[48, 0], [48, 48], [0, 0]]) / 64
    g0, d0 = anno(["Car", "Car"]), anno(["Car"] * 3, score=[0.5, 0.5, 0.25])
    low = [0, 0, 50, 20]
    o1 = np.array([[50, 0, 0], [50, 0, 0], [52, 0, 0], [0, 50, 0], [0, 0, 50], [0, 0, 56]]) / 64
    g1 = anno(["Car"] * 3)
    d1 = anno(["Car"] * 6, bbox=[low, [0, 0, 50, 50], [0, 0, 50, 50], low, [0, 0, 50, 50], low], score=[0.75, 0.75, 0.625, 0.5, 0.5, 0.25])
    n = len(BOUNDARY_OV)
    o2 = np.diag(np.asarray(BOUNDARY_OV, F))
    g2, d2 = anno(["Car"] * n), anno(["Car"] * n, score=[(i % 5 + 2) / 8 for i in range(n)])
    o3 = np.eye(3) * (60 / 64)
    g3, d3 = anno(["Car"] * 3), anno(["Car"] * 3, score=[0.375] * 3)
    return Case("ties", [g0, g1, g2, g3], [d0, d1, d2, d3], [o0, o1, o2, o3], [(0, 0), (0, 1)], [BOUNDARY_MO] * 2, 1, aos=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# clean_data's edges
# ---------------------------------------------------------------------------------------------------------------------------------
TRUNC_EDGES = [F(0.15), UP(0.15), DOWN(0.15), F(0.3), UP(0.3), DOWN(0.3), F(0.5), UP(0.5), DOWN(0.5)]
HEIGHT_EDGES = [F(40), UP(40), DOWN(40), F(25), UP(25), DOWN(25)]
FLAG_NAMES = ["Car", "Van", "Pedestrian", "Person_sitting", "Cyclist", "car", "Truck", "DontCare"]


def flag_images():
    """One gt per edge value and class, each under a detection of its own (overlap 0.75); one detection per height edge and class on a gt
    of its own.  Heights are differences of fp32 corners: y1 = 0, so y2 is the height bit for bit."""
    gts, dts, ovs = [], [], []
    for cls in ("Car", "Pedestrian", "Cyclist"):
        # gt edges: (height, occlusion, truncation), one varied at a time
        var = [(h, 0, 0) for h in HEIGHT_EDGES] + [(50, o, 0) for o in (0, 1, 2, 3)] + [(50, 0, t) for t in TRUNC_EDGES]
        names = [cls] * len(var) + FLAG_NAMES
        var = var + [(50, 0, 0)] * len(FLAG_NAMES)
        n = len(var)
        g = anno(names, bbox=[[0, 0, 30, v[0]] for v in var], occ=[v[1] for v in var], trunc=[v[2] for v in var],
                 alpha=[(i % 7 - 3) / 2 for i in range(n)])
        d = anno([cls] * n, score=[(i % 9 + 1) / 16 for i in range(n)], alpha=[(i % 5 - 2) / 2 for i in range(n)])
        gts.append(g), dts.append(d), ovs.append(np.eye(n) * 0.75)
        # det edges: heights, their negatives (y2 < y1) and a neighbour class, each on a plain gt
        hs = [float(h) for h in HEIGHT_EDGES] + [-float(h) for h in HEIGHT_EDGES] + [-10.0, 50.0, 50.0]
        dn = [cls] * (len(hs) - 1) + ["Van" if cls == "Car" else "Person_sitting"]
        m = len(hs)
        gts.append(anno([cls] * m))
        dts.append(anno(dn, bbox=[[0, 0, 30, h] for h in hs], score=[(i % 6 + 2) / 16 for i in range(m)]))
        ovs.append(np.eye(m) * 0.75)
    return gts, dts, ovs


def flag_cases():
    gts, dts, ovs = flag_images()
    mo = [[0.7 if c == 0 else 0.5] for c, _ in ALL_CD]
    return [Case(f"flags-metric{m}", gts, dts, ovs, ALL_CD, mo, m, aos=True) for m in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# DontCare suppression
# ---------------------------------------------------------------------------------------------------------------------------------
P07 = int(round(float(F(0.7)) * 2 ** 24))   # float32(0.7) = P07 * 2^-24
DC_MO = [0.7, 0.5, 0.25]


def dontcare_images():
    """Unmatched Car detections against DontCare boxes; the ratio inter / area(det) is exact because every area is a power of two.
    image 0: a 64 x 64 det per row y0 = 1000 r, its DontCare box covering `cover` / 64 of its width: ratios 0, 1/4, 1/2, 1 and one
    column to either side of 1/4 and 1/2; the last rows lie partly in two DontCare boxes (3/8 + 3/8: the larger counts, not the sum).
    image 1: 2^24 x 64 dets, DontCare boxes P07 - 1, P07, P07 + 1 wide: the ratio is float32(0.7) and its neighbours.
    Every image has one matched gt whose det has the lowest score, so each threshold keeps all the unmatched dets."""
    cover = [0, 15, 16, 17, 31, 32, 33, 63, 64]
    db, cb = [[0, 0, 50, 50]], []
    for r, c in enumerate(cover):
        y0 = 1000.0 * (r + 1)
        db.append([0, y0, 64, y0 + 64])
        if c:
            cb.append([-8, y0 - 8, c, y0 + 80])
    for r, (a, b) in enumerate([(24, 24), (24, 40), (40, 16)]):   # two boxes from the left and from the right
        y0 = 1000.0 * (len(cover) + r + 1)
        db.append([0, y0, 64, y0 + 64])
        cb += [[-8, y0, a, y0 + 64], [64 - b, y0 - 1, 80, y0 + 65]]
    db.append([200, 0, 264, 64])   # outside every DontCare box
    g0 = anno(["Car"] + ["DontCare"] * len(cb), bbox=[[0, 0, 50, 50]] + cb)
    d0 = anno(["Car"] * len(db), bbox=db, score=[0.125] + [0.5 + 0.015625 * i for i in range(len(db) - 1)])
    o0 = np.zeros((len(db), 1 + len(cb)))
    o0[0, 0] = 0.75
    db1, cb1 = [[0, 0, 50, 50]], []
    for r, w in enumerate([P07 - 1, P07, P07 + 1]):
        y0 = 1000.0 * (r + 1)
        db1.append([0, y0, 2 ** 24, y0 + 64])
        cb1.append([0, y0, w, y0 + 64])
    g1 = anno(["Car"] + ["DontCare"] * 3, bbox=[[0, 0, 50, 50]] + cb1)
    d1 = anno(["Car"] * 4, bbox=db1, score=[0.25, 0.5, 0.625, 0.75])
    o1 = np.zeros((4, 4))
    o1[0, 0] = 0.75
    g2, d2 = anno(["Car", "Pedestrian"]), anno(["Car", "Car"], score=[0.375, 0.5])   # no DontCare box at all
    return [g0, g1, g2], [d0, d1, d2], [o0, o1, np.array([[0.75, 0], [0, 0]])]


def dontcare_cases():
    gts, dts, ovs = dontcare_images()
    return [Case(f"dontcare-metric{m}", gts, dts, ovs, [(0, 0), (0, 2)], [DC_MO] * 2, m, aos=True) for m in (0, 1, 2)]


def full_recall():
    """41 Cars, each under a detection of its own: lane 0 finds all of them (41 thresholds), lane 1 not one (none)"""
    n = 41
    return Case("full-recall", [anno(["Car"] * n)], [anno(["Car"] * n, score=[(i * 5 % n + 1) / 64 for i in range(n)])], [np.eye(n) * 0.75],
                [(0, 0)], [[0.7, 0.8]], 2, aos=True)


def all_cases():
    out = [crowded(nd, ng, 1) for nd, ng in CROWDED_SHAPES] + [crowded(nd, ng, 3) for nd, ng in CROWDED_SHAPES]
    out += [lanes(nk, off) for nk, off in LANE_CASES] + [images(n) for n in IMAGE_COUNTS] + [ties(), full_recall()] + flag_cases() + dontcare_cases()
    return out
