"""GPU: the kernels of csrc/kitti_eval.hip at their edges, against the sequential restatement of tests/kitti_eval_ref.py.

The statistics entry points take the overlap table as an input, so the cases of tests/kitti_eval_cases.py hand them crafted tables (exact
ties, exact boundary values) and every per-image output is compared: `cnt`, `nvalid` and `pr[..., 0:3]` as integers at every
(setting, threshold, image), `tp_score` bit for bit (-inf wherever the gt is no true positive), the recall thresholds, and `sim` /
`pr[..., 3]` within a derived bound.  Outputs start as sentinels (cnt 0x7f7f7f7f, sim / pr NaN, tp_score -inf, nvalid -1) between guard
bands; every element must be written and every guard left alone.  tests/test_kitti_eval_ref_host.py shows that the cases reach the
edges they are named for.

Bound on sim and pr[..., 3]: the terms (1 + cos(delta)) / 2 are doubles in [0, 1].  Device and restatement form delta by the same
fp32 subtraction and add an image's terms in the same gt order, so an image's sum differs only through the two cosine routines, each
within an ulp of a value <= 1: under 2^-51 per term once halved and compared, 2^-50 allowed.  The image sums then meet in a fixed tree
on the device and in image order here; an image contributes one rounding on either side, allowed 2^-50 each time (the sums of these
cases stay small: tens of terms per setting where there are hundreds of images).  Hence |difference| <= (n_terms + n_img) * 2^-50,
with n_terms the true positives of the image (sim) or of all images (pr) and n_img = 1 for sim.  The worst figures are printed."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import kitti_eval_cases as C
import kitti_eval_ref as R

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import kitti_eval as KE  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402

GUARD = 64
NT = R.N_SAMPLE_PTS
CNT_FILL = 0x7F7F7F7F
EPS = 2.0 ** -50


class Guarded:
    """n elements of `fill` between two guard bands of the same fill"""

    def __init__(self, n, dtype, fill):
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        self.n = n
        self.before = self.buf.cpu().numpy().copy()
        self.ptr = self.buf[GUARD:].data_ptr()

    def get(self):
        """the payload, after checking that both guard bands still hold their bytes"""
        now = self.buf.cpu().numpy()
        raw = lambda a: a.view(np.uint8)
        assert np.array_equal(raw(now[:GUARD]), raw(self.before[:GUARD])), "guard before the buffer was written"
        assert np.array_equal(raw(now[GUARD + self.n:]), raw(self.before[GUARD + self.n:])), "guard after the buffer was written"
        return now[GUARD:GUARD + self.n]

    def untouched(self):
        now = self.buf.cpu().numpy()
        return np.array_equal(now.view(np.uint8), self.before.view(np.uint8))


def _args(P, ov):
    return (P.gt.data_ptr(), P.gt_code.data_ptr(), P.dt.data_ptr(), P.dt_code.data_ptr(), P.gt_off.data_ptr(), P.dt_off.data_ptr(),
            P.ov_off.data_ptr(), ov.data_ptr(), P.n_img)


def run_device(case):
    """both entry points as kitti_eval._eval_class calls them, on sentinel-filled guarded outputs -> dict of host arrays"""
    lb = y3d.lib()
    P = KE.Packed(case.gts, case.dts)
    ov = torch.from_numpy(np.concatenate([case.ov, np.zeros(1, np.float32)])).cuda()   # the case's own table, never empty
    ncd, nk, n_img = len(case.cd), case.nk, P.n_img
    S, tg = ncd * nk, max(P.total_gt, 1)
    cd_d = torch.tensor(case.cd, dtype=torch.int32, device="cuda").reshape(-1, 2)
    mo_d = torch.from_numpy(case.mo.reshape(-1).copy()).cuda()
    tp, nvalid = Guarded(S * tg, torch.float32, float("-inf")), Guarded(ncd * n_img, torch.int32, -1)
    lb.kitti_eval_thresholds(*_args(P, ov), P.total_gt, case.metric, cd_d.data_ptr(), ncd, mo_d.data_ptr(), nk, tp.ptr, nvalid.ptr, ops.stream())
    torch.cuda.synchronize()
    tp_h, nv_h = tp.get().reshape(S, tg), nvalid.get().reshape(ncd, n_img)
    thr, nthr = np.zeros((S, NT), np.float32), np.zeros(S, np.int32)
    for s in range(S):   # the host's scan, as _eval_class runs it
        sc = np.sort(tp_h[s][tp_h[s] > -np.inf])[::-1]
        t = KE.get_thresholds(sc, int(nv_h[s // nk].sum()))
        assert len(t) <= NT
        thr[s, :len(t)], nthr[s] = t, len(t)
    thr_d, nthr_d = torch.from_numpy(thr).cuda(), torch.from_numpy(nthr).cuda()
    cnt = Guarded(S * NT * n_img * 3, torch.int32, CNT_FILL)
    sim, pr = Guarded(S * NT * n_img, torch.float64, float("nan")), Guarded(S * NT * 4, torch.float64, float("nan"))
    lb.kitti_eval_counts(*_args(P, ov), case.metric, cd_d.data_ptr(), ncd, mo_d.data_ptr(), nk, thr_d.data_ptr(), nthr_d.data_ptr(),
                         int(case.aos), cnt.ptr, sim.ptr, pr.ptr, ops.stream())
    torch.cuda.synchronize()
    return {"tp_score": tp_h, "nvalid": nv_h, "thr": thr, "nthr": nthr, "cnt": cnt.get().reshape(S, NT, n_img, 3),
            "sim": sim.get().reshape(S, NT, n_img), "pr": pr.get().reshape(S, NT, 4)}


def run_ref(case):
    scene = R.Scene(case.gts, case.dts)
    ov = scene.split(case.ov)
    ncd, nk, n_img = len(case.cd), case.nk, scene.n_img
    S, tg = ncd * nk, max(scene.total_gt, 1)
    out = {"tp_score": np.zeros((S, tg), np.float32), "nvalid": np.zeros((ncd, n_img), np.int64), "thr": np.zeros((S, NT), np.float32),
           "nthr": np.zeros(S, np.int32), "cnt": np.zeros((S, NT, n_img, 3), np.int64), "sim": np.zeros((S, NT, n_img)),
           "pr": np.zeros((S, NT, 4))}
    for r, (cls, diff) in enumerate(case.cd):
        for k in range(nk):
            e = R.eval_setting(scene, ov, cls, diff, case.metric, case.mo[r, k], case.aos)
            s, n = r * nk + k, len(e["thresholds"])
            out["tp_score"][s], out["nvalid"][r], out["nthr"][s] = e["tp_score"], e["nvalid"], n
            out["thr"][s, :n] = e["thresholds"]
            out["cnt"][s], out["sim"][s], out["pr"][s] = e["cnt"], e["sim"], e["pr"]
    return out


def compare(case, dev, ref):
    name = case.name
    assert np.array_equal(dev["nvalid"], ref["nvalid"]), name
    assert np.array_equal(dev["tp_score"].view(np.int32), ref["tp_score"].view(np.int32)), name   # -inf where the gt is no tp
    assert np.array_equal(dev["nthr"], ref["nthr"]) and np.array_equal(dev["thr"].view(np.int32), ref["thr"].view(np.int32)), name
    bad = np.argwhere(dev["cnt"] != ref["cnt"])
    assert bad.shape[0] == 0, (name, "cnt differs at (setting, threshold, image, tp|fp|fn)", bad[:8].tolist(),
                               dev["cnt"][tuple(bad[0])], ref["cnt"][tuple(bad[0])])
    assert not np.isnan(dev["sim"]).any() and not np.isnan(dev["pr"]).any(), (name, "an element was never written")
    assert np.array_equal(dev["pr"][..., :3], ref["pr"][..., :3]), name
    assert np.array_equal(dev["sim"] == -1.0, ref["sim"] == -1.0), name
    n_img = ref["sim"].shape[2]
    err = np.abs(dev["sim"] - ref["sim"])
    tol = (ref["cnt"][..., 0] + 1) * EPS
    print(f"{name}: sim worst {err.max():.3g} (bound there {tol.reshape(-1)[err.argmax()]:.3g})")
    assert (err <= tol).all(), (name, err.max())
    err = np.abs(dev["pr"][..., 3] - ref["pr"][..., 3])
    tol = (ref["pr"][..., 0] + n_img) * EPS
    print(f"{name}: pr[3] worst {err.max():.3g} (bound there {tol.reshape(-1)[err.argmax()]:.3g})")
    assert (err <= tol).all(), (name, err.max())
    if not case.aos:
        assert not dev["sim"].any() and not dev["pr"][..., 3].any(), name


def check(case):
    dev = run_device(case)
    compare(case, dev, run_ref(case))
    return dev


# ---------------------------------------------------------------------------------------------------------------------------------
# the statistics kernels on crafted overlap tables
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 3])
@pytest.mark.parametrize("nd,ng", C.CROWDED_SHAPES)
def test_crowded_image(nd, ng, nk):
    """assigned-detection bitmask words 0..7, gts denied a taken det of a later word, flag loads past 64 and past the block"""
    check(C.crowded(nd, ng, nk))


@pytest.mark.parametrize("nk,official", C.LANE_CASES)
def test_lane_counts(nk, official):
    """41 * nk lanes for nk = 1, 2, 3, 6; 9 (class, difficulty) rows in one launch; lanes t >= nthr write zeros"""
    dev = check(C.lanes(nk, official))
    for s in range(dev["nthr"].shape[0]):
        assert not dev["cnt"][s, dev["nthr"][s]:].any() and not dev["sim"][s, dev["nthr"][s]:].any()


@pytest.mark.parametrize("n_img", C.IMAGE_COUNTS)
def test_image_counts(n_img):
    """the image reduce past one stride of 256; images without gts, dets or either; AOS on; bit-identical from run to run"""
    case = C.images(n_img)
    a = check(case)
    b = run_device(case)
    for k in ("pr", "sim", "cnt", "tp_score", "nvalid"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_ties_and_boundaries():
    check(C.ties())


def test_full_recall_and_no_true_positive():
    dev = check(C.full_recall())
    assert dev["nthr"].tolist() == [41, 0] and not dev["pr"][1].any()


@pytest.mark.parametrize("case", C.flag_cases(), ids=repr)
def test_clean_data_edges(case):
    check(case)


@pytest.mark.parametrize("case", C.dontcare_cases(), ids=repr)
def test_dontcare_suppression(case):
    dev = check(case)
    if case.metric != 0:   # the same boxes under BEV / 3D: every unmatched det of the three images stays a false positive
        assert (dev["cnt"][:, 0, :, 1] == np.array([13, 3, 1])).all()


def test_rejected_arguments_write_nothing():
    """nk = 7 (41 * 7 lanes exceed the block) and metric = 3: Y3D_ERR_INVALID from both entry points, every output untouched"""
    dll = y3d.lib()._dll
    base = C.ties()
    P = KE.Packed(base.gts, base.dts)
    ov = torch.from_numpy(base.ov).cuda()
    for nk, metric in ((7, 0), (1, 3), (0, 0)):
        n = max(nk, 1)
        cd_d = torch.tensor([[0, 0]], dtype=torch.int32, device="cuda")
        mo_d = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
        outs = [Guarded(n * P.total_gt, torch.float32, float("-inf")), Guarded(P.n_img, torch.int32, -1),
                Guarded(n * NT * P.n_img * 3, torch.int32, CNT_FILL), Guarded(n * NT * P.n_img, torch.float64, float("nan")),
                Guarded(n * NT * 4, torch.float64, float("nan"))]
        thr_d, nthr_d = torch.zeros(n * NT, device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
        rc = dll.y3d_kitti_eval_thresholds(*_args(P, ov), P.total_gt, metric, cd_d.data_ptr(), 1, mo_d.data_ptr(), nk, outs[0].ptr, outs[1].ptr,
                                           ops.stream())
        assert rc == -1, (nk, metric, rc)   # Y3D_ERR_INVALID
        rc = dll.y3d_kitti_eval_counts(*_args(P, ov), metric, cd_d.data_ptr(), 1, mo_d.data_ptr(), nk, thr_d.data_ptr(), nthr_d.data_ptr(), 1,
                                       outs[2].ptr, outs[3].ptr, outs[4].ptr, ops.stream())
        assert rc == -1, (nk, metric, rc)
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs), (nk, metric)
    with pytest.raises(y3d.Y3DError, match="min-overlaps"):
        KE._eval_class(P, [0], [0], 0, np.full((7, 3, 1), 0.5), False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the overlap kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def geo_anno(rng, n, det, integer):
    """n Cars: 2D boxes on an integer grid (integer) and 3D boxes within 14 m"""
    x1, y1 = rng.integers(0, 64, n).astype(np.float32), rng.integers(0, 64, n).astype(np.float32)
    bbox = np.stack([x1, y1, x1 + rng.integers(1, 48, n), y1 + rng.integers(1, 48, n)], 1).astype(np.float32)
    if not integer:
        bbox += rng.random((n, 4)).astype(np.float32)
    a = C.anno(["Car"] * n, bbox=bbox, score=rng.random(n) if det else None)
    a["location"] = np.stack([rng.uniform(-6, 6, n), rng.uniform(1, 2, n), rng.uniform(2, 14, n)], 1).astype(np.float32)
    a["dimensions"] = np.stack([rng.uniform(0.5, 5, n), rng.uniform(1, 2, n), rng.uniform(0.5, 2.5, n)], 1).astype(np.float32)   # l, h, w
    a["rotation_y"] = rng.uniform(-math.pi, math.pi, n).astype(np.float32)
    return a


def iou2d_fp32(d, g):
    """image_box_overlap in fp32 without contraction, in the kernel's operation order (numpy rounds each operation to fp32)"""
    qa = (g[2] - g[0]) * (g[3] - g[1])
    iw = min(d[2], g[2]) - max(d[0], g[0])
    if not iw > 0:
        return np.float32(0)
    ih = min(d[3], g[3]) - max(d[1], g[1])
    if not ih > 0:
        return np.float32(0)
    return (iw * ih) / ((d[2] - d[0]) * (d[3] - d[1]) + qa - iw * ih)


def overlaps_into_sentinels(gts, dts, metric):
    P = KE.Packed(gts, dts)
    n = int(P.ov_off_np[-1])
    out = Guarded(n, torch.float32, float("nan"))
    y3d.lib().kitti_box_overlaps(metric, P.gt.data_ptr(), P.dt.data_ptr(), P.gt_off.data_ptr(), P.dt_off.data_ptr(), P.ov_off.data_ptr(),
                                 P.n_img, out.ptr, ops.stream())
    torch.cuda.synchronize()
    got = out.get()
    assert not np.isnan(got).any(), "a pair was never written"
    o = P.ov_off_np
    return [got[o[i]:o[i + 1]].reshape(len(dts[i]["name"]), len(gts[i]["name"])) for i in range(P.n_img)]


def overlap_images(integer):
    """65 x 67 pairs in one image (the 64-lane stride wraps 69 times), between images without gts, without dets and without either"""
    rng = np.random.default_rng(23)
    shapes = [(3, 4), (0, 5), (65, 67), (4, 0), (0, 0), (2, 2), (0, 0)]   # (n_dt, n_gt)
    return [geo_anno(rng, g, False, integer) for _, g in shapes], [geo_anno(rng, d, True, integer) for d, _ in shapes]


@pytest.mark.parametrize("integer", [True, False])
def test_overlap_kernel_2d_is_the_fp32_formula_bit_for_bit(integer):
    gts, dts = overlap_images(integer)
    got = overlaps_into_sentinels(gts, dts, 0)
    for i, o in enumerate(got):
        want = np.array([[iou2d_fp32(d, g) for g in gts[i]["bbox"]] for d in dts[i]["bbox"]], np.float32).reshape(o.shape)
        assert np.array_equal(o.view(np.int32), want.view(np.int32)), i
    assert (got[2] > 0).sum() > 1000 and (got[2] == 0).sum() > 100


def test_overlap_kernel_2d_exact_on_power_of_two_unions():
    """integer boxes, one inside the other, the larger area a power of two: the IoU is inter / 2^k, exact in fp32"""
    pairs = []   # (gt, dt)
    for a, b in ((3, 3), (4, 2), (5, 5), (1, 6), (10, 13)):
        big = [7, 5, 7 + 2 ** a, 5 + 2 ** b]
        for w, h in ((1, 1), (2 ** a, 1), (min(3, 2 ** a), 2 ** b), (2 ** a, 2 ** b), (2 ** a - 1, 2 ** b - 1), (1, 2 ** b)):
            small = [7 + 2 ** a - w, 5, 7 + 2 ** a, 5 + h]
            pairs += [(big, small), (small, big)]
    gts = [C.anno(["Car"], bbox=[g]) for g, _ in pairs]
    dts = [C.anno(["Car"], bbox=[d], score=[0.5]) for _, d in pairs]
    got = overlaps_into_sentinels(gts, dts, 0)
    for (g, d), o in zip(pairs, got):
        area = lambda r: (r[2] - r[0]) * (r[3] - r[1])
        want = Fraction(min(area(g), area(d)), max(area(g), area(d)))
        assert Fraction(float(o[0, 0])) == want, (g, d, float(o[0, 0]))


def test_overlap_kernel_rotated_against_fp64_clipping():
    """BEV and 3D IoU of every pair of the 65 x 67 image (boxes within 14 m) against fp64 polygon clipping, at the 1e-5 of
    test_hip_kitti_eval.py; the empty images around it write nothing"""
    gts, dts = overlap_images(False)
    box = lambda a, i: (*a["location"][i].tolist(), *a["dimensions"][i].tolist(), float(a["rotation_y"][i]))
    bev = lambda b: (b[0], b[2], b[3], b[5], b[6])
    for metric in (1, 2):
        got = overlaps_into_sentinels(gts, dts, metric)
        for i, o in enumerate(got):
            g_, d_ = [box(gts[i], a) for a in range(o.shape[1])], [box(dts[i], a) for a in range(o.shape[0])]
            want = np.array([[R.bev_iou(bev(g), bev(d)) if metric == 1 else R.iou3d(g, d) for g in g_] for d in d_]).reshape(o.shape)
            err = np.abs(o - want)
            print(f"metric {metric} image {i}: worst {err.max() if err.size else 0:.3g}")
            assert (err <= 1e-5).all(), (metric, i, err.max())
        assert (got[2] > 0).mean() > 0.08


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end at the validator's shape
# ---------------------------------------------------------------------------------------------------------------------------------
DIMS = {"Car": (3.9, 1.5, 1.6), "Van": (5.0, 2.2, 1.9), "Truck": (9.0, 3.2, 2.5), "Pedestrian": (0.85, 1.75, 0.65),
        "Person_sitting": (0.9, 1.3, 0.6), "Cyclist": (1.75, 1.75, 0.6), "DontCare": (1.0, 1.0, 1.0)}   # l, h, w


def validator_annos(n_img, n_det):
    rng = np.random.default_rng(300)
    names = ["Car"] * 6 + ["Pedestrian"] * 3 + ["Cyclist"] * 3 + ["Van", "Person_sitting", "Truck", "DontCare", "DontCare"]
    gts, dts = [], []
    for i in range(n_img):
        ng = 0 if i % 37 == 5 else int(rng.integers(2, 10))
        gn = rng.choice(names, ng)
        x1, y1 = rng.uniform(0, 1100, ng), rng.integers(100, 250, ng).astype(np.float64)
        bh = rng.choice([25.0, 40.0, 30.5, 60.25, 90.0, 140.0], ng)
        g = C.anno(gn, bbox=np.stack([x1, y1, x1 + rng.uniform(20, 200, ng), y1 + bh], 1), alpha=rng.uniform(-3, 3, ng),
                   occ=rng.choice([0, 0, 0, 1, 2, 3], ng), trunc=rng.choice([0.0, 0.0, 0.1, 0.2, 0.4, 0.6], ng))
        g["location"] = np.stack([rng.uniform(-15, 15, ng), rng.uniform(1, 2.5, ng), rng.uniform(5, 50, ng)], 1).astype(np.float32)
        g["dimensions"] = (np.array([DIMS[n] for n in gn]).reshape(ng, 3) * rng.uniform(0.9, 1.1, (ng, 3))).astype(np.float32)
        g["rotation_y"] = rng.uniform(-math.pi, math.pi, ng).astype(np.float32)
        real = [j for j in range(ng) if gn[j] != "DontCare"]
        src = rng.choice(real + [-1], n_det) if real else np.full(n_det, -1)   # -1: a detection of nothing
        d = C.anno(["Car"] * n_det, score=np.round(rng.uniform(0.05, 1, n_det), 2), alpha=rng.uniform(-3, 3, n_det))
        for j, s in enumerate(src):
            if s < 0:
                x, y = rng.uniform(0, 1100), float(rng.integers(100, 250))
                d["name"][j] = rng.choice(["Car", "Pedestrian", "Cyclist"])
                d["bbox"][j] = [x, y, x + rng.uniform(20, 200), y + rng.choice([25.0, 40.0, 24.0, 70.5])]
                d["location"][j] = [rng.uniform(-15, 15), rng.uniform(1, 2.5), rng.uniform(5, 50)]
                d["dimensions"][j] = np.array(DIMS[str(d["name"][j])]) * rng.uniform(0.9, 1.1, 3)
                d["rotation_y"][j] = rng.uniform(-math.pi, math.pi)
            else:
                d["name"][j] = gn[s] if rng.random() > 0.1 else rng.choice(["Car", "Pedestrian", "Cyclist"])
                d["bbox"][j] = g["bbox"][s] + rng.normal(0, 3, 4)
                d["location"][j] = g["location"][s] + rng.normal(0, [0.08, 0.05, 0.15])
                d["dimensions"][j] = g["dimensions"][s] * (1 + rng.normal(0, 0.03, 3))
                d["rotation_y"][j] = g["rotation_y"][s] + rng.normal(0, 0.05)
                d["alpha"][j] = g["alpha"][s] + rng.normal(0, 0.3)
        gts.append(g), dts.append(d)
    return gts, dts


def test_validator_shape_end_to_end():
    """300 images x 50 detections: get_official_eval_result for the three classes against the restatement fed the device's own
    overlaps, which separates the matching from the geometry.  Every AP within 1e-9, NaN pattern equal."""
    gts, dts = validator_annos(300, 50)
    P = KE.Packed(gts, dts)
    scene = R.Scene(gts, dts)
    ovs = [scene.split(P.overlaps(m).cpu().numpy()) for m in range(3)]
    seen = 0
    for cls in ("Car", "Pedestrian", "Cyclist"):
        got = KE.get_official_eval_result(gts, dts, cls, _packed=P)["detail"][cls]
        want = R.official_detail(scene, ovs, cls)
        assert set(got) == set(want) and "aos" in got, (cls, set(got) ^ set(want))
        for k in want:
            g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (cls, k, g, w)
            assert np.allclose(g, w, rtol=0, atol=1e-9, equal_nan=True), (cls, k, g, w)
            seen += int((w[~np.isnan(w)] > 1).sum())
    assert seen >= 20   # the set is not degenerate: most APs are well above zero
