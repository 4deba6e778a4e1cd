"""CPU: the sequential restatement of the KITTI AP matching (tests/kitti_eval_ref.py) pinned to the reference's own tables
(tests/golden/kitti_eval.npz), the case lists of tests/test_hip_kitti_eval_edges.py checked - with the restatement alone - to reach the
edges they are named for, and the host layer's refusal of a seventh min-overlap (no GPU needed)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import kitti_eval_cases as C
import kitti_eval_ref as R
from test_kitti_eval_host import fixture_annos

F = np.float32


def _assert_detail(got, z, prefix):
    keys = [k[len(prefix):] for k in z.files if k.startswith(prefix)]
    assert keys and set(keys) == set(got), (prefix, set(keys) ^ set(got))
    worst = 0.0
    for k in keys:
        want, g = z[prefix + k], np.asarray(got[k], np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(want)), (prefix, k, g, want)
        assert np.allclose(g, want, rtol=0, atol=1e-9, equal_nan=True), (prefix, k, g, want)
        if not np.isnan(want).all():
            worst = max(worst, float(np.nanmax(np.abs(g - want))))
    return worst


def test_restatement_reproduces_every_fixture_table():
    """annos + the fixture's own ov0 / ov1 / ov2 blocks -> every detail40, detail11 and subset40 table of the reference within 1e-9
    (measured: 3.6e-14), aos included, NaN pattern equal"""
    z = np.load(os.path.join(GOLDEN, "kitti_eval.npz"))
    gts, dts = fixture_annos()
    scene = R.Scene(gts, dts)
    ovs = [scene.split(z[f"ov{m}"]) for m in range(3)]
    worst = 0.0
    for mode in (40, 11):
        for cls in ("Car", "Pedestrian", "Cyclist"):
            worst = max(worst, _assert_detail(R.official_detail(scene, ovs, cls, mode), z, f"detail{mode}|{cls}|"))
    sub = R.Scene(gts[:7], dts[:7])   # image blocks lie back to back, so the first 7 images' overlaps are a prefix
    worst = max(worst, _assert_detail(R.official_detail(sub, [sub.split(z[f"ov{m}"]) for m in range(3)], "Car", 40), z, "subset40|Car|"))
    print(f"largest distance to the reference's tables: {worst:.3g}")


def test_name_codes_and_geometry_helpers():
    assert R.name_codes(["Car", "car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "tractor", "Trailer", "Truck", "DontCare",
                         "dontcare"]).tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 15, 7]
    sq = (0.0, 10.0, 2.0, 2.0, 0.0)
    assert abs(R.bev_iou(sq, sq) - 1) < 1e-12 and abs(R.bev_iou(sq, (1.0, 10.0, 2.0, 2.0, 0.0)) - 1 / 3) < 1e-12
    assert abs(R.bev_iou(sq, (0.0, 10.0, 2.0, 2.0, np.pi / 4)) - (8 * (np.sqrt(2) - 1)) / (8 - 8 * (np.sqrt(2) - 1))) < 1e-12
    assert abs(R.iou3d((0, 2, 10, 2, 2, 2, 0), (0, 1, 10, 2, 2, 2, 0)) - 1 / 3) < 1e-12
    assert R.mAP(np.ones(41), 40) == 100 and abs(R.mAP(np.ones(41), 11) - 100) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# reachability: what the device cases claim to exercise, established from the restatement alone
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(case, with_trace=True):
    scene = R.Scene(case.gts, case.dts)
    ov = scene.split(case.ov)
    out = {}
    for r, (cls, diff) in enumerate(case.cd):
        for k in range(case.nk):
            tr = {} if with_trace else None
            out[r, k] = (R.eval_setting(scene, ov, cls, diff, case.metric, case.mo[r, k], case.aos, tr), tr)
    return scene, out


def _events(tr, key, img=None, passes=("thresholds", "counts")):
    """all trace entries `key` of the threshold pass and / or the counting pass"""
    out = []
    for i, per in tr.items():
        if img is not None and i != img:
            continue
        for t, d in per.items():
            if ("thresholds" if t == "thresholds" else "counts") in passes:
                out += d.get(key, [])
    return out


def test_crowded_cases_reach_the_high_bitmask_words():
    top = {}
    for nk in (1, 3):
        for nd, ng in C.CROWDED_SHAPES:
            _, out = _run(C.crowded(nd, ng, nk))
            for (r, k), (e, tr) in out.items():
                for passes in (("thresholds",), ("counts",)):
                    det = [j for _, j in _events(tr, "assigned", passes=passes)]
                    den = [j for _, j in _events(tr, "denied", passes=passes)]
                    key = (nd, ng, passes[0])
                    a, d = top.get(key, (-1, -1))
                    top[key] = (max([a] + det), max([d] + den))
                assert len(e["thresholds"]) > 0
    for p in ("thresholds", "counts"):
        assert top[31, 5, p][0] == 30 and top[32, 5, p][0] == 31          # the last bit of word 0
        assert top[33, 34, p] == (32, 32)                                    # first bit of word 1, assigned and then denied
        assert top[64, 65, p][0] == 63 and top[65, 64, p] == (64, 64)       # word 2; nd and ng on either side of the 64-lane stride
        assert top[255, 3, p] == (254, 254) and top[256, 256, p] == (255, 255)   # word 7 (index >= 224)
    # a gt denied a det of word >= 1 goes on to a det of its own in the counting pass, and some are left without one
    _, out = _run(C.crowded(256, 256, 1))
    e, tr = out[0, 0]
    denied_gts = {i for i, j in _events(tr, "denied", passes=("counts",)) if j >= 32}
    assigned_gts = {i for i, _ in _events(tr, "assigned", passes=("counts",))}
    assert denied_gts & assigned_gts and denied_gts - assigned_gts
    assert e["cnt"][:, 0, 2].max() > 0 and e["cnt"][:, 0, 1].max() > 0      # false negatives and false positives both occur
    assert len(set(C.crowded(256, 256, 1).dts[0]["score"].tolist())) == 13   # tied scores


def test_tie_and_boundary_cases_reach_their_branches():
    case = C.ties()
    scene, out = _run(case)
    e, tr = out[0, 0]   # Car easy at min-overlap 0.5
    # image 0: score tie and overlap tie, both resolved to the first det; gt 1 then takes det 1
    assert (0, 0, 1) in _events(tr, "score_tie", 0, ("thresholds",)) and (0, 0, 1) in _events(tr, "ov_tie", 0, ("counts",))
    assert set(_events(tr, "assigned", 0, ("thresholds",))) == {(0, 0), (1, 1)}
    assert set(_events(tr, "assigned", 0, ("counts",))) == {(0, 0), (1, 1)}
    # image 1: the ignored det is taken, replaced by the equal same-class det, that by the better one; taken and kept; not taken
    assert (0, 0) in _events(tr, "aid_taken", 1) and (0, 0, 1) in _events(tr, "aid_replaced", 1)
    assert (0, 2) in _events(tr, "assigned", 1, ("counts",)) and (1, 3) in _events(tr, "assigned", 1, ("counts",))
    assert (1, 3) in _events(tr, "aid_taken", 1) and all(i != 1 for i, _, _ in _events(tr, "aid_replaced", 1))
    last = tr[1][len(e["thresholds"]) - 1]   # at the lowest threshold every det is in play
    assert (2, 4) in last["assigned"] and all(i != 2 for i, _ in last["aid_taken"])
    assert (0, 0, 1) in _events(tr, "score_tie", 1, ("thresholds",))   # and the tied, ignored det 0 keeps gt 0 from being a tp
    g0 = int(scene.gt_off[1])
    assert e["tp_score"][g0] == -np.inf and e["tp_score"][g0 + 2] == F(0.5)
    # image 2: overlaps exactly at 0.5 and 0.25 are below them; float32(0.7) is below 0.7, float32(0.3) above 0.3; one ulp flips each
    want = {0: [0, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0],    # min-overlap 0.5
            1: [1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0],    # 0.25
            2: [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0],    # 0.7
            3: [1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0]}    # 0.3
    g0 = int(scene.gt_off[2])
    for k, w in want.items():
        ek, trk = out[0, k]
        got = (ek["tp_score"][g0:g0 + len(w)] > -np.inf).astype(int).tolist()
        assert got == w, (k, got)
        at = [(i, above) for i, j, above in _events(trk, "at_min", 2, ("thresholds",))]
        assert at == [({0: 0, 1: 1, 2: 2, 3: 5}[k], k == 3)], (k, at)
    # a det's score equals the threshold in every setting with a threshold (the thresholds are scores), and the thresholds tie (image 3)
    for (r, k), (ek, trk) in out.items():
        assert len(ek["thresholds"]) > 0 and _events(trk, "at_thresh", passes=("counts",))
        assert (ek["thresholds"] == F(0.375)).sum() >= 2


def test_flag_cases_reach_every_flag_and_edge():
    gts, dts, _ = C.flag_images()
    nvar = len(C.HEIGHT_EDGES) + 4 + len(C.TRUNC_EDGES)
    for c, (g, d, d2) in enumerate(zip(gts[0::2], dts[0::2], dts[1::2])):
        f = [R.flags(g, d, c, diff)[0] for diff in range(3)]
        h0, o0, t0 = 0, len(C.HEIGHT_EDGES), len(C.HEIGHT_EDGES) + 4
        # gt heights 40, 40+, 40-, 25, 25+, 25-: `<=` ignores the edge itself
        assert [f[0][h0 + i] for i in range(6)] == [1, 0, 1, 1, 1, 1]
        assert [f[1][h0 + i] for i in range(6)] == [0, 0, 0, 1, 0, 1] == [f[2][h0 + i] for i in range(6)]
        # occlusion 0..3 against limits 0, 1, 2
        assert [[f[diff][o0 + i] for i in range(4)] for diff in range(3)] == [[0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]]
        # truncation float32(0.15) > 0.15 and float32(0.3) > 0.3 in double (ignored), 0.5 is exact (kept); one ulp either side
        assert [[f[diff][t0 + i] for i in range(9)] for diff in range(3)] == [[1, 1, 0, 1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 0, 1, 1, 1],
                                                                            [0, 0, 0, 0, 0, 0, 0, 1, 0]]
        # neighbour classes: Van next to Car, Person_sitting next to Pedestrian, nothing next to Cyclist; "car" is Car; DontCare is out
        names = f[1][nvar:]
        assert names == [[0, 1, -1, -1, -1, 0, -1, -1], [-1, -1, 0, 1, -1, -1, -1, -1], [-1, -1, -1, -1, 0, -1, -1, -1]][c]
        assert len(R.flags(g, d, c, 0)[2]) == 1
        # det heights 40, 40+, 40-, 25, 25+, 25-, their negatives, -10, 50 and a neighbour class: `<` keeps the edge itself
        fd = [R.flags(gts[2 * c + 1], d2, c, diff)[1] for diff in range(3)]
        assert fd[0] == [0, 0, 1, 1, 1, 1] * 2 + [1, 0, -1]
        assert fd[1] == [0, 0, 0, 0, 0, 1] * 2 + [1, 0, -1] == fd[2]
    seen_gt, seen_dt = set(), set()
    for case in C.flag_cases():
        scene, out = _run(case, with_trace=False)
        for cls, diff in case.cd:
            for ig, idt, _ in scene.flags(cls, diff):
                seen_gt |= set(ig)
                seen_dt |= set(idt)
        for (r, k), (e, _) in out.items():
            assert len(e["thresholds"]) > 0 and e["pr"][:, 2].max() > 0
    assert seen_gt == {-1, 0, 1} and seen_dt == {-1, 0, 1}
    # what the double comparison decides differently from an fp32 one
    assert float(F(0.15)) > 0.15 and not F(0.15) > F(0.15) and float(F(0.3)) > 0.3 and float(F(0.7)) < 0.7


def test_dontcare_cases_suppress_exactly_above_the_min_overlap():
    gts, dts, _ = C.dontcare_images()
    dc = R.dontcare_overlaps(dts[0]["bbox"], gts[0]["bbox"][1:])
    best = [max(r) for r in dc]
    assert best == [0, 0] + [c / 64 for c in (15, 16, 17, 31, 32, 33, 63, 64)] + [24 / 64, 40 / 64, 40 / 64, 0]
    assert sorted(dc[10])[-2:] == [24 / 64, 24 / 64]    # two boxes of 3/8 each: their sum would pass 0.5 and 0.7, the larger does not
    dc1 = [max(r) for r in R.dontcare_overlaps(dts[1]["bbox"], gts[1]["bbox"][1:])]
    assert dc1 == [0, float(C.DOWN(0.7)), float(F(0.7)), float(C.UP(0.7))]
    cases = C.dontcare_cases()
    for case in cases:
        scene, out = _run(case)
        for (r, k), (e, tr) in out.items():
            n = len(e["thresholds"])
            assert n > 0
            sup = [sorted(set(_events({i: tr[i]}, "suppressed", passes=("counts",)))) for i in range(3)]
            if case.metric != 0:
                assert sup == [[], [], []] and e["cnt"][0, :, 1].tolist() == [13, 3, 1]   # same boxes, other metrics: nothing suppressed
                continue
            want0 = {0: [8, 9], 1: [7, 8, 9, 11, 12], 2: [4, 5, 6, 7, 8, 9, 10, 11, 12]}[k]
            want1 = {0: [3], 1: [1, 2, 3], 2: [1, 2, 3]}[k]
            assert sup == [want0, want1, []], (k, sup)
            assert e["cnt"][0, :, 1].tolist() == [13 - len(want0), 3 - len(want1), 1]
            assert _events({0: tr[0]}, "kept", passes=("counts",))   # taken and not taken side by side


def test_lane_and_image_cases_reach_their_paths():
    seen_n = set()
    for nk, official in C.LANE_CASES:
        case = C.lanes(nk, official)
        assert case.nk == nk and len(case.cd) == 9
        for r in range(9):
            assert official or len(set(case.mo[r].tolist())) == nk   # distinct per k
        _, out = _run(case, with_trace=False)
        ns = [len(e["thresholds"]) for e, _ in out.values()]
        seen_n |= set(ns)
        assert min(ns) < 41 and max(ns) > 0 and sum(n > 0 for n in ns) >= len(ns) // 2
    for n_img in C.IMAGE_COUNTS:
        case = C.images(n_img)
        ng, nd = np.array([len(a["name"]) for a in case.gts]), np.array([len(a["name"]) for a in case.dts])
        assert len(case.gts) == n_img
        if n_img > 1:
            assert ((ng == 0) & (nd > 0)).any() and ((nd == 0) & (ng > 0)).any() and ((ng == 0) & (nd == 0)).any()
        _, out = _run(case, with_trace=False)
        e = out[0, 1][0]
        assert len(e["thresholds"]) > 0
        quiet = (e["cnt"][0, :, 0] == 0) & (e["cnt"][0, :, 1] == 0)
        assert (e["sim"][0][quiet] == -1).all() and (n_img == 1 or quiet.any())    # tp = fp = 0 under AOS
        assert (e["sim"][0][~quiet] >= 0).all() and e["sim"][0].max() > 0
        if n_img > 256:   # images past the first 256 carry counts of their own
            t = len(e["thresholds"]) - 1
            assert e["cnt"][t, 256].min() > 0 and e["sim"][t, 256] > 0
    _, out = _run(C.full_recall(), with_trace=False)
    assert len(out[0, 0][0]["thresholds"]) == 41 and len(out[0, 1][0]["thresholds"]) == 0   # nthr = 41; no true positive at all
    assert out[0, 1][0]["pr"].sum() == 0 and (out[0, 1][0]["tp_score"] == -np.inf).all()
    assert seen_n & set(range(1, 41))


def test_a_seventh_min_overlap_is_refused_by_the_host_layer():
    import yolov10_3d_amd as y3d
    from yolov10_3d_amd import kitti_eval as KE
    with pytest.raises(y3d.Y3DError, match="min-overlaps"):
        KE._eval_class(None, [0], [0, 1, 2], 0, np.full((7, 3, 1), 0.5), False)   # refused before the packed annos are touched
