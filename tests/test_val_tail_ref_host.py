"""CPU: the references of val_tail_ref.py against independent statements (Pillow for the crop, scikit-learn for the fusion), and
every condition the device tests of test_hip_val_tail.py rely on, computed from the references alone: the ambiguity share of each
fusion case against its cap, the clearances of the expf / threshold decisions, and that the case tables reach what they claim."""
import math

import numpy as np
import pytest
import torch

import val_tail_ref as V

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- image crop
def _pillow(img, img2, flip, tinv, out_wh):
    from PIL import Image
    a = Image.fromarray(img)
    if flip:
        a = a.transpose(Image.FLIP_LEFT_RIGHT)
    if img2 is not None:
        b = Image.fromarray(img2)
        if flip:
            b = b.transpose(Image.FLIP_LEFT_RIGHT)
        a = Image.blend(a, b, 0.5)
    return np.asarray(a.transform(tuple(out_wh), Image.AFFINE, tuple(float(v) for v in tinv), resample=Image.BILINEAR))


@pytest.mark.parametrize("name", list(V.AUG_CASES))
def test_image_aug_ref_equals_pillow(name):
    """mirror, blend and affine crop of the restatement against Pillow's own, every pixel, with and without flip and partner"""
    pytest.importorskip("PIL")
    H, W, out_wh, tinv = V.AUG_CASES[name]
    img, part = V.aug_sources(H, W, 11)
    for flip in (0, 1):
        for p in (None, part):
            want = _pillow(img, p, flip, tinv, out_wh)
            got = V.kitti_image_aug(img, p, flip, tinv, out_wh)
            assert got.shape == (out_wh[1], out_wh[0], 3) and got.dtype == np.uint8
            assert np.array_equal(got, want), f"{name} flip {flip} partner {p is not None}: {int((got != want).sum())} values differ"


def test_image_aug_blend_pairs_equal_pillow():
    """all 256 x 256 pairs (a, b) of the mixup blend"""
    pytest.importorskip("PIL")
    img, part = V.blend_pair_sources()
    assert len({(int(a), int(b)) for a, b in zip(img[..., 0].ravel(), part[..., 0].ravel())}) == 65536
    ident = [1, 0, 0, 0, 1, 0]
    for flip in (0, 1):
        assert np.array_equal(V.kitti_image_aug(img, part, flip, ident, (256, 256)), _pillow(img, part, flip, ident, (256, 256)))


def test_image_aug_cases_reach_every_branch():
    """from the maps alone: outside pixels, negative coordinates, clamped neighbours at the left, right and top border, the missing
    y + 1 row, four distinct taps; off-diagonal maps, odd outputs, the all-zero output, the second trip of the grid-stride loop"""
    reach = {n: V.aug_reach(H, W, o, t) for n, (H, W, o, t) in V.AUG_CASES.items()}
    for key in ("outside", "neg", "clamp_l", "clamp_r", "clamp_t", "no_row", "inner"):
        assert sum(r[key] for r in reach.values()) >= 2, f"fewer than two cases reach `{key}`"
    assert reach["half-pixel"]["neg"] and reach["half-pixel"]["clamp_l"] and reach["upscale-odd"]["no_row"]
    assert reach["identity"]["outside"] and reach["identity"]["inner"]
    H, W, o, t = V.AUG_CASES["all-outside"]
    img, part = V.aug_sources(H, W, 11)
    assert not V.kitti_image_aug(img, part, 1, t, o).any() and not reach["all-outside"]["inner"]
    assert any(t[1] != 0 and t[3] != 0 for _, _, _, t in V.AUG_CASES.values())            # off-diagonal terms
    assert any(t[0] < 0 for _, _, _, t in V.AUG_CASES.values())                            # a mirroring map
    assert any(o[0] % 2 and o[1] % 2 and o[0] % 4 for _, _, o, _ in V.AUG_CASES.values())   # both odd, width no multiple of 4
    assert {(V.AUG_CASES[n][0], V.AUG_CASES[n][1]) for n in ("src-1x1", "src-one-row", "src-one-column")} == {(1, 1), (1, 8), (8, 1)}
    sizes = {V.AUG_CASES[n][:2] for n in V.AUG_MIXED}
    assert len(sizes) == len(V.AUG_MIXED) and 0 < sum(V.AUG_MIXED_PARTNER) < len(V.AUG_MIXED) and 0 < sum(V.AUG_MIXED_FLIP) < len(V.AUG_MIXED)
    assert any(f and not p for f, p in zip(V.AUG_MIXED_FLIP, V.AUG_MIXED_PARTNER)) and any(p and not f for f, p in zip(V.AUG_MIXED_FLIP, V.AUG_MIXED_PARTNER))
    B, _, _, (ow, oh) = V.AUG_BIG
    assert 2048 * 256 < B * oh * ow < 2 * 2048 * 256
    assert np.array_equal(V.aug_float(np.full((1, 1, 3), 255, np.uint8)), np.ones((3, 1, 1), F32))


# ---------------------------------------------------------------------------------------------------------------- depth fusion
def _votes(O, M, b, j, thres, iou_thres):
    """the voters of one-to-one row (b, j), written from `kde_fuse_depth`'s docstring with scalar float32 arithmetic"""
    C = O.shape[2]
    o = O[b, j].numpy()
    d, s = [], []
    if F32(math.exp(-float(o[C - 3]))) > thres:
        d.append(o[C - 4])
        s.append(o[C - 3])
    own = len(d) == 1
    for q in M[b].numpy():
        iw, ih = max(F32(0), min(o[2], q[2]) - max(o[0], q[0])), max(F32(0), min(o[3], q[3]) - max(o[1], q[1]))
        inter = F32(iw * ih)
        iou = inter / (F32((o[2] - o[0]) * (o[3] - o[1])) + F32((q[2] - q[0]) * (q[3] - q[1])) - inter + F32(1e-7))
        if iou > iou_thres and q[C - 1] == o[C - 1] and F32(math.exp(-float(q[C - 3]))) > thres:
            d.append(q[C - 4])
            s.append(q[C - 3])
    return np.array(d, F32), np.array(s, F32), own


SK_CASES = ["crowded-mixed-33", "nprop-2", "nprop-257", "nprop-500-small", "c8-mixed-33", "own-excluded", "hi-eq-lo", "tie2", "iou-boundary",
            "thres-boundary"]


@pytest.mark.parametrize("name", SK_CASES)
def test_fusion_ref_equals_sklearn_statement(name):
    """vote sets by scalar arithmetic, the density by scikit-learn's KernelDensity(bandwidth="silverman") with the normalised depth
    scores as sample weights, on np.linspace between the float32 extreme votes: same vote count, same proposals bit for bit, the same
    log-density up to its additive constant, and the same pick wherever the margin is above rounding"""
    sk = pytest.importorskip("sklearn.neighbors")
    B, K, KM, nprop, fam, C, tau, cap = V.FUSION_CASES[name]
    O, M, rows = V.fusion_reference(name)
    thres, iou_thres = V.fusion_thresholds(name)
    fused = V.kde_fuse_depth(O, M, thres, iou_thres, nprop)
    for idx, r in enumerate(rows):
        b, j = divmod(idx, K)
        d, u, own = _votes(O, M, b, j, thres, iou_thres)
        assert (len(d), own) == (r["n"], r["own"]), f"{name} row {(b, j)}: {len(d)} voters, reference {r['n']}"
        if len(d) <= 1:
            assert fused[b, j, C - 4].item() == O[b, j, C - 4].item()
            continue
        s = torch.exp(-torch.from_numpy(u))
        w = (s / s.sum()).numpy().astype(np.float64)
        grid = np.linspace(d.min(), d.max(), nprop)
        assert grid.dtype == F32 and np.array_equal(grid.view(np.int32), r["grid"].view(np.int32)), f"{name} row {(b, j)}: proposals differ"
        kde = sk.KernelDensity(bandwidth="silverman", kernel="gaussian").fit(d.astype(np.float64)[:, None], sample_weight=w)
        ld = kde.score_samples(grid.astype(np.float64)[:, None])
        assert float(np.abs((ld - ld.max()) - (r["ld"] - r["ld"].max())).max()) <= 1e-9, f"{name} row {(b, j)}: log-densities differ"
        if r["margin"] > 1e-9:
            assert grid[int(np.argmax(ld))] == r["grid"][r["pick"]]
        assert fused[b, j, C - 4].numpy().view(np.int32) == r["grid"][r["pick"]].view(np.int32)


@pytest.mark.parametrize("name", list(V.FUSION_CASES))
def test_fusion_case_conditions(name, capsys):
    """what the device test relies on, from the reference alone: restate's fused tensor passes the device test's own assertions; rows
    with a margin under tau stay under the case's cap; every exp(-u) is clear of the threshold by 1e-5 (the planted exact boundary
    aside); the case's counts are printed for the record"""
    B, K, KM, nprop, fam, C, tau, cap = V.FUSION_CASES[name]
    O, M, rows = V.fusion_reference(name)
    thres, iou_thres = V.fusion_thresholds(name)
    assert O.shape == (B, K, C) and M.shape == (B, KM, C) and KM <= V.FUSION_KM_MAX
    ref = V.kde_fuse_depth(O, M, thres, iou_thres, nprop)
    V.check_fusion(ref, O, rows, tau, name)
    for b in range(B):  # the reference's pick is the depth it returns
        for j in range(K):
            r = rows[b * K + j]
            if r["n"] > 1:
                assert ref[b, j, C - 4].numpy().view(np.int32) == r["grid"][r["pick"]].view(np.int32)
    fused, amb, mmin = V.fusion_stats(rows, tau)
    with capsys.disabled():
        print(f"\n[fusion] {name}: (B, K, KM, nprop, C) = {(B, K, KM, nprop, C)}, tau {tau:g}: {fused} fused rows of {B * K}, {amb} with margin "
              f"<= tau, smallest margin {mmin:.3e}, votes {min(r['n'] for r in rows)}..{max(r['n'] for r in rows)}")
    if cap is not None:
        assert amb <= cap * fused, f"{name}: {amb} of {fused} fused rows have a margin <= {tau:g}; the cap is {cap:.0%}"
    us = torch.cat((O[..., C - 3].reshape(-1), M[..., C - 3].reshape(-1))).double()
    gap = (torch.exp(-us) - thres).abs()
    if name == "thres-boundary":
        assert int((us == 0).sum()) >= 3          # the planted u = 0: exp(-0) = 1 = thres on both sides, exactly
        gap = gap[us != 0]
    assert float(gap.min()) >= 1e-5 * thres, f"{name}: an exp(-u) is {float(gap.min()):.2e} from the threshold"


def test_fusion_checker_rejects_wrong_depths():
    """the device test's assertions fail on: a fused depth moved to the neighbouring proposal, a depth off the grid by one ulp, a fused
    row left alone, an unfused row changed, another column touched"""
    name = "crowded-mixed-33"
    B, K, KM, nprop, fam, C, tau, cap = V.FUSION_CASES[name]
    O, M, rows = V.fusion_reference(name)
    good = V.kde_fuse_depth(O, M, *V.fusion_thresholds(name), nprop)
    r = rows[0]
    assert r["n"] > 1 and r["margin"] > tau and 0 < r["pick"] < nprop - 1
    for wrong in (float(r["grid"][r["pick"] + 1]), float(np.nextafter(r["grid"][r["pick"]], F32(1e9))), float(O[0, 0, C - 4])):
        bad = good.clone()
        bad[0, 0, C - 4] = wrong
        with pytest.raises(AssertionError):
            V.check_fusion(bad, O, rows, tau, name)
    bad = good.clone()
    bad[0, 1, 5] += 1
    with pytest.raises(AssertionError):
        V.check_fusion(bad, O, rows, tau, name)
    O2, M2, rows2 = V.fusion_reference("nomatch")
    bad = O2.clone()
    bad[1, 2, 33] = float(np.nextafter(F32(bad[1, 2, 33]), F32(1e9)))
    with pytest.raises(AssertionError):
        V.check_fusion(bad, O2, rows2, V.TAU_MIXED, "nomatch")


def test_fusion_cases_reach_what_they_claim():
    """counted from the reference: every class of vote count, the own vote excluded, hi == lo, each strict boundary, the block edge of
    the proposal loop"""
    R = {n: V.fusion_reference(n)[2] for n in V.FUSION_CASES}
    ns = [r["n"] for rows in R.values() for r in rows]
    assert {0, 1, 2} <= set(ns) and max(ns) > 16
    assert all(r["n"] >= 17 for n in ("crowded-equal-500", "crowded-mixed-33", "crowded-mixed-64") for r in R[n])
    assert {r["n"] for r in R["sparse-mixed-33"]} >= {0, 1, 2, 3}
    assert all(r["n"] <= 1 for n in ("km1", "nomatch") for r in R[n])
    km1 = R["km1"]
    assert (km1[0]["n"], km1[0]["own"], km1[0]["matched"]) == (1, False, 1) and km1[1]["n"] == 0   # the one vote is the one-to-many row's
    assert all(r["matched"] == 0 for r in R["nomatch"])
    assert all(r["n"] >= 3 and not r["own"] for r in R["own-excluded"])
    O = V.fusion_reference("own-excluded")[0]
    assert all(float(r["hi"]) < 100 < float(O[0, j, 33]) for j, r in enumerate(R["own-excluded"]))   # the own depth would move `hi`
    assert all(r["n"] > 1 and r["lo"] == r["hi"] and r["margin"] == math.inf and not r["equal_weights"] for r in R["hi-eq-lo"])
    assert all(r["n"] == 2 and r["margin"] <= V.TAU_EQUAL and r["equal_weights"] for r in R["tie2"])
    assert [r["own"] for r in R["tie2"]] == [True, False]
    assert np.array_equal(R["tie2"][0]["grid"], 10 + np.arange(33, dtype=F32) / 8)
    assert all(r["equal_weights"] for r in R["crowded-equal-500"])
    # strict boundaries: the IoU of the planted pair IS the threshold, exp(-0) IS the threshold, and neither votes
    O, M, rows = V.fusion_reference("iou-boundary")
    iou = V.box_iou_xyxy(O[0, :, :4], M[0, :, :4])
    assert iou[0, 0].item() == V.IOU_THRES and iou[1, 1].item() > V.IOU_THRES
    assert [(r["n"], r["matched"]) for r in rows] == [(1, 0), (2, 1), (1, 0)]
    lower = V.fusion_rows(O, M, V.THRES, float(np.nextafter(F32(V.IOU_THRES), F32(0))), 33)   # had the boundary pair voted, it would show
    assert lower[0]["n"] == 2 and lower[0]["grid"][lower[0]["pick"]] != O[0, 0, 33].item()
    assert rows[1]["grid"][rows[1]["pick"]] != O[0, 1, 33].item()
    assert [(r["n"], r["own"]) for r in R["thres-boundary"]] == [(0, False), (2, False), (2, True)]
    O, M, rows = V.fusion_reference("thres-boundary")
    lower = V.fusion_rows(O, M, float(np.nextafter(F32(1), F32(0))), V.IOU_THRES, 33)             # likewise for exp(-0) = thres
    assert [r["n"] for r in lower] == [3, 3, 3]
    assert all(a["grid"][a["pick"]] != b["grid"][b["pick"]] for a, b in zip(lower[1:], rows[1:]))
    assert V.FUSION_THRES["thres-boundary"] == 1.0 and math.exp(-0.0) == 1.0
    nprops = {c[3] for c in V.FUSION_CASES.values()}
    assert {2, 257, 500, 33, 64} <= nprops
    assert V.FUSION_CASES["large-km"][2] == 3800 < V.FUSION_KM_MAX and 8 in {c[5] for c in V.FUSION_CASES.values()}
    assert 16 * V.FUSION_KM_MAX + 3088 + 16 <= 65536 < 16 * (V.FUSION_KM_MAX + 1) + 3088 + 16


# ---------------------------------------------------------------------------------------------------------------- KITTI decode
@pytest.mark.parametrize("shape", V.DECODE_SHAPES, ids=[f"B{b}-K{k}" for b, k in V.DECODE_SHAPES])
def test_decode_planted_rows_and_clearances(shape):
    """from the reference alone: each planted row does what its name says; every other score is clear of the thresholds; the rows
    span the blocks and the classes the device test claims"""
    B, K = shape
    P, calib, ratio, inv, where = V.decode_inputs(B, K)
    assert B * K > 256 and (B * K) % 256 != 0 and set(where) == set(V.PLANTED)
    flat = sorted(b * K + k for b, k in where.values())
    assert {0, 255, 256, B * K - 1} <= set(flat)
    assert set(P[..., 36].long().reshape(-1).tolist()) == {0, 1, 2}
    if B > 1:
        assert len({tuple(r.tolist()) for r in calib}) == B and len({tuple(r.tolist()) for r in ratio}) == B
    rows, keep = V.decode_reference(B, K, True, False, V.DECODE_THRESHOLD)
    alpha = rows[..., 1]

    def first_bin_alpha(b, k, bin_):
        a = F32(bin_) * V.BIN_W + F32(P[b, k, 21 + bin_])
        return float(a - F32(2 * math.pi) if a > V.PI_F else a)

    for name, first in (("tie2-bin0", 0), ("tie3", 3), ("tie-10-11", 10), ("max-11", 11)):
        b, k = where[name]
        lg = P[b, k, 9:21]
        top = (lg == lg.max()).nonzero().flatten().tolist()
        assert top[0] == first and len(top) == {"tie2-bin0": 2, "tie3": 3, "tie-10-11": 2, "max-11": 1}[name]
        assert alpha[b, k].item() == first_bin_alpha(b, k, first)
        for other in top[1:]:   # the last maximum would show
            assert abs(first_bin_alpha(b, k, other) - alpha[b, k].item()) > 0.01
    b, k = where["ang-at-pi"]
    assert alpha[b, k].item() == float(V.PI_F)                                            # not above pi: kept
    b, k = where["ang-below-pi"]
    assert alpha[b, k].item() == float(np.nextafter(V.PI_F, F32(0)))
    b, k = where["ang-above-pi"]
    assert alpha[b, k].item() == float(F32(np.nextafter(V.PI_F, F32(4)) - F32(2 * math.pi))) < -3.14  # wrapped
    for name, sgn in (("ry-plus", 1.0), ("ry-minus", -1.0)):
        b, k = where[name]
        raw = alpha[b, k].item() + math.atan2(float((rows[b, k, 2] + rows[b, k, 4]) / 2 - calib[b, 0]), float(calib[b, 2]))
        assert sgn * raw > math.pi + 0.1 and abs(rows[b, k, 12].item() - (raw - sgn * 2 * math.pi)) < 1e-12
    b, k = where["score-at-thr"]
    assert rows[b, k, 13].item() == 0.5 == V.DECODE_THRESHOLDS[0]
    assert V.DECODE_THRESHOLDS[2] < 0.5 < V.DECODE_THRESHOLDS[1]
    # a product of two float32 factors has at most 48 significant bits: no ROW can score a float64 neighbour of 0.5, so the
    # threshold is moved to the neighbours instead
    assert [bool(V.decode_reference(B, K, True, False, t)[1][b, k]) for t in V.DECODE_THRESHOLDS] == [True, False, True]
    b, k = where["camdis-nan"]
    assert math.isfinite(rows[b, k, 11].item())
    for with_inv in (True, False):
        rc, _ = V.decode_reference(B, K, with_inv, True, V.DECODE_THRESHOLD)
        assert math.isnan(rc[b, k, 11].item()) and int(rc[..., 11].isnan().sum()) == 1 and bool(rc[..., :11].isfinite().all())
    sc = rows[..., 13].clone()
    sc[where["score-at-thr"]] = 0.0
    gap = (sc - V.DECODE_THRESHOLD).abs().min().item()
    assert gap >= V.DECODE_CLEAR * V.DECODE_THRESHOLD, f"a generated score is {gap:.2e} from the threshold"
    assert 0.1 < keep.float().mean().item() < 0.9
    assert torch.equal(V.p2_of(calib)[:, 0, 2].double(), calib[:, 0].float().double())
