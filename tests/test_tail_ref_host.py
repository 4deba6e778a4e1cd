"""CPU: the host references of tail_ref.py against independent statements of the same operations (oracle/restate.py,
torch.nn.functional and its autograd in float64), and the coverage the case lists of test_hip_eval_tail.py / test_hip_glue.py
claim, checked from the lists themselves."""
import pytest
import torch
import torch.nn.functional as F

import yolov10_3d_amd as y3d
from yolov10_3d_amd._lib import BF16, F32
from oracle import restate as RS

import tail_ref as R
import test_hip_eval_tail as T
import test_hip_glue as G


def test_sentinel_and_bits_helpers():
    for dt in (torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64):
        s = R.sentinel((5,), dt)
        assert bool(R.untouched(s).all())
        if dt.is_floating_point:
            assert bool(s.isnan().all())
            assert not bool(R.untouched(torch.full((3,), float("nan"), dtype=dt)).any())  # an ordinary NaN is not the sentinel
        s[2] = 1
        assert R.untouched(s).tolist() == [True, True, False, True, True]
    assert bool((R.bits(torch.tensor([0.0])) != R.bits(torch.tensor([-0.0]))).all())


@pytest.mark.parametrize("case", [c for c in T.PG_CASES if c[7] == 10], ids=T._ids([c for c in T.PG_CASES if c[7] == 10]))
def test_patch_gather_ref_vs_restated_padding(case):
    """oracle.restate.head3d_sparse: the map padded by ps // 2 on every side, patch rows / columns = (row, col) + 0..ps-1"""
    dt, B, H, W, C, ps, var, K = case
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, W, C, generator=gen).to(T.TDT[dt])
    idx = torch.tensor([T.special_cells(H, W)] * B).int()
    pad = ps // 2
    xp = F.pad(x.float().permute(0, 3, 1, 2), (pad, pad, pad, pad))
    rows, cols = (idx.long() // W).reshape(-1), (idx.long() % W).reshape(-1)
    bidx = torch.arange(B).repeat_interleave(K)
    dr = torch.arange(ps)
    patches = xp[bidx[:, None, None], :, (rows[:, None] + dr)[:, :, None], (cols[:, None] + dr)[:, None, :]]  # (B*K, ps, ps, C)
    assert torch.equal(R.patch_gather(x, idx, ps).float(), patches)


@pytest.mark.parametrize("case", T.SC_CASES[:5], ids=T._ids(T.SC_CASES[:5]))
def test_scatter_ref_vs_restated_assignment(case):
    """oracle.restate.head3d_sparse: full = zeros; full[bidx, :, rows, cols] = o; cat((cls, full), 1)"""
    dt, B, HW, nc, K = case
    gen = torch.Generator().manual_seed(2)
    W = 8 if HW == 64 else 20
    H = HW // W
    cls = torch.randn(B, HW, nc, generator=gen)
    reg = torch.randn(B * K, 35, generator=gen)
    idx = torch.stack([torch.randperm(HW, generator=gen)[:K] for _ in range(B)]).int()
    full = torch.zeros(B, 35, H, W)
    bidx = torch.arange(B).repeat_interleave(K)
    full[bidx, :, (idx.long() // W).reshape(-1), (idx.long() % W).reshape(-1)] = reg
    want = torch.cat((cls.view(B, H, W, nc).permute(0, 3, 1, 2), full), 1).permute(0, 2, 3, 1).reshape(B, HW, nc + 35)
    assert torch.equal(R.head3d_scatter(cls, reg, idx, nc, nc + 35), want)


@pytest.mark.parametrize("case", T.D3_CASES, ids=T._ids(T.D3_CASES))
def test_head3d_decode_ref_vs_restate_float64(case):
    dt, nl, nc, B = case
    gen = torch.Generator().manual_seed(3)
    maps = T.level_maps(dt, nl, nc + 35, B, gen, 3.0)
    ref, mag = R.head3d_decode(maps, T.STRIDES[:nl], nc)
    want = RS.head3d_decode([m.double().permute(0, 3, 1, 2).contiguous() for m in maps], T.STRIDES[:nl], nc)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # the float32 restatement itself stays inside the bound the device test derives for the kernel
    r32 = RS.head3d_decode(T.nchw(maps), T.STRIDES[:nl], nc).double()
    assert bool(((r32[:, nc:nc + 6] - ref[:, nc:nc + 6]).abs() <= 2.0 ** -24 * mag * (1 + 2.0 ** -20) + 1e-30).all())
    assert bool((mag >= 0).all())


@pytest.mark.parametrize("case", T.D2_CASES, ids=T._ids(T.D2_CASES))
def test_head2d_decode_ref_vs_restate_float64(case):
    """also prints the distance the device test's bound is 4 x of: float32 restatement vs float64 reference on the test's inputs"""
    dt, nl, nc, B = case
    gen = torch.Generator().manual_seed(nl * 100 + nc)  # the device test's inputs
    maps = T.level_maps(dt, nl, 64 + nc, B, gen, 4.0)
    ref, tb, ts = T.head2d_bounds(maps, T.STRIDES[:nl], nc)
    print(f"head2d_decode {case}: float32 restatement vs float64: boxes {tb / 4:.3e} px, scores {ts / 4:.3e}")
    want = RS.head2d_decode([m.double().permute(0, 3, 1, 2).contiguous() for m in maps], T.STRIDES[:nl], nc)
    assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert 0 < tb < 4e-3 and 0 < ts < 1e-6  # sanity: a few fp32 ulps of a box coordinate below 2 048 px / of a score
    # saturated family: the float64 reference agrees with the exact expectation the device test asserts
    maps, d, s = T.saturated_maps(dt, nl, nc, B, gen)
    ref = R.head2d_decode(maps, T.STRIDES[:nl], nc)
    assert float((ref[:, 4:].permute(0, 2, 1) - s).abs().max()) < 1e-30
    lv, hy, hx = R.anchors(T.LEVELS[:nl])
    st = torch.tensor([T.STRIDES[l] for l in lv], dtype=torch.float64)
    assert float((ref[:, 2] - (d[..., 0] + d[..., 2]) * st).abs().max()) < 1e-30
    assert float((ref[:, 3] - (d[..., 1] + d[..., 3]) * st).abs().max()) < 1e-30


@pytest.mark.parametrize("A,nc,K,bf", [(2100, 3, 50, 0), (2100, 80, 300, 1), (64, 3, 64, 0), (700, 1, 1, 1), (8400, 1, 300, 0)])
def test_postprocess_ref_vs_restate_on_distinct_scores(A, nc, K, bf):
    """on distinct scores the order is unambiguous: the two stable sorts equal the restated torch.topk chain exactly"""
    gen = torch.Generator().manual_seed(A + nc)
    B, nr = 2, 4 if bf else 35
    n = B * A * nc
    sc = (torch.randperm(n, generator=gen).float() / n).view(B, A, nc)
    rg = torch.randn(B, A, nr, generator=gen)
    preds = torch.cat((rg, sc), -1) if bf else torch.cat((sc, rg), -1)
    want = (RS.postprocess2d if bf else RS.postprocess3d)(preds, K, nc)
    got = R.v10_postprocess(preds.permute(0, 2, 1).contiguous(), nc, K, bf)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2].long())


def test_postprocess_ref_tie_rule():
    """(value desc, index asc) in both stages, -0 equal to +0"""
    y = torch.tensor([[[0.5, 0.5, 0.25, 0.5], [0.5, 0.25, 0.5, -0.0], [1.0, 2.0, 3.0, 4.0]]])  # nc = 2, one reg row, A = 4
    reg, sc, lab = R.v10_postprocess(y, 2, 3, 0)
    # stage 1: best = .5 .5 .5 .5 -> anchors 0, 1, 2; stage 2 flat = [.5 .5 | .5 .25 | .25 .5] -> 0, 1, 2
    assert sc.tolist() == [[0.5, 0.5, 0.5]] and lab.tolist() == [[0, 1, 0]] and reg[0, :, 0].tolist() == [1.0, 1.0, 2.0]
    assert R._top_desc([0.0, -0.0, 0.0], 3).tolist() == [0, 1, 2]
    assert R.postprocess_nseg(15165, 300) == 16 and R.postprocess_nseg(30000, 2000) == 4 and R.postprocess_nseg(100, 300) == 1


@pytest.mark.parametrize("case", G.MP_CASES, ids=T._ids(G.MP_CASES))
def test_maxpool_ref_vs_aten_float64(case):
    """F.max_pool2d(k, 1, k // 2, return_indices=True) in float64 on the tied / -inf / NaN inputs of the device test: values, the
    arg-max (first maximum, last NaN, first in-map element of a window of -inf only) and the autograd of integer gradients"""
    dt, B, H, W, C, k, val, lay = case
    x, dy, _ = G.mp_input(case)
    pad = k // 2
    xa = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ya, ia = F.max_pool2d(xa, k, 1, pad, return_indices=True)
    ya.backward(dy.double().permute(0, 3, 1, 2))
    y, arg = R.maxpool_fwd(x, k)
    nan = ya.isnan()
    assert torch.equal(y.double().permute(0, 3, 1, 2).isnan(), nan)
    assert torch.equal(torch.where(nan, 0.0, y.double().permute(0, 3, 1, 2)), torch.where(nan, 0.0, ya.detach()))
    a = arg.long()
    h, w = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1)
    flat = (h - pad + a // k) * W + (w - pad + a % k)
    assert torch.equal(flat.permute(0, 3, 1, 2), ia)
    assert torch.equal(R.maxpool_bwd(dy.double(), arg, k).permute(0, 3, 1, 2), xa.grad)
    if val == "neginf":  # the case the issue asks about: windows of -inf only exist, on the border too
        assert bool((y[:, 0, 0, 0] == float("-inf")).all())


@pytest.mark.parametrize("case", G.UP_CASES, ids=T._ids(G.UP_CASES))
def test_upsample_ref_vs_interpolate_float64(case):
    dt, B, H, W, C, lay = case
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, C, generator=gen).double()
    dy = torch.randint(-200, 201, (B, 2 * H, 2 * W, C), generator=gen).double()
    xa = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ya = F.interpolate(xa, scale_factor=2, mode="nearest")
    ya.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(R.upsample2x_fwd(x).permute(0, 3, 1, 2), ya.detach())
    assert torch.equal(R.upsample2x_bwd(dy).permute(0, 3, 1, 2), xa.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_copy_add_expectations_vs_cat_and_plus(dtype):
    """what the copy2d / add2d tests expect, stated with torch.cat and `+`: a copied slice is the member of the concat; a sum of two
    stored values on the k / 64 grid is exact in fp32, so torch's fp32 `+` followed by ONE conversion is the same number"""
    gen = torch.Generator().manual_seed(6)
    a = (torch.randint(-512, 513, (77, 24), generator=gen).double() / 64).to(dtype)
    b = (torch.randint(-512, 513, (77, 24), generator=gen).double() / 64).to(dtype)
    cat = torch.cat((a, b), 1)
    assert torch.equal(R.bits(cat[:, 24:]), R.bits(b))
    s32 = a.float() + b.float()
    assert torch.equal(s32.double(), a.double() + b.double())
    assert torch.equal(R.bits(R.rnd(a.double() + b.double(), dtype).to(dtype)), R.bits(s32.to(dtype)))


@pytest.mark.parametrize("case", G.NH_CASES, ids=T._ids(G.NH_CASES))
def test_layout_refs_vs_permute(case):
    dt, B, C, H, W, Cpad, lay = case
    gen = torch.Generator().manual_seed(7)
    x = G.special_f32(B * C * H * W, gen).view(B, C, H, W)
    y = R.nchw_to_nhwc(x, Cpad, T.TDT[dt])
    want = F.pad(x.to(T.TDT[dt]).permute(0, 2, 3, 1), (0, Cpad - C))
    assert torch.equal(R.bits(y), R.bits(want))
    assert torch.equal(R.bits(R.nhwc_to_nchw(y[..., :C])), R.bits(x.to(T.TDT[dt]).float()))
    assert bool(x.isinf().any()) and bool((R.bits(x) == R.bits(torch.tensor([-0.0]))).any())


def test_case_lists_reach_every_path():
    """from the case lists themselves: both dtypes everywhere; both postprocess paths, the segmented one with 16 and with fewer
    segments (decided by the library's host rule y3d_v10_postprocess_scratch_floats), the LDS boundary on both sides, a short
    last segment, max_det == A, nc == 1; a strided input and a strided output for every kernel that takes strides; a case past
    each grid cap (2 048 blocks of 256 in post.hip, 4 096 in misc.hip)"""
    L = y3d.lib()
    for name, cases in (("patch_gather", T.PG_CASES), ("head3d_scatter", T.SC_CASES), ("head3d_decode", T.D3_CASES), ("head2d_decode", T.D2_CASES),
                        ("maxpool", G.MP_CASES), ("upsample2x", G.UP_CASES), ("copy2d / add2d", G.CP_CASES), ("layout", G.NH_CASES)):
        assert {c[0] for c in cases} == {BF16, F32}, f"{name}: a dtype is missing"
    # patch_gather: every ps and C of the issue, all three input layouts in both dtypes, the oversized patch, the cap
    assert {c[5] for c in T.PG_CASES} == {1, 3, 5, 7}
    assert {(c[0], c[6]) for c in T.PG_CASES} == {(dt, v) for dt in (BF16, F32) for v in ("dense", "slice", "crop")}
    assert {c[4] // T.CE[c[0]] for c in T.PG_CASES} >= {1} and {c[4] for c in T.PG_CASES} >= {64, 72}
    assert {c[5] for c in T.PG_CASES if (c[2], c[3]) == (3, 3)} == {5, 7}
    assert {(c[2], c[3]) for c in T.PG_CASES} == {(3, 3), (7, 11), (20, 20)}
    assert max(T.pg_chunks(c) for c in T.PG_CASES) > T.POST_CAP
    # head3d_scatter: strided cls and reg, every nc, the three K regimes, the cap
    assert T.SC_CSW_EXTRA > 0 and T.SC_RSW > 35
    assert {c[3] for c in T.SC_CASES} == {1, 3, 10}
    assert any(c[4] == 1 for c in T.SC_CASES) and any(c[4] == c[2] for c in T.SC_CASES) and any(c[2:5:2] == (400, 50) for c in T.SC_CASES)
    assert any(c[1] * c[2] > T.POST_CAP and c[3] == 1 for c in T.SC_CASES)
    # decodes: 1..4 levels in both dtypes, non-square levels, the class counts
    for cases, ncs in ((T.D3_CASES, {1, 3}), (T.D2_CASES, {1, 2, 80})):
        assert {c[1] for c in cases if c[0] == BF16} == {1, 2, 3, 4} == {c[1] for c in cases if c[0] == F32}
        assert {c[2] for c in cases} == ncs
    assert all(H != W for H, W in T.LEVELS) and len(T.LEVELS) == 4
    # v10_postprocess
    paths = {T.pp_path(c) for c in T.PP_CASES}
    assert "lds" in paths and 16 in paths and any(p != "lds" and p < 16 for p in paths), paths
    assert {c[3] for c in T.PP_CASES} == {0, 1} and {c[1] for c in T.PP_CASES} == {1, 3, 80} and {c[4] for c in T.PP_CASES} == {2, 3}
    assert {c[2] for c in T.PP_CASES} >= {1, 50, 300} and any(c[2] == c[0] for c in T.PP_CASES)
    assert {c[0] for c in T.PP_CASES} >= {64, 2100, 8400}
    assert {c[5] for c in T.PP_CASES} == {"grid", "const", "pair"}
    for nc, K in ((80, 300), (3, 50)):
        a = T.lds_max_anchors(nc, K)
        assert L.v10_postprocess_scratch_floats(2, a, nc, K) == 0 and L.v10_postprocess_scratch_floats(2, a + 1, nc, K) == 2 * (a + 1)
        for fam_path in (("lds", a), (16, a + 1)):
            assert any(c[:3] == (fam_path[1], nc, K) and T.pp_path(c) == fam_path[0] for c in T.PP_CASES), f"boundary case {fam_path} of nc={nc} K={K}"
    seg = [c for c in T.PP_CASES if T.pp_path(c) != "lds"]
    assert any(c[0] % T.pp_path(c) for c in seg), "no A that is not a multiple of the segment count"
    assert {c[5] for c in seg} == {"grid", "const", "pair"} and {c[3] for c in seg} == {0, 1}
    for c in seg:
        if T.pp_path(c) < 16:
            assert 16 * c[2] * 2 > c[0]
    # glue: both layouts per kernel family (strided = distinct strides on inputs AND outputs), every k / map / C, the cap
    for name, cases in (("maxpool", G.MP_CASES), ("upsample2x", G.UP_CASES), ("copy2d / add2d", G.CP_CASES), ("nhwc_to_nchw", G.NH_CASES)):
        assert {c[-1] for c in cases} == {"dense", "strided"}, f"{name}: a layout is missing"
        assert {c[0] for c in cases if c[-1] == "strided"} == {BF16, F32}, f"{name}: strided in one dtype only"
    assert {c[5] for c in G.MP_CASES} == {3, 5, 9, 15} and {(c[2], c[3]) for c in G.MP_CASES} == {(1, 1), (2, 7), (13, 17), (20, 20)}
    assert {c[6] for c in G.MP_CASES} == {"grid", "neginf", "nan"}
    for cases, ci in ((G.MP_CASES, 4), (G.UP_CASES, 4)):
        assert {c[ci] for c in cases} >= {16, 72} and any(c[ci] == T.CE[c[0]] for c in cases)
    assert {(c[2], c[3]) for c in G.UP_CASES} == {(1, 1), (3, 5), (20, 20)}
    assert {c[2] for c in G.CP_CASES} >= {24, 520} and any(c[2] == T.CE[c[0]] for c in G.CP_CASES)
    assert {c[1] for c in G.CP_CASES} >= {1, 77} and max(G.cp_chunks(c) for c in G.CP_CASES) > G.MISC_CAP
    assert {c[2] for c in G.NH_CASES} == {1, 3, 5} and {c[5] for c in G.NH_CASES} >= {8, 16} and any(c[5] == c[2] for c in G.NH_CASES)
    assert all(c[3] % 2 and c[4] % 2 for c in G.NH_CASES)
