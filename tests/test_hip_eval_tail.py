"""The eval head tail (csrc/post.hip) kernel by kernel against the host references of tail_ref.py: y3d_patch_gather,
y3d_head3d_scatter, y3d_head3d_decode, y3d_head2d_decode, y3d_v10_postprocess, and the argument rejections of the C wrappers.

* selection and copy kernels are held to BIT equality; the two decodes to the bounds stated in their tests;
* every output is pre-filled with a sentinel (a NaN with a payload, -7 for integers) and allocated with guard space behind it:
  every element that must be written was written, every guard element still holds the sentinel;
* inputs that take strides are also read from channel slices and row / column crops of wider buffers filled with other values.
tests/test_tail_ref_host.py pins the references and checks from these case lists that they still reach every path."""
import ctypes
import math

import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32, Y3DError

import tail_ref as R

DEV = "cuda"
POST_CAP = 2048 * 256  # post.hip ew_grid: at most 2 048 blocks of 256 threads; larger launches walk the grid-stride loop
TDT = {BF16: torch.bfloat16, F32: torch.float32}
CE = {BF16: 8, F32: 4}
LEVELS = [(12, 20), (6, 10), (3, 5), (2, 3)]  # non-square: a row / column mix-up in the level lookup moves every anchor
STRIDES = [8.0, 16.0, 32.0, 64.0]


def guarded(shape, dtype, guard=256):
    """(whole buffer, view of `shape` at its start): sentinel everywhere, `guard` elements behind the view"""
    n = math.prod(shape)
    buf = R.sentinel(n + guard, dtype, DEV)
    return buf, buf[:n].view(shape)


def check_guard(buf, view, what):
    assert not bool(R.untouched(view).any()), f"{what}: {int(R.untouched(view).sum())} elements were never written"
    assert bool(R.untouched(buf[view.numel():]).all()), f"{what}: a store went past the end of the output"


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    ne = R.bits(got) != R.bits(want)
    if bool(ne.any()):
        i = ne.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ; first at {i}: got {got[tuple(i)]!r}, "
                             f"expected {want[tuple(i)]!r}")


def lds_max_anchors(nc, max_det):
    """the largest A whose score row y3d_v10_postprocess keeps in LDS, by bisection on the library's own (host) rule"""
    L = y3d.lib()
    lo, hi = max_det, 1 << 20  # lo fits, hi does not
    assert L.v10_postprocess_scratch_floats(1, lo, nc, max_det) == 0 and L.v10_postprocess_scratch_floats(1, hi, nc, max_det) != 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if L.v10_postprocess_scratch_floats(1, mid, nc, max_det) == 0:
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------------------------------------------- patch_gather
# (dtype, B, H, W, C, ps, input variant, K)
PG_CASES = [
    (BF16, 2, 3, 3, 8, 5, "dense", 10),      # the patch sticks out of the map on all four sides
    (F32, 2, 3, 3, 4, 7, "slice", 10),
    (BF16, 2, 3, 3, 72, 7, "crop", 10),
    (BF16, 2, 7, 11, 64, 1, "slice", 10),
    (F32, 2, 7, 11, 72, 3, "crop", 10),
    (BF16, 3, 7, 11, 72, 5, "dense", 10),
    (F32, 2, 7, 11, 64, 7, "dense", 10),
    (BF16, 2, 7, 11, 8, 7, "crop", 10),
    (BF16, 2, 20, 20, 64, 3, "crop", 10),
    (F32, 2, 20, 20, 4, 5, "slice", 10),
    (BF16, 2, 20, 20, 72, 5, "slice", 10),
    (F32, 2, 20, 20, 64, 5, "crop", 10),
    (BF16, 8, 20, 20, 512, 5, "dense", 100),  # 1 280 000 chunks: past the 2 048-block cap
]


def _ids(cases):
    return ["-".join(("bf16" if v == BF16 else "f32") if i == 0 else str(v) for i, v in enumerate(c)) for c in cases]


def pg_chunks(case):
    dt, B, H, W, C, ps, var, K = case
    return B * K * ps * ps * (C // CE[dt])


def special_cells(H, W):
    """the four corners, one cell on each edge, the centre, and one of them again"""
    rc = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H // 2, W - 1), (H - 1, W // 2), (H // 2, W // 2), (0, W - 1)]
    return [r * W + c for r, c in rc]


def strided_input(x, var, ce, gen):
    """device copy of the host NHWC tensor `x` as a dense tensor, a channel slice of a wider buffer (xsw > C), or a row / column
    crop of a larger and wider one (xsh != W * xsw, xsb != H * xsh); the surroundings hold other finite values"""
    B, H, W, C = x.shape
    if var == "dense":
        return x.to(DEV).contiguous()
    r0, c0, dh, dw = (0, 0, 0, 0) if var == "slice" else (1, 2, 2, 3)
    buf = (torch.randn(B, H + dh, W + dw, C + 2 * ce, generator=gen) * 5).to(x.dtype)
    buf[:, r0:r0 + H, c0:c0 + W, ce:ce + C] = x
    return buf.to(DEV)[:, r0:r0 + H, c0:c0 + W, ce:ce + C]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PG_CASES, ids=_ids(PG_CASES))
def test_patch_gather_bit_equal(case):
    """zero-padded ps x ps patches around corner, edge, centre and duplicated cells, from dense, channel-sliced and cropped inputs"""
    dt, B, H, W, C, ps, var, K = case
    gen = torch.Generator().manual_seed(H * W + C + ps)
    x = (torch.randn(B, H, W, C, generator=gen) * 3).to(TDT[dt])
    cells = special_cells(H, W)
    idx = torch.stack([torch.tensor((cells[b:] + cells[:b]) + torch.randint(0, H * W, (K - 10,), generator=gen).tolist()) for b in range(B)]).int()
    xd = strided_input(x, var, CE[dt], gen)
    assert (var == "dense") == (xd.stride(2) == C) and (var != "crop" or (xd.stride(1) != W * xd.stride(2) and xd.stride(0) != H * xd.stride(1)))
    buf, out = guarded((B * K, ps, ps, C), TDT[dt])
    y3d.lib().patch_gather(dt, xd.data_ptr(), xd.stride(0), xd.stride(1), xd.stride(2), idx.to(DEV).data_ptr(), out.data_ptr(), B, H, W, C, K, ps,
                           ops.stream())
    torch.cuda.synchronize()
    check_guard(buf, out, "patch_gather")
    assert_bits(out, R.patch_gather(x, idx, ps), f"patch_gather {case}")


# ---------------------------------------------------------------------------------------------------------------- head3d_scatter
# (dtype, B, HW, nc, K): cls is a slice of a wider buffer (csw = nc + 5), reg rows have a stride of 40 > 35
SC_CASES = [
    (BF16, 2, 400, 3, 50),
    (F32, 2, 400, 10, 1),
    (BF16, 3, 64, 1, 64),       # K = HW: every cell carries a candidate
    (F32, 2, 400, 1, 50),
    (BF16, 2, 400, 10, 50),
    (BF16, 2, 262401, 1, 50),   # B * HW = 524 802 cells: past the 2 048-block cap, no = 36
]
SC_CSW_EXTRA, SC_RSW = 5, 40


@pytest.mark.gpu
@pytest.mark.parametrize("case", SC_CASES, ids=_ids(SC_CASES))
def test_head3d_scatter_bit_equal(case):
    """dense cls + the candidates' regression rows on their cells, exactly +0 on every other cell"""
    dt, B, HW, nc, K = case
    no = nc + 35
    gen = torch.Generator().manual_seed(HW + nc + K)
    clsb = (torch.randn(B, HW, nc + SC_CSW_EXTRA, generator=gen) * 3).to(TDT[dt])
    regb = (torch.randn(B * K, SC_RSW, generator=gen) * 3).to(TDT[dt])
    regb[regb == 0] = 1  # a candidate's row never looks like an empty cell
    idx = torch.stack([torch.randperm(HW, generator=gen)[:K] for _ in range(B)]).int()
    cd, rd = clsb.to(DEV), regb.to(DEV)
    cv, rv = cd[..., 2:2 + nc], rd[:, 3:3 + 35]
    buf, out = guarded((B, HW, no), TDT[dt])
    y3d.lib().head3d_scatter(dt, cv.data_ptr(), cv.stride(1), rv.data_ptr(), rv.stride(0), idx.to(DEV).data_ptr(), out.data_ptr(), B, HW, nc, no, K,
                             ops.stream())
    torch.cuda.synchronize()
    check_guard(buf, out, "head3d_scatter")
    assert_bits(out, R.head3d_scatter(clsb[..., 2:2 + nc], regb[:, 3:3 + 35], idx, nc, no), f"head3d_scatter {case}")


# ---------------------------------------------------------------------------------------------------------------- decodes
# (dtype, levels, nc, B) on the first `levels` of LEVELS
D3_CASES = [(BF16, 1, 3, 2), (F32, 2, 1, 2), (BF16, 3, 3, 3), (F32, 4, 3, 2), (BF16, 4, 1, 2), (F32, 3, 1, 2), (BF16, 2, 3, 2), (F32, 1, 3, 2)]
D2_CASES = [(BF16, 1, 80, 2), (F32, 2, 1, 2), (BF16, 3, 2, 2), (F32, 4, 80, 2), (BF16, 4, 1, 3), (F32, 3, 2, 2), (BF16, 2, 80, 2), (F32, 1, 1, 2)]


def level_maps(dt, nl, no, B, gen, scale):
    return [(torch.randn(B, H, W, no, generator=gen) * scale).to(TDT[dt]) for H, W in LEVELS[:nl]]


def launch_decode(fn, dt, maps, nc, C):
    nl, B = len(maps), maps[0].shape[0]
    md = [m.to(DEV).contiguous() for m in maps]
    A = sum(m.shape[1] * m.shape[2] for m in maps)
    buf, out = guarded((B, C, A), torch.float32)
    fn(dt, nl, (ctypes.c_void_p * nl)(*[m.data_ptr() for m in md]), (ctypes.c_int * nl)(*[m.shape[1] for m in maps]),
       (ctypes.c_int * nl)(*[m.shape[2] for m in maps]), (ctypes.c_float * nl)(*STRIDES[:nl]), B, nc, out.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    check_guard(buf, out, "decode")
    return out.cpu()


def nchw(maps):
    return [m.float().permute(0, 3, 1, 2).contiguous() for m in maps]


@pytest.mark.gpu
@pytest.mark.parametrize("case", D3_CASES, ids=_ids(D3_CASES))
def test_head3d_decode_passthrough_exact_and_boxes_bounded(case):
    """cls, size-3d, heading, depth and depth-uncertainty are the stored values converted to fp32, bit for bit, at every anchor
    (the first and last anchor of every level included); the six computed channels against float64.

    Bound, from the fp32 roundings of the kernel's expression chain (every operation is one correctly rounded fp32 operation,
    eps = 2^-24, the library is built with -ffp-contract=off; the stored values convert to fp32 exactly):
      c = fl(fl(o + anchor) * stride)      two roundings                     |c_fl - c| <= (2 eps + eps^2) |c|
      h = fl(size * stride) / 2            one rounding, the halving exact   |h_fl - h| <= eps |h|
      corner = fl(c_fl -+ h_fl)            one rounding                      <= eps |corner_fl|
    so |corner_fl - corner| <= eps (2 |c| + |h| + |corner|) (1 + 2^-20) and |centre3d_fl - centre3d| <= 2 eps |centre3d| (1 + 2^-20);
    + 1e-30 as in test_hip_eval_epilogues.bound.  (With the power-of-two strides used here the products are exact as well; the
    bound does not rely on it.)

    Also asserted: the whole output is bit-equal to oracle.restate.head3d_decode run in float32 on the CPU - the same operations
    in the same order without contraction; it held on the MI355X for every case of this list (the fp32 cases reach 0.59 - 0.61 of
    the bound; bf16 maps, 8 significant bits, decode without any rounding)."""
    from oracle import restate as RS
    dt, nl, nc, B = case
    no = nc + 35
    gen = torch.Generator().manual_seed(nl * 10 + nc)
    maps = level_maps(dt, nl, no, B, gen, 3.0)
    out = launch_decode(y3d.lib().head3d_decode, dt, maps, nc, no)
    ref, mag = R.head3d_decode(maps, STRIDES[:nl], nc)
    passthrough = list(range(nc)) + list(range(nc + 6, no))
    assert_bits(out[:, passthrough], ref[:, passthrough].float(), f"head3d_decode pass-through {case}")
    err = (out[:, nc:nc + 6].double() - ref[:, nc:nc + 6]).abs()
    tol = 2.0 ** -24 * mag * (1 + 2.0 ** -20) + 1e-30
    print(f"head3d_decode {case}: max err / bound = {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), f"{case}: {int((err > tol).sum())} box / centre values outside the bound, worst ratio {float((err / tol).max()):.3f}"
    assert_bits(out, RS.head3d_decode(nchw(maps), STRIDES[:nl], nc), f"head3d_decode vs the float32 restatement {case}")


def saturated_maps(dt, nl, nc, B, gen):
    """DFL rows with one bin at +80 and the rest at -80 (expectation = that bin) or of equal bins (expectation 7.5); class logits at
    +-90 (sigmoid exactly 1 / 0).  Returns the maps, the expected distances (B, A, 4) and the expected scores (B, A, nc)"""
    maps, dist, score = [], [], []
    for H, W in LEVELS[:nl]:
        hot = torch.randint(0, 16, (B, H, W, 4), generator=gen)
        flat = torch.rand(B, H, W, 4, generator=gen) < 0.25
        bins = torch.full((B, H, W, 4, 16), -80.0)
        bins.scatter_(-1, hot.unsqueeze(-1), 80.0)
        bins[flat] = 3.0
        pos = torch.rand(B, H, W, nc, generator=gen) < 0.5
        maps.append(torch.cat((bins.reshape(B, H, W, 64), torch.where(pos, 90.0, -90.0)), -1).to(TDT[dt]))
        dist.append(torch.where(flat, 7.5, hot.double()).reshape(B, H * W, 4))
        score.append(pos.double().reshape(B, H * W, nc))
    return maps, torch.cat(dist, 1), torch.cat(score, 1)


def head2d_bounds(maps, strides, nc):
    """(box bound, score bound): 4 x the largest distance of the float32 CPU restatement from the float64 reference on these inputs"""
    from oracle import restate as RS
    ref = R.head2d_decode(maps, strides, nc)
    r32 = RS.head2d_decode(nchw(maps), strides, nc).double()
    return ref, 4 * float((r32[:, :4] - ref[:, :4]).abs().max()), 4 * float((r32[:, 4:] - ref[:, 4:]).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", D2_CASES, ids=_ids(D2_CASES))
def test_head2d_decode_bounded_and_saturated_exact(case):
    """DFL expectation + dist2bbox + sigmoid against float64 on `randn * 4` logits, and exactly on saturated logits.

    The tolerance depends on the device expf, so it is measured against the reference, not derived: per case and separately
    for the four box channels (pixels) and the score channels, the largest distance of the float32 CPU restatement
    (oracle.restate.head2d_decode) from the float64 reference on the same inputs, times 4 (a different but equally accurate
    expf, another summation order over the 16 bins).  The distance is computed when the test runs (it depends a little on the
    host's vector math library).  Measured over this list: CPU distances of 3.5e-5 (one level, stride 8) to 2.7e-4 px (four levels,
    stride 64) for the boxes and 7.5e-8 to 8.8e-8 for the scores, so the kernel is allowed 1.4e-4 to 1.1e-3 px and 3.0e-7 to
    3.5e-7 (test_tail_ref_host.py prints the distances per case); the kernel on an MI355X was 3.8e-5 to 2.1e-4 px and 7.5e-8 to
    8.8e-8 from the reference, at most 0.36 of its bound for the boxes and 0.25 for the scores.
    Saturated family: one-hot DFL rows (+80 / -80) give the bin index, equal bins give 7.5, class logits of +-90 give exactly
    1 / 0 - the output equals the exactly computed boxes and scores, nothing non-finite."""
    dt, nl, nc, B = case
    gen = torch.Generator().manual_seed(nl * 100 + nc)
    maps = level_maps(dt, nl, 64 + nc, B, gen, 4.0)
    out = launch_decode(y3d.lib().head2d_decode, dt, maps, nc, 4 + nc)
    ref, tb, ts = head2d_bounds(maps, STRIDES[:nl], nc)
    eb, es = float((out[:, :4].double() - ref[:, :4]).abs().max()), float((out[:, 4:].double() - ref[:, 4:]).abs().max())
    print(f"head2d_decode {case}: boxes {eb:.3e} (bound {tb:.3e}), scores {es:.3e} (bound {ts:.3e})")
    assert eb <= tb and es <= ts, f"{case}: boxes {eb:.3e} > {tb:.3e} or scores {es:.3e} > {ts:.3e}"
    # saturated logits: exact
    maps, d, s = saturated_maps(dt, nl, nc, B, gen)
    out = launch_decode(y3d.lib().head2d_decode, dt, maps, nc, 4 + nc)
    assert bool(torch.isfinite(out).all())
    lv, hy, hx = R.anchors(LEVELS[:nl])
    st = torch.tensor([STRIDES[l] for l in lv], dtype=torch.float64)
    ax, ay = torch.from_numpy(hx + 0.5), torch.from_numpy(hy + 0.5)
    x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
    want = torch.cat((torch.stack(((x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st), 1), s.permute(0, 2, 1)), 1)
    assert_bits(out, want.float(), f"head2d_decode saturated {case}")


# ---------------------------------------------------------------------------------------------------------------- v10_postprocess
def pp_cases():
    """(A, nc, max_det, boxes_first, B, score family)"""
    a80, a3 = lds_max_anchors(80, 300), lds_max_anchors(3, 50)
    return [
        (64, 3, 64, 0, 2, "grid"),            # max_det == A
        (64, 1, 64, 1, 3, "const"),
        (64, 80, 64, 1, 2, "pair"),
        (2100, 3, 50, 0, 3, "grid"),
        (2100, 80, 300, 1, 2, "pair"),
        (2100, 1, 1, 0, 2, "const"),
        (2100, 3, 1, 1, 2, "grid"),
        (8400, 80, 300, 1, 2, "grid"),
        (8400, 3, 50, 0, 2, "pair"),
        (8400, 1, 300, 1, 2, "grid"),
        (8400, 3, 300, 0, 3, "const"),
        (a80, 80, 300, 1, 2, "grid"),         # the largest A on the LDS path ...
        (a80 + 1, 80, 300, 1, 2, "grid"),     # ... and the first on the segmented one (16 segments, a short last one)
        (a80 + 1, 80, 300, 0, 2, "pair"),
        (a3, 3, 50, 0, 2, "grid"),
        (a3 + 1, 3, 50, 0, 2, "grid"),
        (a3 + 1, 3, 50, 1, 2, "const"),
        (a3 + 1, 3, 50, 0, 3, "pair"),
        (30000, 1, 2000, 1, 2, "grid"),       # 16 * max_det * 2 > A: the wrapper falls back to 4 segments
        (30001, 1, 2000, 0, 2, "const"),
    ]


PP_CASES = pp_cases()


def pp_path(case):
    """'lds' or the segment count of the hi-res path, from the library's host rule"""
    A, nc, K, bf, B, fam = case
    if y3d.lib().v10_postprocess_scratch_floats(B, A, nc, K) == 0:
        return "lds"
    return R.postprocess_nseg(A, K)


def pp_scores(A, nc, B, fam, gen):
    """(B, nc, A) scores built to tie: a grid of 1/8 (hundreds of equal values inside and across segments and at the K-th value),
    a constant map, or the grid with one anchor's classes tied and neighbouring anchors equal"""
    if fam == "const":
        return torch.full((B, nc, A), 0.375)
    s = torch.round(torch.rand(B, 1, A, generator=gen) * torch.rand(B, nc, A, generator=gen) * 8) / 8
    if fam == "pair":
        if nc > 1:
            s[:, 1, ::2] = s[:, 0, ::2]          # two classes of one anchor tie
        n = s[:, :, 1::4].shape[2]
        s[:, :, 1::4] = s[:, :, 0::4][:, :, :n].clone()  # whole anchors repeat: ties between anchors in the second stage
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("case", PP_CASES, ids=[f"A{c[0]}-nc{c[1]}-k{c[2]}-bf{c[3]}-B{c[4]}-{c[5]}" for c in PP_CASES])
def test_v10_postprocess_ties_exact_on_both_paths(case):
    """reg, scores and labels equal two stable sorts by (value desc, flat index asc) exactly, on tied scores, on the LDS path and on
    the segmented path (16 and fewer segments, a short last segment), through the C ABI and through loss.v10postprocess /
    v10_3Dpostprocess"""
    from yolov10_3d_amd.loss import v10_3Dpostprocess, v10postprocess
    A, nc, K, bf, B, fam = case
    L = y3d.lib()
    gen = torch.Generator().manual_seed(A + nc + K)
    nr = 4 if bf else 35
    C = nc + nr
    sc = pp_scores(A, nc, B, fam, gen)
    rg = torch.randn(B, nr, A, generator=gen) * 100
    y = torch.cat((rg, sc), 1) if bf else torch.cat((sc, rg), 1)
    path = pp_path(case)
    if path != "lds" and path < 16:
        assert 16 * K * 2 > A, "premise: the wrapper's rule `16 * max_det * 2 > A` is what leaves fewer than 16 segments"
    want = R.v10_postprocess(y, nc, K, bf)
    yd = y.to(DEV).contiguous()
    rb, reg = guarded((B, K, nr), torch.float32)
    sb, scores = guarded((B, K), torch.float32)
    lb, labels = guarded((B, K), torch.int64)
    ns = L.v10_postprocess_scratch_floats(B, A, nc, K)
    assert (ns == 0) == (path == "lds")
    scb, scratch = guarded((max(ns, 1),), torch.float32)
    L.v10_postprocess(yd.data_ptr(), B, C, A, nc, K, bf, reg.data_ptr(), scores.data_ptr(), labels.data_ptr(), scratch.data_ptr() if ns else None,
                      ops.stream())
    torch.cuda.synchronize()
    for b_, v_, w_ in ((rb, reg, "reg"), (sb, scores, "scores"), (lb, labels, "labels")):
        check_guard(b_, v_, f"v10_postprocess {w_}")
    assert bool(R.untouched(scb[max(ns, 1):]).all()), "a store went past the end of the scratch"
    assert torch.equal(labels.cpu(), want[2]), f"{case} ({path}): labels differ in rows {(labels.cpu() != want[2]).any(1).nonzero().flatten().tolist()}"
    assert_bits(scores, want[1], f"v10_postprocess scores {case} ({path})")
    assert_bits(reg, want[0], f"v10_postprocess reg {case} ({path})")
    got = (v10postprocess if bf else v10_3Dpostprocess)(yd.permute(0, 2, 1), K, nc)
    for g, w, what in zip(got, want, ("reg", "scores", "labels")):
        assert_bits(g, w, f"loss wrapper {what} {case} ({path})")


# ---------------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.gpu
def test_wrappers_reject_bad_arguments_without_writing():
    """the C wrappers return the library's error before any launch: the outputs still hold the sentinel"""
    L, st = y3d.lib(), ops.stream()
    x16 = torch.zeros(4096, dtype=torch.bfloat16, device=DEV)
    x32 = torch.zeros(4096, dtype=torch.float32, device=DEV)
    ib, idx = guarded((2, 50), torch.int32)
    with pytest.raises(Y3DError, match="topk_cells"):
        L.topk_cells(F32, x32.data_ptr(), 3, 2, 40, 3, 50, idx.data_ptr(), st)          # K > H*W
    ob, out = guarded((1024,), torch.bfloat16)
    cells = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(Y3DError, match="patch_gather"):
        L.patch_gather(BF16, x16.data_ptr(), 12 * 16, 12 * 4, 12, cells.data_ptr(), out.data_ptr(), 1, 4, 4, 12, 2, 3, st)  # C % 8 != 0
    with pytest.raises(Y3DError, match="patch_gather"):
        L.patch_gather(BF16, x16.data_ptr(), 20 * 16, 20 * 4, 20, cells.data_ptr(), out.data_ptr(), 1, 4, 4, 16, 2, 3, st)  # xsw % 8 != 0
    A = lds_max_anchors(3, 50) + 1
    rb, reg = guarded((1, 50, 35), torch.float32)
    sb, sc = guarded((1, 50), torch.float32)
    lb, lab = guarded((1, 50), torch.int64)
    yy = torch.zeros(38 * A, dtype=torch.float32, device=DEV)
    with pytest.raises(Y3DError, match="v10_postprocess"):
        L.v10_postprocess(yy.data_ptr(), 1, 38, A, 3, 50, 0, reg.data_ptr(), sc.data_ptr(), lab.data_ptr(), None, st)  # no scratch
    yb, yo = guarded((1024,), torch.bfloat16)
    ab, arg = guarded((1024,), torch.uint8)
    for k in (4, 17):
        with pytest.raises(Y3DError, match="maxpool_fwd"):
            L.maxpool_fwd(BF16, x16.data_ptr(), 128, 32, 8, yo.data_ptr(), 8, arg.data_ptr(), 1, 4, 4, 8, k, st)
    nb, no_ = guarded((1024,), torch.float32)
    with pytest.raises(Y3DError, match="nchw_to_nhwc"):
        L.nchw_to_nhwc(F32, x32.data_ptr(), no_.data_ptr(), 1, 5, 4, 4, 4, st)           # Cpad < C
    torch.cuda.synchronize()
    for b in (ib, ob, rb, sb, lb, yb, ab, nb):
        assert bool(R.untouched(b).all()), "a rejected call wrote to its output"
