"""The training conv entry points against exact references: y3d_conv2d_fwd with BatchNorm partials, y3d_conv2d_bwd_data and
y3d_conv2d_bwd_weight on every kernel that serves them, and at every geometry one S-3D training step launches.

* bf16 mode, bit-exact WITH rounding: x, w and dy are integers (amplitude chosen per case from the contraction length so that most
  accumulators exceed 256 in magnitude).  Every product and partial sum is then an exact fp32 integer in any summation order, as each
  case asserts (sum |a||b| < 2^24).  y and dx must equal round-to-nearest-even of the exact integer (fp32 -> bf16), value for value
  (a zero may carry either sign); at least 25 % of the outputs exceed 256 and some are exact bf16 ties, so a store that truncates,
  rounds ties away from zero or rounds twice fails.  dW (fp32) must equal the exact integer whatever nsplit is.
* BatchNorm partials: folded over their rows in fp64 they must give the statistics of the STORED y.  Sum y is exact (integers, each
  row's sum |y| < 2^24, asserted).  Sum y^2 is a sum of exact squares in fp32 (a bf16 value has 8 significant bits): a row that covers
  n pixels is within (n - 1) 2^-24 of its true value, in any order, so |sum_rows - ref| <= (n_max - 1) 2^-24 (1 + 2^-10) sum y^2 + the
  fp64 fold.  n_max, the most pixels one partial row covers, per route:
      GENERIC            128 (one row per 128-pixel tile)
      TILE8 / WIDE3_8    128 (8 x 16 tile);  TILE16 / WIDE3_16  256 (16 x 16 tile)
      FLAT               512 positions of the flat padded space
      SMALL / SMALL_S2   ceil(tiles / rows) x 128: a persistent worker per row, 8 x 16 output tiles dealt round-robin
      STREAM1X1          ceil(ceil(M / 128) / rows) x 128: a worker per row, 128-pixel tiles dealt round-robin
  Each case also shows a gap between the statistics of the stored y and those of the fp32 accumulators larger than that bound, so
  summing the accumulator instead of the stored value fails.
* fp32 mode, exact with operands bf16 cannot hold: one operand of each product is a * 2^-6 with a an integer of 12 significant bits
  (bf16 keeps 8, xf32 11), the other a small integer, sum |.||.| < 2^18: every partial sum is a multiple of 2^-6 within 24 bits.  y,
  dx and dW must equal the exact result; which operand is the wide one alternates over the cases.
* placement and poison: x and dy are channel slots of wider buffers whose other channels (and, cropped, the pixels around the map)
  hold 2^100; outputs, partial rows, slabs and dW are NaN-filled, and everything outside the output slot must still be NaN.
The references are fp64 on the device (patch . weight dot products; per-tap pixel contractions for dW)."""
import math

import pytest
import torch

from test_hip_eval_epilogues import ROUTE_NAME, ROUTES, _exact_acc, _sample_pixels

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402
from yolov10_3d_amd._lib import BF16, F32, Y3DError  # noqa: E402

DEV = "cuda"
FWD, DGRAD, WGRAD = 0, 1, 2
OPNAME = {FWD: "fwd", DGRAD: "dgrad", WGRAD: "wgrad"}
EPI_PARTIALS = 1
OFF, EXTRA = 8, 24  # operand / output slot: channels [OFF, OFF + C) of a buffer with C + EXTRA channels
SENT = 2.0 ** 100  # sentinel around the operand slots: finite, exact in bf16, and ruinous in any product it enters
DENSE_ONLY = {(FWD, "STREAM1X1"), (DGRAD, "STREAM1X1"), (DGRAD, "S2_DGRAD"), (WGRAD, "WGRAD_STREAM1X1")}


def _cdiv(a, b):
    return -(-a // b)


def _out_hw(case):
    _, _, H, W, _, _, _, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _route(op, case):
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    return y3d.lib().conv2d_route(dt, op, EPI_PARTIALS if op == FWD else 0, B, H, W, Cin, Cout, g, k, k, s, p)


def _rname(op, case):
    return ROUTE_NAME.get(_route(op, case), "?")


# (dtype, B, H, W, Cin, Cout, groups, k, stride, pad), the route y3d_conv2d_route gives it today, extras (wgrad: nsplit, cin_real,
# accumulate).  Checked by test_train_case_routes.
FWD_CASES = [
    ((BF16, 3, 20, 24, 128, 80, 1, 1, 1, 0), "STREAM1X1", {}),
    ((BF16, 3, 20, 24, 640, 320, 4, 1, 1, 0), "STREAM1X1", {}),
    ((BF16, 2, 16, 20, 24, 32, 1, 3, 1, 1), "SMALL", {}),
    ((BF16, 1, 17, 33, 64, 64, 1, 3, 1, 1), "SMALL", {}),
    ((BF16, 2, 33, 40, 32, 64, 1, 3, 2, 1), "SMALL_S2", {}),
    ((BF16, 4, 32, 32, 128, 128, 1, 3, 1, 1), "TILE16", {}),
    ((BF16, 3, 24, 40, 128, 80, 1, 3, 1, 1), "TILE8", {}),
    ((BF16, 5, 24, 40, 256, 640, 2, 3, 1, 1), "TILE8", {}),
    ((BF16, 3, 32, 40, 160, 640, 2, 3, 1, 1), "WIDE3_16", {}),
    ((BF16, 3, 24, 40, 80, 320, 1, 3, 1, 1), "WIDE3_8", {}),
    ((BF16, 11, 20, 20, 80, 1024, 1, 3, 1, 1), "WIDE3_8", {}),
    ((BF16, 5, 23, 37, 64, 2048, 1, 3, 1, 1), "FLAT", {}),
    ((BF16, 15, 20, 20, 240, 960, 3, 3, 1, 1), "FLAT", {}),
    ((BF16, 3, 9, 9, 96, 80, 1, 3, 1, 0), "GENERIC", {}),
    ((BF16, 2, 10, 12, 64, 64, 2, 3, 1, 1), "GENERIC", {}),
    ((BF16, 2, 12, 12, 128, 64, 1, 3, 2, 1), "GENERIC", {}),
    ((F32, 3, 13, 11, 24, 40, 1, 3, 1, 1), "GENERIC", {}),
    ((F32, 2, 9, 9, 64, 96, 2, 3, 2, 0), "GENERIC", {}),
    ((F32, 3, 32, 40, 64, 80, 1, 3, 1, 1), "TILE16", {}),
    ((F32, 2, 24, 24, 128, 48, 1, 3, 1, 1), "TILE8", {}),
]
# the data gradient runs the flipped-tap conv on dy: its tile route is y3d_conv3x3_tile_route with (Cg, Cn) = (Cout/g, Cin/g)
DGRAD_CASES = [
    ((BF16, 3, 20, 24, 128, 80, 1, 1, 1, 0), "STREAM1X1", {}),
    ((BF16, 3, 20, 24, 640, 320, 4, 1, 1, 0), "STREAM1X1", {}),
    ((BF16, 2, 16, 20, 24, 32, 1, 3, 1, 1), "SMALL", {}),
    ((BF16, 1, 17, 33, 64, 64, 1, 3, 1, 1), "SMALL", {}),
    ((BF16, 2, 33, 40, 32, 64, 1, 3, 2, 1), "S2_DGRAD", {}),
    ((BF16, 4, 20, 20, 64, 128, 1, 3, 2, 1), "S2_DGRAD", {}),
    ((BF16, 4, 32, 32, 128, 128, 1, 3, 1, 1), "TILE16", {}),
    ((BF16, 5, 24, 40, 256, 640, 2, 3, 1, 1), "TILE8", {}),
    ((BF16, 3, 32, 40, 640, 160, 2, 3, 1, 1), "WIDE3_16", {}),
    ((BF16, 3, 24, 40, 128, 80, 1, 3, 1, 1), "WIDE3_8", {}),
    ((BF16, 11, 20, 20, 1024, 80, 1, 3, 1, 1), "WIDE3_8", {}),
    ((BF16, 5, 23, 37, 2048, 64, 1, 3, 1, 1), "FLAT", {}),
    ((BF16, 15, 20, 20, 960, 240, 3, 3, 1, 1), "FLAT", {}),
    ((BF16, 3, 9, 9, 96, 80, 1, 3, 1, 0), "GENERIC", {}),
    ((BF16, 2, 10, 12, 64, 64, 2, 3, 1, 1), "GENERIC", {}),
    ((BF16, 2, 12, 12, 64, 32, 2, 1, 1, 0), "GENERIC", {}),
    ((BF16, 5, 7, 7, 64, 48, 1, 5, 2, 2), "GENERIC", {}),
    ((F32, 3, 13, 11, 24, 40, 1, 3, 1, 1), "GENERIC", {}),
    ((F32, 2, 9, 9, 64, 96, 2, 3, 2, 0), "GENERIC", {}),
    ((F32, 3, 32, 40, 80, 64, 1, 3, 1, 1), "TILE16", {}),
    ((F32, 2, 24, 24, 48, 128, 1, 3, 1, 1), "TILE8", {}),
]
WGRAD_CASES = [
    ((BF16, 2, 16, 16, 32, 32, 1, 3, 1, 1), "WGRAD_SMALL", {}),
    ((BF16, 2, 16, 20, 64, 48, 1, 3, 1, 1), "WGRAD_SMALL", {"accumulate": 1}),
    ((BF16, 2, 16, 16, 128, 128, 1, 3, 1, 1), "WGRAD_TILE", {}),
    ((BF16, 2, 12, 16, 128, 128, 1, 3, 1, 1), "WGRAD_TILE", {}),
    ((BF16, 2, 16, 16, 256, 256, 2, 3, 1, 1), "WGRAD_TILE", {"accumulate": 1}),
    ((BF16, 3, 20, 24, 128, 80, 1, 1, 1, 0), "WGRAD_STREAM1X1", {}),
    ((BF16, 3, 20, 24, 128, 80, 1, 1, 1, 0), "WGRAD_STREAM1X1", {"nsplit": 13}),
    ((BF16, 2, 16, 16, 32, 32, 1, 1, 1, 0), "GENERIC", {}),
    ((BF16, 2, 16, 16, 32, 32, 1, 1, 1, 0), "GENERIC", {"cin_real": 27}),
    ((BF16, 4, 16, 16, 64, 24, 1, 1, 1, 0), "GENERIC", {"nsplit": 70}),
    ((BF16, 4, 16, 16, 64, 24, 1, 1, 1, 0), "GENERIC", {"nsplit": 40, "accumulate": 1}),
    ((BF16, 3, 20, 20, 64, 64, 2, 1, 1, 0), "GENERIC", {"nsplit": 12}),
    ((BF16, 2, 9, 9, 96, 80, 1, 3, 1, 0), "GENERIC", {}),
    ((BF16, 2, 16, 16, 16, 16, 1, 3, 2, 1), "GENERIC", {}),
    ((BF16, 2, 20, 20, 40, 160, 1, 3, 1, 1), "GENERIC", {"nsplit": 3}),
    ((F32, 2, 16, 16, 64, 64, 1, 3, 1, 1), "GENERIC", {}),
    ((F32, 2, 9, 9, 64, 96, 2, 3, 2, 0), "GENERIC", {"nsplit": 5}),
]
CASES = {FWD: FWD_CASES, DGRAD: DGRAD_CASES, WGRAD: WGRAD_CASES}

FWD_ROUTES = {"GENERIC", "STREAM1X1", "SMALL", "SMALL_S2", "TILE8", "TILE16", "WIDE3_8", "WIDE3_16", "FLAT"}
DGRAD_ROUTES = {"GENERIC", "STREAM1X1", "SMALL", "S2_DGRAD", "TILE8", "TILE16", "WIDE3_8", "WIDE3_16", "FLAT"}
WGRAD_ROUTES = {"GENERIC", "WGRAD_SMALL", "WGRAD_TILE", "WGRAD_STREAM1X1"}


# ---- restated launch rules (conv_gemm.hip) ---------------------------------------------------------------------------------------


def _nsplit(case, ex):
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    return ex.get("nsplit") or y3d.lib().conv2d_wgrad_plan(dt, B, H, W, Cin, Cout, g, k, k, s, p)


def _reduce_variant(case, nsplit):
    """launch_wgrad_reduce: the fold kernel (split lanes) for n = Cout * taps * Cg slab elements"""
    _, _, _, _, Cin, Cout, g, k, _, _ = case
    n = Cout * k * k * (Cin // g)
    if n <= 65536 and nsplit >= 64:
        return 16
    if n <= 1048576 and nsplit >= 32:
        return 8
    return 2 if nsplit >= 8 else 1


def _wgrad_tile_w(n):
    return 32 if n <= 32 else (64 if n <= 64 else 128)


def _generic_wgrad_tiles(case):
    """(wd, wx) operand tile widths of conv_wgrad_kernel: output channels per group, k*k*Cin/g"""
    _, _, _, _, Cin, Cout, g, k, _, _ = case
    return _wgrad_tile_w(Cout // g), _wgrad_tile_w(k * k * (Cin // g))


def _wgrad_splits_used(case, nsplit):
    """splits that own pixels: chunk_px = ceil(ceil(M / nsplit) / bpk) * bpk (bpk: 64 bf16, 32 fp32)"""
    dt = case[0]
    Ho, Wo = _out_hw(case)
    M = case[1] * Ho * Wo
    bpk = 64 if dt == BF16 else 32
    chunk = _cdiv(_cdiv(M, nsplit), bpk) * bpk
    return _cdiv(M, chunk)


def _nondense_route(op, route):
    """conv_route when the streamed operand (x; dy for the data gradient) is not pixel-dense: the 1x1 / stride-2 streaming kernels
    drop out (the 1x1 forward with BatchNorm partials is refused: its partial layout was sized for the streaming kernel), every other
    kernel takes full strides"""
    if (op, route) not in DENSE_ONLY:
        return route
    return "REFUSED" if op == FWD else "GENERIC"


def test_train_case_routes():
    """CPU: every training case takes the route it was written for, and the lists reach every route and launch variant"""
    for op, cases in CASES.items():
        for case, want, _ in cases:
            got = _route(op, case)
            assert got == ROUTES[want], (f"{OPNAME[op]} {case} now routes to {ROUTE_NAME.get(got, got)}, not {want}: add a case that "
                                         f"reaches {want}")
    assert {r for _, r, _ in FWD_CASES} == FWD_ROUTES, FWD_ROUTES - {r for _, r, _ in FWD_CASES}
    assert {r for _, r, _ in DGRAD_CASES} == DGRAD_ROUTES, DGRAD_ROUTES - {r for _, r, _ in DGRAD_CASES}
    assert {r for _, r, _ in WGRAD_CASES} == WGRAD_ROUTES, WGRAD_ROUTES - {r for _, r, _ in WGRAD_CASES}
    L = y3d.lib()
    # the resident-tile weight gradient with 8- and 4-row tiles (y3d_wgrad_tile_height: H % 8, else H % 4)
    ths = {8 if c[2] % 8 == 0 else 4 for c, r, _ in WGRAD_CASES if r == "WGRAD_TILE"}
    assert ths == {8, 4}, ths
    # all four fold kernels of launch_wgrad_reduce
    red = {_reduce_variant(c, _nsplit(c, ex)) for c, _, ex in WGRAD_CASES}
    assert red == {16, 8, 2, 1}, red
    # the generic weight gradient's tile widths, each on both axes
    tiles = [_generic_wgrad_tiles(c) for c, r, _ in WGRAD_CASES if r == "GENERIC"]
    assert {t[0] for t in tiles} == {32, 64, 128} and {t[1] for t in tiles} == {32, 64, 128}, tiles
    # fp32 on the generic and tile routes of every op (the resident-tile / small / streaming weight gradients are bf16 only)
    for op, want in ((FWD, {"GENERIC", "TILE8", "TILE16"}), (DGRAD, {"GENERIC", "TILE8", "TILE16"}), (WGRAD, {"GENERIC"})):
        assert {r for c, r, _ in CASES[op] if c[0] == F32} >= want, OPNAME[op]
    for r in ("TILE8", "WIDE3_16", "FLAT", "STREAM1X1", "GENERIC"):
        assert any(c[6] > 1 for c, rr, _ in FWD_CASES if rr == r), f"no grouped forward case on {r}"
        assert any(c[6] > 1 for c, rr, _ in DGRAD_CASES if rr == r), f"no grouped data-gradient case on {r}"
    assert any(c[6] > 1 for c, r, _ in WGRAD_CASES if r in ("GENERIC", "WGRAD_TILE"))
    assert any(c[2] % 8 for c, r, _ in FWD_CASES if r == "WIDE3_8"), "no ragged-height forward case on wide3"
    assert any(c[2] % 8 for c, r, _ in DGRAD_CASES if r == "WIDE3_8"), "no ragged-height data-gradient case on wide3"
    assert any((c[5] // c[6]) % 128 for c, r, _ in FWD_CASES if r in ("WIDE3_16", "WIDE3_8", "FLAT")), "no partial channel tile"
    assert any((c[4] // c[6]) % 128 for c, r, _ in DGRAD_CASES if r in ("WIDE3_16", "WIDE3_8", "FLAT")), "no partial dgrad channel tile"
    assert any(ex.get("cin_real", c[4]) < c[4] for c, r, ex in WGRAD_CASES if r == "GENERIC"), "no Cin_real < Cin case"
    assert any(ex.get("accumulate") for _, _, ex in WGRAD_CASES), "no accumulate = 1 case"
    # a free nsplit that leaves empty trailing splits, on each weight-gradient route that takes one
    for r in ("GENERIC", "WGRAD_STREAM1X1"):
        assert any("nsplit" in ex and _wgrad_splits_used(c, ex["nsplit"]) < ex["nsplit"] for c, rr, ex in WGRAD_CASES if rr == r), r
    # a case with Cin_real < Cin must still route to the generic kernel (cin_full is false): y3d_conv2d_route assumes full channels
    assert all(r == "GENERIC" for c, r, ex in WGRAD_CASES if ex.get("cin_real", c[4]) < c[4])
    # the planned nsplit of the resident kernels is a fixed function of the geometry: the routes that take a free one are the others
    for c, r, ex in WGRAD_CASES:
        if r in ("WGRAD_SMALL", "WGRAD_TILE"):
            assert "nsplit" not in ex
    assert L.conv2d_route(BF16, FWD, EPI_PARTIALS, 2, 8, 8, 64, 64, 1, 3, 3, 1, 1) >= 0


# ---- operands --------------------------------------------------------------------------------------------------------------------


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, amp, density, gen):
    """integers uniform in +-{1..amp} with probability `density`, else 0 (fp32, device)"""
    mag = torch.randint(1, amp + 1, shape, generator=gen, device=DEV).float()
    u = torch.rand(shape, generator=gen, device=DEV)
    return torch.where(u < density / 2, mag, torch.where(u > 1 - density / 2, -mag, torch.zeros_like(mag)))


def _wide(shape, gen):
    """a * 2^-6, a an integer with 12 significant bits (2048..4095), random sign: representable in fp32, not in bf16 / xf32"""
    a = torch.randint(2048, 4096, shape, generator=gen, device=DEV).float()
    sgn = torch.where(torch.rand(shape, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
    return a * sgn * 2.0 ** -6


def _amp(k_eff):
    """amplitude of the bf16-mode integers: E[v^2] of +-{1..A} is (A+1)(2A+1)/6; aim the accumulator's spread at ~500"""
    want = 500.0 / math.sqrt(max(k_eff, 1.0))
    for a in range(1, 17):
        if (a + 1) * (2 * a + 1) / 6 >= want:
            return a
    return 16


def _place(t, dt, m, seed_off=0):
    """t (B, H, W, C) fp32 -> a view of a sentinel-filled buffer in the compute dtype: channel slot [OFF, OFF + C), and m pixels of
    sentinel around the map (a spatial crop) when m > 0.  Returns (buffer, view)."""
    B, H, W, C = t.shape
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    buf = torch.full((B, H + 2 * m, W + 2 * m, C + EXTRA), SENT, dtype=tdt, device=DEV)
    v = buf[:, m:m + H, m:m + W, OFF:OFF + C]
    v.copy_(t.to(tdt))
    return buf, v


def _slot(shape, dt):
    """NaN-filled output buffer (B, H, W, C + EXTRA) and its channel slot"""
    B, H, W, C = shape
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    buf = torch.full((B, H, W, C + EXTRA), float("nan"), dtype=tdt, device=DEV)
    return buf, buf[..., OFF:OFF + C]


def _check_slot(buf, C, what):
    assert bool(buf[..., :OFF].isnan().all()) and bool(buf[..., OFF + C:].isnan().all()), f"{what}: a store left the output slot"


def _fail(what, got, ref, tol, idx_fmt):
    """AssertionError naming the first bad element"""
    bad = ~((got - ref).abs() <= tol)
    i = int(bad.reshape(-1).nonzero()[0][0])
    tolv = float(tol.reshape(-1)[i]) if torch.is_tensor(tol) else float(tol)
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong; first at {idx_fmt(i)}: got {float(got.reshape(-1)[i])!r} "
                         f"expected {float(ref.reshape(-1)[i])!r} bound {tolv:.3g}")


def _is_tie(a):
    """|a| exactly halfway between two bf16 neighbours (a: exact fp64 integers / fixed-point values)"""
    x = a.abs()
    nz = x > 0
    e = torch.floor(torch.log2(torch.where(nz, x, torch.ones_like(x))))
    q = x / torch.exp2(e - 7)
    return nz & (q - torch.floor(q) == 0.5)


def _acc_chunks(xd, wd, g, k, s, p, B, Ho, Wo, full_px, gen):
    """exact accumulators (fp64, device) at every pixel (full_px) or a sample; -> (acc (N, Cout), b, h, w)"""
    b, h, w = _sample_pixels(B, Ho, Wo, gen, full_px)
    outs = []
    for i in range(0, len(b), 8192):
        outs.append(_exact_acc(xd, wd, g, k, s, p, b[i:i + 8192], h[i:i + 8192], w[i:i + 8192]))
    return torch.cat(outs), b.to(DEV), h.to(DEV), w.to(DEV)


def _flip_dgrad(dy, H, W, k, s, p):
    """the data gradient as a stride-1 conv: dy scattered into a zero map (B, H + k - 1, W + k - 1, Cout) at k-1-p + ho*s, and the
    weight transposed per group with flipped taps (Cin, Cout/g, k, k); then dx = _exact_acc(dyd, wT, g, k, 1, 0, ...)"""
    B, Ho, Wo, Cout = dy.shape
    dyd = torch.zeros(B, H + k - 1, W + k - 1, Cout, dtype=torch.float32, device=DEV)
    o = k - 1 - p
    dyd[:, o:o + (Ho - 1) * s + 1:s, o:o + (Wo - 1) * s + 1:s] = dy
    return dyd


def _flip_weight(w, g):
    Cout, Cg, k, _ = w.shape
    Cn = Cout // g
    wt = w.reshape(g, Cn, Cg, k, k).transpose(1, 2).flip(-1, -2)  # (g, Cg, Cn, k, k)
    return wt.reshape(g * Cg, Cn, k, k).contiguous()


def _exact_dw(xd, dyd, case, co_sel=None, ci_sel=None):
    """exact weight gradient (fp64, device): dW[co, ci, r, q] = sum_p dy[p, co] x[p*s - pad + (r, q), g(co) * Cg + ci].
    co_sel / ci_sel: index subsets (default all); -> (len(co), len(ci), k, k)"""
    _, B, H, W, Cin, Cout, g, k, s, p = case
    Ho, Wo = _out_hw(case)
    Cg, Cn = Cin // g, Cout // g
    co_sel = torch.arange(Cout, device=DEV) if co_sel is None else co_sel.to(DEV)
    ci_sel = torch.arange(Cg, device=DEV) if ci_sel is None else ci_sel.to(DEV)
    out = torch.zeros(len(co_sel), len(ci_sel), k, k, dtype=torch.float64, device=DEV)
    M = B * Ho * Wo
    for gi in range(g):
        rows = ((co_sel // Cn) == gi).nonzero().reshape(-1)
        if len(rows) == 0:
            continue
        dyg = dyd.reshape(M, Cout)[:, co_sel[rows]].double()  # (M, a)
        xg = xd[..., gi * Cg + ci_sel]  # (B, H, W, b)
        xp = torch.zeros(B, H + 2 * p, W + 2 * p, len(ci_sel), dtype=torch.float32, device=DEV)
        xp[:, p:p + H, p:p + W] = xg
        for r in range(k):
            for q in range(k):
                xs = xp[:, r:r + (Ho - 1) * s + 1:s, q:q + (Wo - 1) * s + 1:s].reshape(M, -1).double()
                out[rows, :, r, q] = dyg.T @ xs
    return out


# ---- one launch, checked ---------------------------------------------------------------------------------------------------------


def _n_max(route, case, rows):
    """most pixels one BatchNorm partial row covers (module docstring)"""
    _, B, H, W, Cin, Cout, g, k, s, p = case
    Ho, Wo = _out_hw(case)
    if route in ("TILE8", "WIDE3_8", "GENERIC"):
        return 128
    if route in ("TILE16", "WIDE3_16"):
        return 256
    if route == "FLAT":
        return 512
    if route in ("SMALL", "SMALL_S2"):
        return _cdiv(B * _cdiv(Ho, 8) * _cdiv(Wo, 16), rows) * 128
    if route == "STREAM1X1":
        return _cdiv(_cdiv(B * Ho * Wo, 128), rows) * 128
    raise AssertionError(route)


def run_fwd(case, mode, seed, crop=0, bias=False, check_stats=True, full_px=True, strides=None):
    """y3d_conv2d_fwd with BatchNorm partials (or a bias).  mode 'int': bf16 rounding test; 'x' / 'w': fp32, that operand wide.
    strides: (xsb, xsh, xsw, ysw) to replay exactly (x then lives in a sentinel-filled buffer of that shape)."""
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = _out_hw(case)
    route = _rname(FWD, case)
    tag = f"fwd {route} {case} mode={mode} crop={crop}"
    gd = _gen(seed)
    Cg = Cin // g
    if mode == "int":
        a = _amp(k * k * Cg)
        xd = _ints((B, H, W, Cin), a, 1.0, gd)
        wd = _ints((Cout, Cg, k, k), a, 1.0, gd)
    elif mode == "x":
        xd = _wide((B, H, W, Cin), gd)
        wd = _ints((Cout, Cg, k, k), 2, min(1.0, 3000.0 / (1.5 * k * k * Cg)), gd)
    else:
        xd = _ints((B, H, W, Cin), 2, min(1.0, 3000.0 / (1.5 * k * k * Cg)), gd)
        wd = _wide((Cout, Cg, k, k), gd)
    # sum |x||w| per output <= max|x| * max over co of sum |w[co]|  (or max|w| * k^2 * max over pixels of sum_c |x|)
    sx = float(xd.abs().max()) * float(wd.abs().reshape(Cout, -1).sum(1).max())
    sw_ = float(wd.abs().max()) * k * k * float(xd.abs().sum(3).max())
    lim = 2.0 ** 24 if mode == "int" else 2.0 ** 18
    assert min(sx, sw_) < lim, f"{tag}: operands too large for an exact reference ({min(sx, sw_):.3g})"
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    if strides is None:
        xbuf, xin = _place(xd, dt, crop)
        xsb, xsh, xsw = xin.stride(0), xin.stride(1), xin.stride(2)
        ybuf, y = _slot((B, Ho, Wo, Cout), dt)
        ysw = ybuf.stride(2)
    else:
        xsb, xsh, xsw, ysw = strides
        xbuf = torch.full(((B - 1) * xsb + (H - 1) * xsh + (W - 1) * xsw + Cin + 8,), SENT, dtype=tdt, device=DEV)
        xin = xbuf.as_strided((B, H, W, Cin), (xsb, xsh, xsw, 1))
        xin.copy_(xd.to(tdt))
        ybuf = torch.full((B * Ho * Wo * ysw + 8,), float("nan"), dtype=tdt, device=DEV)
        y = ybuf[:B * Ho * Wo * ysw].view(B, Ho, Wo, ysw)[..., :Cout]
    K = k * k * Cg
    wp = torch.empty(Cout * K, dtype=tdt, device=DEV)
    L.pack_weight_fwd(dt, wd.data_ptr(), wp.data_ptr(), Cout, Cg, Cg, k, k, st)
    bvec = _ints((Cout,), 8, 1.0, gd) if bias else None
    rows = L.conv2d_stat_rows(dt, B, H, W, Cin, Cout, g, k, k, s, p)
    part = None if bias or not check_stats else torch.full(((rows + 1) * Cout * 2,), float("nan"), device=DEV)
    dense = (H == 1 or xsh == W * xsw) and (B == 1 or xsb == H * W * xsw)
    expect = route if dense else _nondense_route(FWD, route)
    call = lambda: L.conv2d_fwd(dt, xin.data_ptr(), xsb, xsh, xsw, B, H, W, Cin, wp.data_ptr(), bvec.data_ptr() if bias else None,
                                y.data_ptr(), ysw, Ho, Wo, Cout, g, k, k, s, p, part.data_ptr() if part is not None else None, st)
    if expect == "REFUSED" and part is not None:
        with pytest.raises(Y3DError, match="pixel-dense"):
            call()
        return expect
    call()
    torch.cuda.synchronize()
    if strides is None:
        _check_slot(ybuf, Cout, tag)
    else:
        assert bool(ybuf.view(-1)[:B * Ho * Wo * ysw].view(B, Ho, Wo, ysw)[..., Cout:].isnan().all()), f"{tag}: a store left the slot"
    gen = torch.Generator().manual_seed(seed)
    acc, b, h, w = _acc_chunks(xd, wd, g, k, s, p, B, Ho, Wo, full_px, gen)
    if bias:
        acc = acc + bvec.double()
    got = y[b, h, w].double()
    ref = acc.float().to(tdt).double()  # exact fp32, then one RNE to the storage type
    if not bool((got == ref).all()):
        _fail(tag, got, ref, 0.0, lambda i: f"pixel {(int(b[i // Cout]), int(h[i // Cout]), int(w[i // Cout]))} channel {i % Cout} "
                                             f"(acc {float(acc.reshape(-1)[i])})")
    if mode == "int" and strides is None:
        frac = float((acc.abs() > 256).double().mean())
        assert frac >= 0.25, f"{tag}: only {frac:.0%} of the accumulators exceed 256 - the store is barely rounding"
        assert bool(_is_tie(acc).any()), f"{tag}: no exact bf16 tie among the accumulators"
    if part is not None:
        pr = part.view(rows + 1, Cout, 2)
        assert not bool(pr[:rows].isnan().any()), f"{tag}: a partial row below y3d_conv2d_stat_rows ({rows}) was not written"
        assert bool(pr[rows].isnan().all()), f"{tag}: a partial row past y3d_conv2d_stat_rows was written"
        if dt == BF16 and mode == "int":
            ys = y.double()
            n = _n_max(route, case, rows)
            assert n * float(ys.abs().max()) < 2 ** 24, f"{tag}: a partial row's sum |y| may not be exact in fp32"
            s1 = pr[:rows, :, 0].double().sum(0)
            s2 = pr[:rows, :, 1].double().sum(0)
            r1 = ys.sum((0, 1, 2))
            r2 = (ys * ys).sum((0, 1, 2))
            if not bool((s1 == r1).all()):
                _fail(f"{tag} partial sum y", s1, r1, 0.0, lambda i: f"channel {i}")
            tol = (n - 1) * 2.0 ** -24 * (1 + 2.0 ** -10) * r2 + 2.0 ** -40 * r2
            if not bool(((s2 - r2).abs() <= tol).all()):
                _fail(f"{tag} partial sum y^2 (n_max {n})", s2, r2, tol, lambda i: f"channel {i}")
            if full_px:
                # the test can tell stored values from accumulators: the accumulators' statistics miss the bound
                a = acc.reshape(B, Ho, Wo, Cout)
                gap1 = (a.sum((0, 1, 2)) - r1).abs()
                gap2 = ((a * a).sum((0, 1, 2)) - r2).abs()
                assert bool((gap1 > 0).any()) and bool((gap2 > tol).any()), f"{tag}: accumulator and stored statistics indistinguishable"
    return expect


def run_dgrad(case, mode, seed, crop=0, full_px=True, strides=None):
    """y3d_conv2d_bwd_data: dy a channel slot (offset OFF, pitch Cout + EXTRA: dsw > Cout, as dx_range makes it) of a sentinel buffer,
    optionally a spatial crop; dx written into a NaN-filled slot with xsw > Cin.  strides: (dsb, dsh, dsw, xsw) to replay."""
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = _out_hw(case)
    route = _rname(DGRAD, case)
    tag = f"dgrad {route} {case} mode={mode} crop={crop}"
    gd = _gen(seed)
    Cg, Cn = Cin // g, Cout // g
    keff = k * k * Cn / (s * s)
    if mode == "int":
        a = _amp(keff)
        dy = _ints((B, Ho, Wo, Cout), a, 1.0, gd)
        wd = _ints((Cout, Cg, k, k), a, 1.0, gd)
    elif mode == "dy":
        dy = _wide((B, Ho, Wo, Cout), gd)
        wd = _ints((Cout, Cg, k, k), 2, min(1.0, 3000.0 / (1.5 * k * k * Cn)), gd)
    else:
        dy = _ints((B, Ho, Wo, Cout), 2, min(1.0, 3000.0 / (1.5 * k * k * Cn)), gd)
        wd = _wide((Cout, Cg, k, k), gd)
    # sum |dy||w| per dx element <= max|dy| * max over ci of sum |w[:, ci]|  (or max|w| * k^2 * max over pixels of sum_c |dy|)
    b1 = float(dy.abs().max()) * float(wd.abs().transpose(0, 1).reshape(Cg, -1).sum(1).max())
    b2 = float(wd.abs().max()) * k * k * float(dy.abs().sum(3).max())
    lim = 2.0 ** 24 if mode == "int" else 2.0 ** 18
    assert min(b1, b2) < lim, f"{tag}: operands too large for an exact reference"
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    if strides is None:
        dbuf, dyv = _place(dy, dt, crop)
        dsb, dsh, dsw = dyv.stride(0), dyv.stride(1), dyv.stride(2)
        xbuf, dx = _slot((B, H, W, Cin), dt)
        xsw = xbuf.stride(2)
    else:
        dsb, dsh, dsw, xsw = strides
        off = dsw - Cout  # the dx_range view: the last Cout channels of a wider gradient
        dbuf = torch.full(((B - 1) * dsb + (Ho - 1) * dsh + (Wo - 1) * dsw + dsw + 8,), SENT, dtype=tdt, device=DEV)
        dyv = dbuf[off:].as_strided((B, Ho, Wo, Cout), (dsb, dsh, dsw, 1))
        dyv.copy_(dy.to(tdt))
        xbuf = torch.full((B * H * W * xsw,), float("nan"), dtype=tdt, device=DEV).view(B, H, W, xsw)
        dx = xbuf[..., :Cin]
    kp = L.conv_kpad(dt, k * k * Cn)
    wpd = torch.empty(Cin * kp, dtype=tdt, device=DEV)
    L.pack_weight_dgrad(dt, wd.data_ptr(), wpd.data_ptr(), Cout, Cg, g, k, k, st)
    L.conv2d_bwd_data(dt, dyv.data_ptr(), dsb, dsh, dsw, B, Ho, Wo, Cout, wpd.data_ptr(), dx.data_ptr(), xsw, H, W, Cin, g, k, k, s, p, st)
    torch.cuda.synchronize()
    dense = (Ho == 1 or dsh == Wo * dsw) and (B == 1 or dsb == Ho * Wo * dsw)
    expect = route if dense else _nondense_route(DGRAD, route)
    tag = f"{tag} (expected route {expect})"
    if strides is None:
        _check_slot(xbuf, Cin, tag)
    else:
        assert bool(xbuf[..., Cin:].isnan().all()), f"{tag}: a store left the dx slot"
    gen = torch.Generator().manual_seed(seed)
    dyd = _flip_dgrad(dy, H, W, k, s, p)
    acc, b, h, w = _acc_chunks(dyd, _flip_weight(wd, g), g, k, 1, 0, B, H, W, full_px, gen)
    got = dx[b, h, w].double()
    ref = acc.float().to(tdt).double()
    if not bool((got == ref).all()):
        _fail(tag, got, ref, 0.0, lambda i: f"pixel {(int(b[i // Cin]), int(h[i // Cin]), int(w[i // Cin]))} channel {i % Cin} "
                                             f"(acc {float(acc.reshape(-1)[i])})")
    if mode == "int" and strides is None:
        frac = float((acc.abs() > 256).double().mean())
        assert frac >= 0.25, f"{tag}: only {frac:.0%} of the accumulators exceed 256"
        assert bool(_is_tie(acc).any()), f"{tag}: no exact bf16 tie"
    return expect


def run_wgrad(case, mode, seed, ex, crop=0, strides=None, sample=False):
    """y3d_conv2d_bwd_weight: x a channel slot (optionally cropped) of a sentinel buffer, dy a channel slot (dsw > Cout), the slab and
    dW NaN-filled (or dW pre-filled with integers for accumulate = 1).  strides: (xsb, xsh, xsw, dsw, cin_real, nsplit) to replay."""
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = _out_hw(case)
    M = B * Ho * Wo
    route = _rname(WGRAD, case)
    cin_real = ex.get("cin_real", Cin)
    nsplit = _nsplit(case, ex)
    accumulate = ex.get("accumulate", 0)
    gd = _gen(seed)
    Cg, Cn = Cin // g, Cout // g
    if mode == "int":
        # Sum over all pixels of |x||dy| < 2^24: amplitude 4, density from M
        d = min(1.0, math.sqrt(2.0 ** 22 / (M * 16.0)))
        xd = _ints((B, H, W, Cin), 4, d, gd)
        dy = _ints((B, Ho, Wo, Cout), 4, d, gd)
    elif mode == "x":
        xd = _wide((B, H, W, Cin), gd)
        dy = _ints((B, Ho, Wo, Cout), 2, min(1.0, 2000.0 / (1.5 * M)), gd)
    else:
        xd = _ints((B, H, W, Cin), 2, min(1.0, 2000.0 / (1.5 * B * H * W)), gd)
        dy = _wide((B, Ho, Wo, Cout), gd)
    if cin_real < Cin:
        xd[..., cin_real:] = 0  # the padded channels of the stem's column tensor are zeros
    b1 = float(xd.abs().max()) * float(dy.abs().reshape(M, Cout).sum(0).max())
    b2 = float(dy.abs().max()) * float(xd.abs().reshape(-1, Cin).sum(0).max())
    lim = 2.0 ** 24 if mode == "int" else 2.0 ** 18
    assert min(b1, b2) < lim, f"wgrad {case}: operands too large for an exact reference"
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    if strides is None:
        xbuf, xin = _place(xd, dt, crop)
        xsb, xsh, xsw = xin.stride(0), xin.stride(1), xin.stride(2)
        dbuf, dyv = _place(dy, dt, 0)
        dsw = dyv.stride(2)
    else:
        xsb, xsh, xsw, dsw = strides
        xbuf = torch.full(((B - 1) * xsb + (H - 1) * xsh + (W - 1) * xsw + Cin + 8,), SENT, dtype=tdt, device=DEV)
        xin = xbuf.as_strided((B, H, W, Cin), (xsb, xsh, xsw, 1))
        xin.copy_(xd.to(tdt))
        dbuf = torch.full((M * dsw + 8,), SENT, dtype=tdt, device=DEV)
        dyv = dbuf[:M * dsw].view(B, Ho, Wo, dsw)[..., :Cout]
        dyv.copy_(dy.to(tdt))
    dense = (H == 1 or xsh == W * xsw) and (B == 1 or xsb == H * W * xsw)
    expect = route if (dense and cin_real == Cin) else ("GENERIC" if cin_real < Cin else _nondense_route(WGRAD, route))
    if not dense and expect != route and expect == "GENERIC" and "nsplit" not in ex:
        # the resident kernels' plan does not apply to the generic kernel the view falls back to
        nsplit = L.conv2d_wgrad_splits(dt, B, Ho, Wo, Cout, Cg, g, k, k)
    tag = (f"wgrad {route} {case} mode={mode} crop={crop} nsplit={nsplit} cin_real={cin_real} accumulate={accumulate} "
           f"(expected route {expect})")
    slab = torch.full((nsplit * Cout * k * k * Cg,), float("nan"), device=DEV)
    ci_n = cin_real if g == 1 else Cg
    prior = None
    if accumulate:
        prior = _ints((Cout, ci_n, k, k), 64, 1.0, gd)
        dW = prior.clone()
    else:
        dW = torch.full((Cout, ci_n, k, k), float("nan"), device=DEV)
    L.conv2d_bwd_weight(dt, xin.data_ptr(), xsb, xsh, xsw, B, H, W, Cin, cin_real, dyv.data_ptr(), dsw, Ho, Wo, Cout, g, k, k, s, p,
                        slab.data_ptr(), nsplit, dW.data_ptr(), accumulate, st)
    torch.cuda.synchronize()
    if sample:
        gen = torch.Generator().manual_seed(seed)
        first = torch.arange(min(16, Cout))
        co = torch.unique(torch.cat((first, torch.arange(max(0, Cout - 16), Cout), torch.randint(0, Cout, (16,), generator=gen))))
        ci = torch.unique(torch.cat((torch.arange(min(16, ci_n)), torch.arange(max(0, ci_n - 16), ci_n),
                                     torch.randint(0, ci_n, (16,), generator=gen))))
        assert int(co.max()) < Cout and int(ci.max()) < ci_n  # indices into per-group channels, checked on the host
        ref = _exact_dw(xd, dy, case, co, ci)
        got = dW[co.to(DEV)][:, ci.to(DEV)].double()
        pri = prior[co.to(DEV)][:, ci.to(DEV)].double() if accumulate else 0.0
        idx = lambda i: f"dW[{int(co[i // (len(ci) * k * k)])}, {int(ci[(i // (k * k)) % len(ci)])}, tap {i % (k * k)}]"
    else:
        ref = _exact_dw(xd, dy, case)[:, :ci_n]
        got = dW.double()
        pri = prior.double() if accumulate else 0.0
        idx = lambda i: f"dW[{i // (ci_n * k * k)}, {(i // (k * k)) % ci_n}, tap {i % (k * k)}]"
    ref = ref + pri
    if not bool((got == ref).all()):
        _fail(tag, got, ref, 0.0, idx)
    return expect


# ---- B + D: bf16 rounding, placement, poison --------------------------------------------------------------------------------------


def _ids(cases):
    return [f"{r}-" + "x".join(map(str, c)) + "".join(f"-{k}{v}" for k, v in ex.items()) for c, r, ex in cases]


BF_FWD = [c for c in FWD_CASES if c[0][0] == BF16]
BF_DGRAD = [c for c in DGRAD_CASES if c[0][0] == BF16]
BF_WGRAD = [c for c in WGRAD_CASES if c[0][0] == BF16]


@pytest.mark.gpu
@pytest.mark.parametrize("crop", [0, 1])
@pytest.mark.parametrize("case,route,ex", BF_FWD, ids=_ids(BF_FWD))
def test_fwd_partials_bf16_exact(case, route, ex, crop):
    got = run_fwd(case, "int", seed=sum(case) + crop, crop=crop)
    assert got == (route if crop == 0 else _nondense_route(FWD, route))


@pytest.mark.gpu
@pytest.mark.parametrize("crop", [0, 1])
@pytest.mark.parametrize("case,route,ex", BF_DGRAD, ids=_ids(BF_DGRAD))
def test_dgrad_bf16_exact(case, route, ex, crop):
    run_dgrad(case, "int", seed=sum(case) + 11 + crop, crop=crop)


@pytest.mark.gpu
@pytest.mark.parametrize("crop", [0, 1])
@pytest.mark.parametrize("case,route,ex", BF_WGRAD, ids=_ids(BF_WGRAD))
def test_wgrad_bf16_exact(case, route, ex, crop):
    run_wgrad(case, "int", seed=sum(case) + 23 + crop, ex=ex, crop=crop)


# ---- C: fp32 mode with operands bf16 / xf32 cannot hold ---------------------------------------------------------------------------

F32_FWD = [(c, r, ex, m) for i, (c, r, ex) in enumerate(x for x in FWD_CASES if x[0][0] == F32) for m in ("x", "w")]
F32_DGRAD = [(c, r, ex, m) for (c, r, ex) in DGRAD_CASES if c[0] == F32 for m in ("dy", "w")]
F32_WGRAD = [(c, r, ex, m) for (c, r, ex) in WGRAD_CASES if c[0] == F32 for m in ("x", "dy")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,route,ex,wide", F32_FWD, ids=[f"{r}-{m}-" + "x".join(map(str, c)) for c, r, _, m in F32_FWD])
def test_fwd_f32_exact(case, route, ex, wide):
    run_fwd(case, wide, seed=sum(case) + 5, check_stats=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case,route,ex,wide", F32_DGRAD, ids=[f"{r}-{m}-" + "x".join(map(str, c)) for c, r, _, m in F32_DGRAD])
def test_dgrad_f32_exact(case, route, ex, wide):
    run_dgrad(case, wide, seed=sum(case) + 9)


@pytest.mark.gpu
@pytest.mark.parametrize("case,route,ex,wide", F32_WGRAD, ids=[f"{r}-{m}-" + "x".join(map(str, c)) for c, r, _, m in F32_WGRAD])
def test_wgrad_f32_exact(case, route, ex, wide):
    run_wgrad(case, wide, seed=sum(case) + 13, ex=ex)


# ---- E: every training geometry of the benchmark step -----------------------------------------------------------------------------


@pytest.fixture(scope="module")
def train_launches():
    """distinct argument lists (pointers dropped) of every conv2d_fwd / conv2d_bwd_data / conv2d_bwd_weight launch of one eager bf16
    S-3D training step at B = 32, 640 x 640"""
    import bench

    L = y3d.lib()
    rec = {"fwd": {}, "dgrad": {}, "wgrad": {}}
    real = {n: getattr(L, n) for n in ("conv2d_fwd", "conv2d_bwd_data", "conv2d_bwd_weight")}

    def fwd(dt, x, xsb, xsh, xsw, B, H, W, Cin, wp, bias, y, ysw, Ho, Wo, Cout, g, kh, kw, s, p, part, st):
        rec["fwd"].setdefault((dt, B, H, W, Cin, Cout, g, kh, s, p, xsb, xsh, xsw, ysw, bias is not None, part is not None), None)
        return real["conv2d_fwd"](dt, x, xsb, xsh, xsw, B, H, W, Cin, wp, bias, y, ysw, Ho, Wo, Cout, g, kh, kw, s, p, part, st)

    def dgrad(dt, dy, dsb, dsh, dsw, B, Ho, Wo, Cout, wpd, dx, xsw, H, W, Cin, g, kh, kw, s, p, st):
        rec["dgrad"].setdefault((dt, B, H, W, Cin, Cout, g, kh, s, p, dsb, dsh, dsw, xsw), None)
        return real["conv2d_bwd_data"](dt, dy, dsb, dsh, dsw, B, Ho, Wo, Cout, wpd, dx, xsw, H, W, Cin, g, kh, kw, s, p, st)

    def wgrad(dt, x, xsb, xsh, xsw, B, H, W, Cin, cin_real, dy, dsw, Ho, Wo, Cout, g, kh, kw, s, p, slab, nsplit, dw, acc, st):
        rec["wgrad"].setdefault((dt, B, H, W, Cin, Cout, g, kh, s, p, xsb, xsh, xsw, dsw, cin_real, nsplit, acc), None)
        return real["conv2d_bwd_weight"](dt, x, xsb, xsh, xsw, B, H, W, Cin, cin_real, dy, dsw, Ho, Wo, Cout, g, kh, kw, s, p, slab,
                                         nsplit, dw, acc, st)

    old = y3d.compute_dtype()
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "conv2d_fwd", fwd)
        mp.setattr(L, "conv2d_bwd_data", dgrad)
        mp.setattr(L, "conv2d_bwd_weight", wgrad)
        try:
            model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").to(DEV).train()
            if hasattr(model.model[-1], "restack"):
                model.model[-1].restack()
            batch = bench.synth_batch(32, 640, 640, 0, DEV)
            loss, _ = model(batch)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            if old is not None:
                y3d.set_compute_dtype(old)
    del model, batch, loss
    torch.cuda.empty_cache()
    return {k: sorted(v) for k, v in rec.items()}


@pytest.mark.gpu
def test_every_train_geometry(train_launches):
    """each distinct conv launch of the training step, replayed at its geometry and strides with integer operands: y and dx at
    sampled pixels (bit-exact RNE), BatchNorm partials in full, dW on every tap of the first / last / random channels"""
    seen = {"fwd": set(), "dgrad": set(), "wgrad": set()}
    n = {k: 0 for k in seen}
    assert len(train_launches["fwd"]) >= 20 and len(train_launches["wgrad"]) >= 20, {k: len(v) for k, v in train_launches.items()}
    for i, (dt, B, H, W, Cin, Cout, g, k, s, p, xsb, xsh, xsw, ysw, bias, part) in enumerate(train_launches["fwd"]):
        case = (dt, B, H, W, Cin, Cout, g, k, s, p)
        seen["fwd"].add(_rname(FWD, case))
        run_fwd(case, "int", seed=2000 + i, bias=bias, check_stats=part, full_px=False, strides=(xsb, xsh, xsw, ysw))
        n["fwd"] += 1
    for i, (dt, B, H, W, Cin, Cout, g, k, s, p, dsb, dsh, dsw, xsw) in enumerate(train_launches["dgrad"]):
        case = (dt, B, H, W, Cin, Cout, g, k, s, p)
        seen["dgrad"].add(_rname(DGRAD, case))
        run_dgrad(case, "int", seed=3000 + i, full_px=False, strides=(dsb, dsh, dsw, xsw))
        n["dgrad"] += 1
    for i, (dt, B, H, W, Cin, Cout, g, k, s, p, xsb, xsh, xsw, dsw, cin_real, nsplit, acc) in enumerate(train_launches["wgrad"]):
        case = (dt, B, H, W, Cin, Cout, g, k, s, p)
        seen["wgrad"].add(_rname(WGRAD, case))
        run_wgrad(case, "int", seed=4000 + i, ex={"nsplit": nsplit, "cin_real": cin_real, "accumulate": acc},
                  strides=(xsb, xsh, xsw, dsw), sample=True)
        n["wgrad"] += 1
    assert all(n[k] == len(train_launches[k]) for k in n), (n, {k: len(v) for k, v in train_launches.items()})
    print("train step routes:", {k: sorted(v) for k, v in seen.items()}, "launches replayed:", n)
