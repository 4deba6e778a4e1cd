"""The eval conv epilogues against fp64: y3d_conv2d_fwd_affine (folded BatchNorm + SiLU in the conv epilogue) and
y3d_conv2d_fwd_affine_res (the same plus the Bottleneck residual) on every kernel that carries them, and at every geometry the
S-3D eval forward launches.

* operands: x, w in {0, +-1}, sparse: the accumulator is an exact integer on every kernel, so the reference is exact up to the
  epilogue: z_ref = silu(acc * scale + shift) (+ res) in fp64 from fp32 scale / shift;
* bound: ONE bf16 rounding of the result plus the fp32 epilogue arithmetic (v_exp_f32 and v_rcp_f32 in fast_sigmoid_f):
  |z - z_ref| <= 2^-8 |z_ref| + 2^-20 (|silu term| + |res|) + 2^-22 (|acc * scale| + |shift|) + 1e-30.  The last term is the
  rounding of u = acc * scale + shift: the kernels multiply and add as two fp32 operations (no FMA), so where u cancels its error
  is one ulp of the product, not of u (silu' <= 1.1).  fp32 mode: no output rounding; v_exp_f32 on the rounded product
  u * log2(e) adds |u| ulps to the sigmoid, so 2^-22 |z_ref| + 2^-22 (4 + |u|) |silu term| + 2^-23 |res| + the same u term;
* placement: the output is a channel slot of a wider NaN-filled NHWC buffer (ysw > Cout, as ops.out_tensor's concat slots); every
  channel outside the slot must still be NaN afterwards.
The route each case takes comes from y3d_conv2d_route, and a CPU test checks that the case list still reaches every kernel."""
import math
import re

import pytest
import torch

from conftest import ROOT

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402
from yolov10_3d_amd._lib import BF16, F32  # noqa: E402

DEV = "cuda"
OFF, EXTRA = 8, 24  # output slot: channels [OFF, OFF + Cout) of a buffer with Cout + EXTRA channels


def _route_codes():
    src = open(f"{ROOT}/include/y3d.h").read()
    return {k: int(v) for k, v in re.findall(r"\bY3D_ROUTE_(\w+)\s*=\s*(\d+)", src)}


ROUTES = _route_codes()
ROUTE_NAME = {v: k for k, v in ROUTES.items()}
EPI_AFFINE, EPI_AFFINE_RES = 2, 3

# (dtype, B, H, W, Cin, Cout, groups, k, stride, pad) -> the route y3d_conv2d_route gives today (asserted by test_case_routes)
AFFINE_CASES = [
    # conv3x3_small.hip: LDS row of 64 bytes (Cin <= 32) / 128 bytes, 1-4 output-channel tiles of 16; ragged tiles, Cout % 16 != 0
    ((BF16, 3, 21, 27, 32, 16, 1, 3, 1, 1), "SMALL"),
    ((BF16, 2, 16, 20, 24, 32, 1, 3, 1, 1), "SMALL"),
    ((BF16, 2, 12, 40, 16, 48, 1, 3, 1, 1), "SMALL"),
    ((BF16, 1, 17, 33, 32, 64, 1, 3, 1, 1), "SMALL"),
    ((BF16, 3, 21, 27, 64, 12, 1, 3, 1, 1), "SMALL"),
    ((BF16, 2, 16, 20, 48, 24, 1, 3, 1, 1), "SMALL"),
    ((BF16, 3, 13, 11, 40, 40, 1, 3, 1, 1), "SMALL"),
    ((BF16, 1, 17, 33, 64, 64, 1, 3, 1, 1), "SMALL"),
    # conv3x3_tile.hip (bf16: fewer 512-pixel tiles than half the CUs)
    ((BF16, 4, 32, 32, 128, 128, 1, 3, 1, 1), "TILE16"),
    ((BF16, 5, 32, 48, 128, 320, 1, 3, 1, 1), "TILE16"),
    ((BF16, 3, 24, 40, 128, 80, 1, 3, 1, 1), "TILE8"),
    ((BF16, 5, 24, 40, 256, 640, 2, 3, 1, 1), "TILE8"),
    # conv3x3_wide3.hip: 16- and 8-row tiles, the ragged 20-row map; groups with Cn % 128 != 0, odd B, partial column tiles
    ((BF16, 3, 32, 40, 160, 640, 2, 3, 1, 1), "WIDE3_16"),
    ((BF16, 3, 32, 32, 80, 160, 1, 3, 1, 1), "WIDE3_16"),
    ((BF16, 3, 24, 40, 80, 320, 1, 3, 1, 1), "WIDE3_8"),
    ((BF16, 11, 20, 20, 80, 1024, 1, 3, 1, 1), "WIDE3_8"),
    ((BF16, 9, 20, 20, 160, 1280, 2, 3, 1, 1), "WIDE3_8"),
    # conv3x3_flat.hip
    ((BF16, 5, 23, 37, 64, 2048, 1, 3, 1, 1), "FLAT"),
    ((BF16, 15, 20, 20, 240, 960, 3, 3, 1, 1), "FLAT"),
    # conv_gemm.hip generic: unpadded (the sparse head's patch convs), grouped ragged, fp32
    ((BF16, 3, 9, 9, 96, 80, 1, 3, 1, 0), "GENERIC"),
    ((BF16, 9, 20, 20, 160, 640, 2, 3, 1, 1), "GENERIC"),
    ((BF16, 5, 7, 7, 64, 48, 1, 5, 2, 2), "GENERIC"),
    ((F32, 3, 13, 11, 24, 40, 1, 3, 1, 1), "GENERIC"),
    ((F32, 3, 20, 24, 128, 80, 1, 1, 1, 0), "GENERIC"),
    ((F32, 2, 9, 9, 64, 96, 2, 3, 2, 0), "GENERIC"),
    # fp32 mode on the tile kernel
    ((F32, 3, 32, 40, 64, 80, 1, 3, 1, 1), "TILE16"),
    ((F32, 2, 24, 24, 128, 48, 1, 3, 1, 1), "TILE8"),
    # conv3x3_small.hip stride 2
    ((BF16, 3, 40, 41, 16, 32, 1, 3, 2, 1), "SMALL_S2"),
    ((BF16, 2, 33, 40, 32, 64, 1, 3, 2, 1), "SMALL_S2"),
    # conv1x1_stream.hip, dense and grouped
    ((BF16, 3, 20, 24, 128, 80, 1, 1, 1, 0), "STREAM1X1"),
    ((BF16, 3, 20, 24, 640, 320, 4, 1, 1, 0), "STREAM1X1"),
]
# y3d_conv2d_fwd_affine_res: the narrow kernel only; the residual is a slice of a wider buffer (rsw != Cout)
RES_CASES = [
    ((BF16, 3, 21, 27, 32, 16, 1, 3, 1, 1), "SMALL"),
    ((BF16, 2, 16, 20, 64, 64, 1, 3, 1, 1), "SMALL"),
    ((BF16, 1, 12, 40, 48, 40, 1, 3, 1, 1), "SMALL"),
]

# the kernel templates behind each route that the case lists must keep reaching
FWD_AFFINE_ROUTES = {"GENERIC", "STREAM1X1", "SMALL", "SMALL_S2", "TILE8", "TILE16", "WIDE3_8", "WIDE3_16", "FLAT"}


def _route(case, epi=EPI_AFFINE):
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    return y3d.lib().conv2d_route(dt, 0, epi, B, H, W, Cin, Cout, g, k, k, s, p)


def _small_variant(case):
    """(LDS row bytes, output-channel tiles) of the conv3x3_small.hip instantiation: conv3x3_small.hip's launch rule"""
    _, _, _, _, Cin, Cout, *_ = case
    return (64 if Cin <= 32 else 128, min(4, -(-Cout // 16)))


def test_case_routes():
    """CPU: every case still takes the route it was written for, and the lists reach every forward-affine kernel.  A heuristic
    change that moves a case elsewhere fails here and names the route that lost its case."""
    for case, want in AFFINE_CASES:
        got = _route(case)
        assert got == ROUTES[want], f"{case} now routes to {ROUTE_NAME.get(got, got)}, not {want}: add a case that reaches {want}"
    for case, want in RES_CASES:
        assert _route(case, EPI_AFFINE_RES) == ROUTES[want], f"affine_res {case}"
    hit = {want for _, want in AFFINE_CASES}
    assert hit == FWD_AFFINE_ROUTES, f"no case reaches {FWD_AFFINE_ROUTES - hit}"
    # sub-variants: both small-kernel row widths x 1-4 channel tiles; fp32 on the tile and generic kernels; groups on the
    # persistent / flat / streaming kernels; the ragged 20-row map on wide3
    small = {_small_variant(c) for c, r in AFFINE_CASES if r == "SMALL"}
    assert small == {(cb, n) for cb in (64, 128) for n in (1, 2, 3, 4)}, small
    assert {r for c, r in AFFINE_CASES if c[0] == F32} >= {"GENERIC", "TILE8", "TILE16"}
    for r in ("WIDE3_16", "WIDE3_8", "FLAT", "STREAM1X1", "GENERIC", "TILE8"):
        assert any(c[6] > 1 for c, rr in AFFINE_CASES if rr == r), f"no grouped case on {r}"
    assert any(c[2] % 8 for c, r in AFFINE_CASES if r == "WIDE3_8"), "no ragged-height case on wide3"
    assert any((c[5] // c[6]) % 128 for c, r in AFFINE_CASES if r in ("WIDE3_16", "WIDE3_8", "FLAT")), "no partial channel tile"


# ---------------------------------------------------------------------------------------------------------------------------------


def _sparse_int(shape, gen, density):
    u = torch.rand(shape, generator=gen)
    return (u < density / 2).float() - (u > 1 - density / 2).float()


def _epilogue_consts(Cout, gen):
    scale = 0.05 + 1.95 * torch.rand(Cout, generator=gen)
    shift = torch.randn(Cout, generator=gen)
    return scale.float(), shift.float()


def _sample_pixels(B, Ho, Wo, gen, full):
    """(b, h, w) index vectors: every pixel (full) or all pixels of the first and last image, the tile seams (rows / columns at
    multiples of 8 and 16 and their predecessors, the last row / column) of two inner images, and a seeded random set"""
    if full:
        b, h, w = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
        return b.reshape(-1), h.reshape(-1), w.reshape(-1)
    parts = []
    hh, ww = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    hh, ww = hh.reshape(-1), ww.reshape(-1)
    for b in sorted({0, B - 1}):
        parts.append(torch.stack((torch.full_like(hh, b), hh, ww)))
    seam = ((hh % 8 == 0) | (hh % 8 == 7) | (hh == Ho - 1) | (ww % 16 == 0) | (ww % 16 == 15) | (ww == Wo - 1))
    for b in sorted({min(1, B - 1), B // 2} - {0, B - 1}):
        parts.append(torch.stack((torch.full_like(hh[seam], b), hh[seam], ww[seam])))
    n = 2048
    parts.append(torch.stack((torch.randint(0, B, (n,), generator=gen), torch.randint(0, Ho, (n,), generator=gen),
                              torch.randint(0, Wo, (n,), generator=gen))))
    idx = torch.unique(torch.cat(parts, 1), dim=1)
    return idx[0], idx[1], idx[2]


def _exact_acc(xd, wd, g, k, s, p, b, h, w):
    """exact conv accumulators at the pixels (b, h, w): fp64 patch . weight dot products.  xd: (B, H, W, Cin) fp32 device,
    wd: (Cout, Cin/g, k, k) fp32 device -> (N, Cout) fp64"""
    B, H, W, Cin = xd.shape
    Cout, Cg = wd.shape[0], Cin // g
    xp = torch.zeros(B, H + 2 * p, W + 2 * p, Cin, dtype=torch.float32, device=xd.device)
    xp[:, p:p + H, p:p + W] = xd
    b, h, w = b.to(xd.device), h.to(xd.device), w.to(xd.device)
    r = torch.arange(k, device=xd.device)
    rows = (h * s)[:, None, None] + r[None, :, None]
    cols = (w * s)[:, None, None] + r[None, None, :]
    patch = xp[b[:, None, None], rows, cols]  # (N, k, k, Cin)
    Cn = Cout // g
    out = []
    for gi in range(g):
        pg = patch[..., gi * Cg:(gi + 1) * Cg].reshape(len(b), -1).double()
        wg = wd[gi * Cn:(gi + 1) * Cn].permute(0, 2, 3, 1).reshape(Cn, -1).double()
        out.append(pg @ wg.T)
    return torch.cat(out, 1)


def bound(dt, ref, t, res, u, prod, shift):
    """the module docstring's bound; prod = acc * scale, shift broadcast against it"""
    ua = 2.0 ** -22 * (prod.abs() + shift.abs())
    if dt == BF16:
        return 2.0 ** -8 * ref.abs() + 2.0 ** -20 * (t.abs() + res.abs()) + ua + 1e-30
    return 2.0 ** -22 * ref.abs() + 2.0 ** -22 * (4 + u.abs()) * t.abs() + 2.0 ** -23 * res.abs() + ua + 1e-30


def run_affine(case, act, seed, res=False, full=True):
    """launch y3d_conv2d_fwd_affine(_res) at `case` and compare (a sample of) its output with the fp64 reference; returns the route"""
    dt, B, H, W, Cin, Cout, g, k, s, p = case
    L, st = y3d.lib(), ops.stream()
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gen = torch.Generator().manual_seed(seed)
    K = k * k * (Cin // g)
    density = min(0.5, max(0.06, 6.0 / math.sqrt(K)))  # a few tens of non-zero products per output
    gd = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.rand((B, H, W, Cin), generator=gd, device=DEV)
    xd = (u < density / 2).float() - (u > 1 - density / 2).float()
    del u
    wd = _sparse_int((Cout, Cin // g, k, k), gen, density).to(DEV)
    scale, shift = _epilogue_consts(Cout, gen)
    sd, hd = scale.to(DEV), shift.to(DEV)
    xin = xd.to(tdt)
    wp = torch.empty(Cout * K, dtype=tdt, device=DEV)
    L.pack_weight_fwd(dt, wd.data_ptr(), wp.data_ptr(), Cout, Cin // g, Cin // g, k, k, st)
    buf = torch.full((B, Ho, Wo, Cout + EXTRA), float("nan"), dtype=tdt, device=DEV)
    y = buf[..., OFF:OFF + Cout]
    ysw = buf.stride(2)
    sb, sh, sw = xin.stride(0), xin.stride(1), xin.stride(2)
    if res:
        rbuf = torch.full((B, Ho, Wo, Cout + 16), float("nan"), dtype=tdt, device=DEV)
        rv = rbuf[..., 8:8 + Cout]
        rv.copy_(torch.randn((B, Ho, Wo, Cout), generator=gd, device=DEV).to(tdt))
        L.conv2d_fwd_affine_res(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin, wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), act,
                                rv.data_ptr(), rbuf.stride(2), y.data_ptr(), ysw, Ho, Wo, Cout, g, k, k, s, p, st)
    else:
        L.conv2d_fwd_affine(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin, wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), act,
                            y.data_ptr(), ysw, Ho, Wo, Cout, g, k, k, s, p, st)
    torch.cuda.synchronize()
    # nothing outside the slot was written
    assert bool(buf[..., :OFF].isnan().all()) and bool(buf[..., OFF + Cout:].isnan().all()), "a store left the output slot"
    b, h, w = _sample_pixels(B, Ho, Wo, gen, full)
    acc = _exact_acc(xd, wd, g, k, s, p, b, h, w).cpu()
    assert float(acc.abs().max()) < 2 ** 24
    z = y[b.to(DEV), h.to(DEV), w.to(DEV)].double().cpu()
    uu = acc * scale.double() + shift.double()
    t = uu * torch.sigmoid(uu) if act else uu
    r64 = rv[b.to(DEV), h.to(DEV), w.to(DEV)].double().cpu() if res else torch.zeros_like(t)
    ref = t + r64
    err = (z - ref).abs()
    tol = bound(dt, ref, t, r64, uu, acc * scale.double(), shift.double().expand_as(uu))
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.nonzero()[0][0])
        j = int(bad[i].nonzero()[0][0])
        raise AssertionError(f"{case} act={act} res={res} route {ROUTE_NAME.get(_route(case), '?')}: {int(bad.sum())} of {bad.numel()} "
                             f"outputs outside the bound; first at pixel {(int(b[i]), int(h[i]), int(w[i]))} channel {j}: "
                             f"z={float(z[i, j])!r} ref={float(ref[i, j])!r} acc={float(acc[i, j])} tol={float(tol[i, j]):.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("case,route", AFFINE_CASES, ids=[f"{r}-" + "x".join(map(str, c)) for c, r in AFFINE_CASES])
def test_fwd_affine_route_against_fp64(case, route, act):
    run_affine(case, act, seed=sum(case) + 7 * act)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("case,route", RES_CASES, ids=[f"{r}-" + "x".join(map(str, c)) for c, r in RES_CASES])
def test_fwd_affine_res_against_fp64(case, route, act):
    run_affine(case, act, seed=sum(case) + 3 * act, res=True)


# ---- the eval forward's own geometries -------------------------------------------------------------------------------------------


class _Recorder:
    """stands in for ops.TIMER: records the key of every bracketed launch, times nothing"""

    def __init__(self):
        self.keys = {}

    def bracket(self, key, fn):
        self.keys.setdefault(key, None)
        return fn()


@pytest.fixture(scope="module")
def eval_geometries():
    """distinct conv_eval keys (dt, B, H, W, Cin, Cout, k, s, g, p) of one eager S-3D eval forward at B = 32, 640 x 640"""
    old = y3d.compute_dtype()
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").to(DEV).train()
    if hasattr(model.model[-1], "restack"):
        model.model[-1].restack()
    model.eval()
    img = torch.rand(32, 3, 640, 640, generator=torch.Generator(device=DEV).manual_seed(0), device=DEV)
    rec, prev = _Recorder(), ops.TIMER
    ops.TIMER = rec
    try:
        with torch.no_grad():
            model(img)
        torch.cuda.synchronize()
    finally:
        ops.TIMER = prev
        if old is not None:
            y3d.set_compute_dtype(old)
    del model, img
    torch.cuda.empty_cache()
    # Cin = 3 is the stem's own kernel (stem_conv_eval), not the conv epilogues
    return sorted({key[1:] for key in rec.keys if key[0] == "conv_eval" and key[5] != 3})


@pytest.mark.gpu
def test_fwd_affine_at_every_eval_geometry(eval_geometries):
    """each distinct conv of the S-3D eval forward, at its exact geometry and batch, on a sample of output pixels"""
    geos = eval_geometries
    assert len(geos) >= 20, geos
    # the sparse head's patch convolutions: unpadded 3x3 on 5x5 and 3x3 maps, 1 600 patches
    assert any(p == 0 and k == 3 and H in (5, 3) for (_, B, H, W, Cin, Cout, k, s, g, p) in geos), geos
    seen = set()
    for i, (dt, B, H, W, Cin, Cout, k, s, g, p) in enumerate(geos):
        case = (dt, B, H, W, Cin, Cout, g, k, s, p)
        seen.add(ROUTE_NAME.get(_route(case)))
        run_affine(case, act=1, seed=1000 + i, full=False)
    print("eval routes:", sorted(seen))
