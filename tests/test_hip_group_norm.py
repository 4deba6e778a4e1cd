"""GPU: the GroupNorm kernels of csrc/group_norm.hip (ops.gn_forward / ops.gn_backward) alone, against the float64 restatement of
tests/depth_predictor_ref.py (gn_fwd / gn_bwd), plus the column sum and the depth expectation of the same file.

Bound.  The kernels compute in float32 whatever the maps' dtype, so the yardstick of a case is the restatement itself run in float32 on the
same inputs against its float64 run (max |a - ref| / max |ref| per result).  One such run can be lucky, so the yardstick is never taken
below what float32 sums of this length carry in ANY order: rounding errors of a sum of N terms add up like a random walk, sqrt(N) unit
roundoffs (2^-24) of the result's scale (the worst case is N), and no result here sums more than N = 4 B HW terms (a group's statistics
over one sample: 4 HW; a parameter gradient: B HW).  A kernel may sum in another, equally valid order: four times the yardstick, as
tests/test_hip_fgdm_loss.py.  A result stored in bfloat16 (out, dy) adds the half ulp of
its final rounding, element by element.  Sources, outputs and gradients are pixel-strided slices of sentinel-filled arenas whose other
elements must come back untouched."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

import depth_predictor_ref as R
import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import Y3DError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV, C, G = "cuda", 128, 32
CHUNK = 256  # pixels per block of the kernels: one chunk, one chunk +- 1, several chunks
SHAPES = ((1, 1), (5, 7), (16, 16), (15, 17), (1, 257), (24, 80))
SENTINEL, GUARD, PITCH = 77.0, 3, C + 8


def bf16_half_ulp(v):
    _, e = np.frexp(np.abs(v))
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 9))


class Arena:
    """a (B, C, H, W) pixel-strided slice (pixel stride PITCH) of a sentinel-filled buffer with GUARD pixels before and after"""

    def __init__(self, B, H, W, dtype, value=None, pitch=PITCH, c=C):
        self.buf = torch.full(((B * H * W + 2 * GUARD) * pitch,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf.as_strided((B, c, H, W), (H * W * pitch, 1, W * pitch, pitch), GUARD * pitch)
        if value is not None:
            self.t.copy_(value.to(DEV))
        self.before = self.buf.clone()

    def untouched_outside(self, written):
        """every element outside the slice is what it was; `written`: the slice itself was (over)written"""
        now, was = self.buf.clone(), self.before.clone()
        mask = torch.zeros_like(self.buf, dtype=torch.bool)
        mask.as_strided(self.t.shape, self.t.stride(), self.t.storage_offset()).fill_(True)
        ok = torch.equal(now[~mask], was[~mask])
        return ok and (written or torch.equal(now[mask], was[mask]))


def draw(B, H, W, nsrc, dtype, seed, bias=None):
    g = torch.Generator().manual_seed(seed)
    rnd = (lambda t: t.bfloat16().float()) if dtype == torch.bfloat16 else (lambda t: t)
    ys = [rnd(torch.randn(B, C, H, W, generator=g) * (1 + i)) for i in range(nsrc)]
    bs = [torch.randn(C, generator=g) if bias is None else torch.full((C,), float(bias)) for _ in range(nsrc)]
    gammas = [torch.rand(C, generator=g) + 0.5 for _ in range(nsrc)]
    betas = [torch.rand(C, generator=g) - 0.5 for _ in range(nsrc)]
    dz = rnd(torch.randn(B, C, H, W, generator=g))
    return ys, bs, gammas, betas, dz


def restated(ys, bs, gammas, betas, dz, scale, relu, eps, dt):
    a = [[t.to(dt) for t in l] for l in (ys, bs, gammas, betas)]
    out, cache = R.gn_fwd(*a, eps, scale, relu)
    back = R.gn_bwd(dz.to(dt), a[2], cache, scale, relu)
    res = {"out": out}
    for i, (dy, dg, db, dbc) in enumerate(back):
        res.update({f"dy{i}": dy, f"dgamma{i}": dg, f"dbeta{i}": db, f"dbconv{i}": dbc})
    return {k: v.double().numpy() for k, v in res.items()}


def device(ys, bs, gammas, betas, dz, scale, relu, eps, dtype):
    B, _, H, W = ys[0].shape
    src = [Arena(B, H, W, dtype, y) for y in ys]
    out, dza = Arena(B, H, W, dtype), Arena(B, H, W, dtype, dz)
    dys = [Arena(B, H, W, dtype) for _ in ys]
    vec = [[v.to(DEV) for v in l] for l in (bs, gammas, betas)]
    o, stats = ops.gn_forward([a.t for a in src], *vec, eps=eps, scale=scale, relu=relu, out=out.t)
    _, dg, db, dbc = ops.gn_backward([a.t for a in src], *vec, stats, dza.t, scale=scale, relu=relu, dys=[a.t for a in dys])
    torch.cuda.synchronize()
    assert o.data_ptr() == out.t.data_ptr()
    assert all(a.untouched_outside(False) for a in src + [dza]), "a source or dz was written"
    assert out.untouched_outside(True) and all(a.untouched_outside(True) for a in dys), "written outside the output slice"
    res = {"out": out.t}
    for i in range(len(ys)):
        res.update({f"dy{i}": dys[i].t, f"dgamma{i}": dg[i], f"dbeta{i}": db[i], f"dbconv{i}": dbc[i]})
    return {k: v.float().cpu().double().numpy() for k, v in res.items()}, stats


def check(got, ref, yard, dtype, what, nterms):
    worst = 0.0
    for k, r in ref.items():
        y = max(R.rel_max(yard[k], r), nterms ** 0.5 * 2.0 ** -24)
        tol = 4 * y * np.abs(r).max()
        if dtype == torch.bfloat16 and (k == "out" or k.startswith("dy")):
            tol = tol + bf16_half_ulp(r)
        err = np.abs(got[k] - r)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert np.isfinite(got[k]).all() and (err <= tol).all(), f"{what} {k}: off by {float((err - tol).max()):.3e} beyond the bound ({y:.2e} yardstick)"
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_and_backward(B, hw, dtype):
    for nsrc, relu in ((1, False), (1, True), (3, False), (3, True)):
        scale = 1.0 if nsrc == 1 else 1.0 / 3.0
        args = draw(B, *hw, nsrc, dtype, seed=100 * B + hw[0] + 7 * nsrc + relu)
        ref = restated(*args, scale, relu, R.EPS, torch.float64)
        yard = restated(*args, scale, relu, R.EPS, torch.float32)
        got, _ = device(*args, scale, relu, R.EPS, dtype)
        w = check(got, ref, yard, dtype, f"nsrc {nsrc} relu {relu}", 4 * B * hw[0] * hw[1])
        print(f"B {B} {hw} {dtype} nsrc {nsrc} relu {relu}: worst error / bound {w:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_large_mean(dtype):
    """y ~ N(0, 1), conv bias 1000: E[x^2] - E[x]^2 in float32 would lose the variance (1 against 10^6 at 2^-24) entirely"""
    for nsrc, relu in ((1, True), (3, False)):
        scale = 1.0 if nsrc == 1 else 1.0 / 3.0
        args = draw(3, 15, 17, nsrc, dtype, seed=5, bias=1000.0)
        ref = restated(*args, scale, relu, R.EPS, torch.float64)
        yard = restated(*args, scale, relu, R.EPS, torch.float32)
        got, stats = device(*args, scale, relu, R.EPS, dtype)
        w = check(got, ref, yard, dtype, f"large mean nsrc {nsrc}", 4 * 3 * 15 * 17)
        rstd = stats.view(nsrc, 3, G, 2)[..., 1].cpu().numpy()
        print(f"large mean {dtype} nsrc {nsrc}: worst error / bound {w:.3f}, rstd in [{rstd.min():.4f}, {rstd.max():.4f}]")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(5, 7), (15, 17), (24, 80)], ids=["35", "255", "1920"])
def test_exact(hw, dtype):
    """values +-1, two of each sign in every pixel's group: mean 0 and variance 1 exactly in every chunk; eps = 0, small integer gamma /
    beta, scale 1: every result is a small integer, compared bit for bit"""
    B, (H, W) = 2, hw
    g = torch.Generator().manual_seed(3)
    for nsrc, relu in ((1, False), (1, True), (3, True)):
        ys = []
        for i in range(nsrc):
            pat = torch.tensor([[1, 1, -1, -1], [1, -1, 1, -1], [-1, 1, 1, -1]], dtype=torch.float32)[torch.randint(0, 3, (B, G, H, W), generator=g)]
            sign = torch.randint(0, 2, (B, G, H, W, 1), generator=g).float() * 2 - 1
            ys.append((pat * sign).permute(0, 1, 4, 2, 3).reshape(B, C, H, W))
        bs = [torch.zeros(C) for _ in range(nsrc)]
        gammas = [torch.randint(-3, 4, (C,), generator=g).float() for _ in range(nsrc)]
        betas = [torch.randint(-2, 3, (C,), generator=g).float() for _ in range(nsrc)]
        dz = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
        ref, _ = R.gn_fwd([y.double() for y in ys], [b.double() for b in bs], [v.double() for v in gammas], [v.double() for v in betas], 0.0, 1.0, relu)
        src = [Arena(B, H, W, dtype, y) for y in ys]
        vec = [[v.to(DEV) for v in l] for l in (bs, gammas, betas)]
        out, stats = ops.gn_forward([a.t for a in src], *vec, eps=0.0, scale=1.0, relu=relu)
        _, dg, db, _ = ops.gn_backward([a.t for a in src], *vec, stats, ops.to_nhwc(dz.to(DEV), dtype, dense=True), scale=1.0, relu=relu)
        st = stats.view(nsrc, B, G, 2).cpu()
        assert torch.equal(st[..., 0], torch.zeros(nsrc, B, G)) and torch.equal(st[..., 1], torch.ones(nsrc, B, G)), "mean 0, rstd 1 exactly"
        assert torch.equal(out.float().cpu(), ref.float()), f"nsrc {nsrc} relu {relu}"
        dzh = dz.double() * ((ref > 0).double() if relu else 1.0)
        for i in range(nsrc):
            assert torch.equal(dg[i].cpu().double(), (dzh * ys[i].double()).sum((0, 2, 3))) and torch.equal(db[i].cpu().double(), dzh.sum((0, 2, 3)))


def test_all_negative_relu_gives_plus_zero():
    ys, bs, gammas, betas, dz = draw(2, 15, 17, 1, torch.float32, seed=8)
    gammas = [-gammas[0]]  # a zero times a negative gamma is -0 before the kernel's last add
    betas = [torch.full((C,), -100.0)]
    for dtype in (torch.float32, torch.bfloat16):
        src = ops.to_nhwc(ys[0].to(DEV), dtype, dense=True)
        vec = [[v.to(DEV) for v in l] for l in (bs, gammas, betas)]
        out, stats = ops.gn_forward([src], *vec, relu=True)
        dys, dg, db, dbc = ops.gn_backward([src], *vec, stats, ops.to_nhwc(dz.to(DEV), dtype, dense=True), relu=True)
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        assert not out.contiguous().view(bits).any() and not dys[0].contiguous().view(bits).any(), "exactly +0"
        assert not dg.view(torch.int32).any() and not db.view(torch.int32).any() and not (dbc != 0).any()


def test_same_bits_on_two_runs():
    args = draw(3, 24, 80, 3, torch.bfloat16, seed=2)
    a, sa = device(*args, 1.0 / 3.0, True, R.EPS, torch.bfloat16)
    b, sb = device(*args, 1.0 / 3.0, True, R.EPS, torch.bfloat16)
    assert torch.equal(sa, sb) and all(np.array_equal(a[k], b[k]) for k in a)


def test_refused_arguments():
    ys, bs, gammas, betas, dz = draw(1, 5, 7, 1, torch.float32, seed=1)
    with pytest.raises(Y3DError, match="no CPU fallback"):  # a host pointer never reaches the library
        ops.gn_forward(ys, bs, gammas, betas)
    dev = lambda l: [v.to(DEV) for v in l]  # noqa: E731
    y = ops.to_nhwc(ys[0].to(DEV), torch.float32, dense=True)
    with pytest.raises(Y3DError, match="no CPU fallback"):
        ops.gn_forward([y], bs, dev(gammas), dev(betas))
    with pytest.raises(Y3DError, match=r"only GroupNorm\(32 groups, 128 channels\)"):
        ops.gn_forward([y], dev(bs), dev(gammas), dev(betas), groups=16)
    y64 = ops.to_nhwc(torch.randn(1, 64, 5, 7, device=DEV), torch.float32, dense=True)
    v64 = [torch.ones(64, device=DEV)]
    with pytest.raises(Y3DError, match=r"only GroupNorm\(32 groups, 128 channels\)"):
        ops.gn_forward([y64], v64, v64, v64)
    y132 = Arena(1, 5, 7, torch.bfloat16, torch.randn(1, 132, 5, 7), pitch=136, c=132).t
    v132 = [torch.ones(132, device=DEV)]
    with pytest.raises(Y3DError, match="16-byte chunks"):
        ops.gn_forward([y132], v132, v132, v132)
    with pytest.raises(Y3DError, match="nsrc = 2"):
        ops.gn_forward([y, y], dev(bs) * 2, dev(gammas) * 2, dev(betas) * 2)
    with pytest.raises(Y3DError, match="pixel-dense"):
        ops.gn_forward([torch.randn(1, 128, 5, 7, device=DEV)], dev(bs), dev(gammas), dev(betas))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_colsum_and_depth_expect(dtype):
    """the classifier's bias gradient (two-stage column sum, several blocks) and weighted_depth (81 bins in an 88-channel row)"""
    g = torch.Generator().manual_seed(4)
    B, h, w = 3, 24, 80
    x = torch.randn(B, 88, h, w, generator=g)
    x = x.bfloat16().float() if dtype == torch.bfloat16 else x
    xd = ops.to_nhwc(x.to(DEV), dtype, dense=True)
    L, M = ops.lib(), B * h * w
    part = torch.empty(L.colsum_blocks(M) * 88, dtype=torch.float32, device=DEV)
    out = torch.empty(88, dtype=torch.float32, device=DEV)
    L.colsum(ops.code(dtype), xd.data_ptr(), 88, M, 88, part.data_ptr(), out.data_ptr(), ops.stream())
    ref = x.double().sum((0, 2, 3))
    yard = max(R.rel_max(x.sum((0, 2, 3)), ref), M ** 0.5 * 2.0 ** -24)  # (the module docstring's floor for a sum of M terms)
    assert L.colsum_blocks(M) > 1 and R.rel_max(out.cpu(), ref) <= 4 * yard
    bins = R.bin_values()
    wd = ops.depth_expect(xd[:, :81], bins.to(DEV))
    refw = (x[:, :81].double().softmax(1) * bins.double().view(1, -1, 1, 1)).sum(1)
    yard = max(R.rel_max((x[:, :81].softmax(1) * bins.view(1, -1, 1, 1)).sum(1), refw), 2.0 ** -23)
    assert wd.shape == (B, h, w) and wd.dtype == torch.float32 and R.rel_max(wd.cpu(), refw) <= 4 * yard
    with pytest.raises(Y3DError, match="no CPU fallback"):
        ops.depth_expect(x[:, :81], bins)
