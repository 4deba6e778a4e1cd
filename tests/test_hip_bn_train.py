"""The BatchNorm training kernels of bn_act.hip against fp64: bn_finalize, bn_act_fwd, bn_act_bwd_reduce -> bn_bwd_finalize ->
bn_act_bwd_apply, colsum_partials, and conv BatchNorm partials through bn_finalize.

Bounds (u = 2^-24, fp32 unit roundoff; every reference is fp64 from the exact fp32 / bf16 inputs the kernel read):
* storage: a bf16 result is one round-to-nearest-even of the fp32 value v: |z - v| <= half an ulp of v = 2^-9 * 2^(e+1) for
  2^e <= |v| < 2^(e+1) (a flat 2^-9 |v| is not an RNE bound: 1 + 2^-8 rounds to 1, an error of 2^-8 |v|).  A truncating store misses
  it by up to a whole ulp.  fp32 results: u |v|.
* u = y * scale + shift (+ res): FMA contraction or a separate multiply and add, so 3u (|y scale| + |shift| + |res|) covers both;
  silu through v_exp_f32 / v_rcp_f32 adds 2^-21 (4 + |u|) |t| (t = silu(u)) and propagates the u error with silu' <= 1.1;
  silu'(u) = s (1 + u (1 - s)) from the same sigmoid: 2^-21 (2 + |u|)^2.
* fp32 sums of n terms (partial rows, in any order): (n - 1) u sum |term|; the fp64 folds add nblk 2^-52 sum |partial|.
* bn_finalize: mean, invstd from fp64 sums of the fp32 partials, each rounded once to fp32 (u); the variance q/n - mean^2 loses
  (mean^2 + var) / var of its relative accuracy to cancellation, so every fold error is scaled by that term; scale = gamma * invstd
  (one rounding); shift = beta - mean * scale and the running statistics (momentum, unbiased variance) are fp32 expressions of two
  to three operations: 3u of their terms.  End to end from conv partials the Sum y^2 error of a partial row of n pixels,
  (n - 1) u Sum y^2, enters the variance as (n - 1) u (mean^2 + var) / var relative."""
import math

import pytest
import torch

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402
from yolov10_3d_amd._lib import BF16, F32  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24


def _half_ulp_bf16(v):
    a = v.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.exp2(e - 8), torch.zeros_like(a)) + 2.0 ** -133


def _store_tol(dt, ref, e):
    """|stored - ref| bound for a result whose fp32 value is within e of ref"""
    if dt == BF16:
        return _half_ulp_bf16(ref.abs() + e) + e + 1e-30
    return U * (ref.abs() + e) + e + 1e-30


def _check(what, got, ref, tol):
    bad = ~((got - ref).abs() <= tol)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at flat index {i}: got "
                             f"{float(got.reshape(-1)[i])!r} expected {float(ref.reshape(-1)[i])!r} bound {float(tol.reshape(-1)[i]):.3g}")


def _slot(P, C, pitch, dt, fill):
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    buf = torch.full((P, pitch), fill, dtype=tdt, device=DEV)
    return buf, buf[:, 8:8 + C]


# ---- bn_finalize ---------------------------------------------------------------------------------------------------------------


def _finalize_ref(part, count, gamma, beta, eps, mom, rm, rv):
    """fp64 reference and bounds from the same fp32 partials -> dict name -> (ref, tol)"""
    p = part.double()
    nblk = p.shape[0]
    s, q = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    es = (nblk + 32) * 2.0 ** -52 * p[:, :, 0].abs().sum(0)
    eq = (nblk + 32) * 2.0 ** -52 * p[:, :, 1].abs().sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0)
    em = es / count
    ev = eq / count + 2 * mean.abs() * em + 2.0 ** -52 * (q / count + mean * mean)  # fp64 cancellation: (mean^2 + var) / var amplifies
    invstd = 1.0 / torch.sqrt(var + eps)
    e_is = U * invstd + 0.5 * invstd ** 3 * ev
    g, b = gamma.double(), beta.double()
    scale = g * invstd
    e_sc = U * scale.abs() + g.abs() * e_is
    shift = b - mean * scale
    e_sh = 3 * U * (b.abs() + (mean * scale).abs()) + mean.abs() * e_sc + scale.abs() * (em + U * mean.abs())
    unb = var * count / (count - 1)
    rm_new = (1 - mom) * rm.double() + mom * mean
    rv_new = (1 - mom) * rv.double() + mom * unb
    e_rm = 3 * U * ((1 - mom) * rm.double().abs() + mom * mean.abs()) + mom * (em + U * mean.abs()) + 1e-30
    e_rv = 3 * U * ((1 - mom) * rv.double().abs() + mom * unb) + mom * (count / (count - 1)) * ev + mom * U * unb + 1e-30
    return {"mean": (mean, U * mean.abs() + em + 1e-30), "invstd": (invstd, e_is), "scale": (scale, e_sc), "shift": (shift, e_sh),
            "running_mean": (rm_new, e_rm), "running_var": (rv_new, e_rv)}


def _run_finalize(part, count, gamma, beta, eps, mom, rm, rv):
    L, st = y3d.lib(), ops.stream()
    nblk, C, _ = part.shape
    out = torch.full((4, C), float("nan"), device=DEV)
    rm_k, rv_k = rm.clone(), rv.clone()
    L.bn_finalize(part.data_ptr(), nblk, C, count, gamma.data_ptr(), beta.data_ptr(), eps, mom, rm_k.data_ptr(), rv_k.data_ptr(),
                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), st)
    torch.cuda.synchronize()
    return {"mean": out[0], "invstd": out[1], "scale": out[2], "shift": out[3], "running_mean": rm_k, "running_var": rv_k}


@pytest.mark.gpu
@pytest.mark.parametrize("nblk", [7, 32, 77, 128, 129, 517])
def test_bn_finalize_against_fp64(nblk):
    """partials of P = nblk * 100 values per channel; channel 0 constant (variance 0, clamped), the others with |mean| / std up to 10"""
    C, rows = 72, 100
    g = torch.Generator(device=DEV).manual_seed(nblk)
    mu = torch.randn(C, generator=g, device=DEV) * 4
    sd = torch.rand(C, generator=g, device=DEV) + 0.4
    mu[1], sd[1] = 10.0, 1.0  # |mean| / std = 10
    y = torch.randn(nblk * rows, C, generator=g, device=DEV) * sd + mu
    y[:, 0] = 3.0  # constant: every partial (300, 900) is exact, var = 0 exactly
    yb = y.view(nblk, rows, C).double()
    part = torch.stack((yb.sum(1), (yb * yb).sum(1)), 2).float().contiguous()
    count = nblk * rows
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV)
    rm, rv = torch.randn(C, generator=g, device=DEV), torch.rand(C, generator=g, device=DEV) + 0.5
    got = _run_finalize(part, count, gamma, beta, 1e-3, 0.03, rm, rv)
    ref = _finalize_ref(part, count, gamma, beta, 1e-3, 0.03, rm, rv)
    for k, (r, t) in ref.items():
        _check(f"bn_finalize nblk={nblk} {k}", got[k].double(), r, t)
    assert float(got["invstd"][0]) == pytest.approx(1 / math.sqrt(1e-3), rel=2 ** -22), "constant channel: variance must clamp to 0"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(1, 3, 20, 24, 128, 80, 1, 1, 1, 0), (1, 4, 32, 32, 128, 128, 1, 3, 1, 1),
                                  (1, 3, 9, 9, 96, 80, 1, 3, 1, 0)])
def test_conv_partials_through_bn_finalize(case):
    """y3d_conv2d_fwd partials -> bn_finalize against the fp64 statistics of the stored y (integer operands; an offset on x makes
    |mean| / std large, so the cancellation term (mean^2 + var) / var is exercised, not hidden)"""
    import test_hip_train_convs as TC

    dt, B, H, W, Cin, Cout, g, k, s, p = case
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = TC._out_hw(case)
    gd = torch.Generator(device=DEV).manual_seed(sum(case))
    a = TC._amp(k * k * Cin)
    xd = TC._ints((B, H, W, Cin), a, 1.0, gd).abs()  # x >= 0 and w with a per-channel sign bias: a mean several stds from 0
    wd = TC._ints((Cout, Cin, k, k), a, 1.0, gd) + 1
    assert float(xd.abs().max()) * float(wd.abs().reshape(Cout, -1).sum(1).max()) < 2 ** 24
    xin = xd.to(torch.bfloat16)
    wp = torch.empty(Cout * k * k * Cin, dtype=torch.bfloat16, device=DEV)
    L.pack_weight_fwd(dt, wd.data_ptr(), wp.data_ptr(), Cout, Cin, Cin, k, k, st)
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=DEV)
    rows = L.conv2d_stat_rows(dt, B, H, W, Cin, Cout, g, k, k, s, p)
    part = torch.full((rows, Cout, 2), float("nan"), device=DEV)
    L.conv2d_fwd(dt, xin.data_ptr(), *xin.stride()[:3], B, H, W, Cin, wp.data_ptr(), None, y.data_ptr(), Cout, Ho, Wo, Cout, g, k, k, s, p,
                 part.data_ptr(), st)
    C, count = Cout, B * Ho * Wo
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    got = _run_finalize(part, count, gamma, beta, 1e-3, 0.1, rm, rv)
    ys = y.double().reshape(-1, C)
    mean = ys.mean(0)
    var = ys.var(0, unbiased=False)
    route = TC._rname(TC.FWD, case)
    n = TC._n_max(route, case, rows)
    cancel = (mean * mean + var) / var
    assert float(cancel.max()) > 4, "the case should exercise the cancellation term"
    ev = (n - 1) * U * (1 + 2.0 ** -10) * (mean * mean + var) + 2.0 ** -44 * (mean * mean + var)
    invstd = 1 / torch.sqrt(var + 1e-3)
    _check(f"conv {route} {case} -> bn_finalize mean", got["mean"].double(), mean, U * mean.abs() + 1e-30)
    _check(f"conv {route} {case} -> bn_finalize invstd (cancellation (mean^2+var)/var up to {float(cancel.max()):.3g})",
           got["invstd"].double(), invstd, U * invstd + 0.5 * invstd ** 3 * ev)


# ---- bn_act_fwd ------------------------------------------------------------------------------------------------------------------


def _fwd_ref(y, sc, sh, act, res_mode, r):
    """fp64 u, t, z and the fp32 error bound of z (module docstring)"""
    ysc = y * sc
    u = ysc + sh + (r if res_mode == 2 else 0)
    eu = 3 * U * (ysc.abs() + sh.abs() + (r.abs() if res_mode == 2 else 0))
    if act:
        t = u * torch.sigmoid(u)
        et = 1.1 * eu + 2.0 ** -21 * (4 + u.abs()) * t.abs()
    else:
        t, et = u, eu
    z = t + (r if res_mode == 1 else 0)
    ez = et + (U * (t.abs() + r.abs()) if res_mode == 1 else 0)
    return u, z, ez


def _bn_inputs(dt, P, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    y = (torch.randn(P, C, generator=g, device=DEV) * 3 + 1).to(tdt)
    r = torch.randn(P, C, generator=g, device=DEV).to(tdt)
    sc = (torch.rand(C, generator=g, device=DEV) * 2 - 0.5)
    sh = torch.randn(C, generator=g, device=DEV)
    return y, r, sc, sh, g


def _run_fwd(dt, y, r, sc, sh, act, res_mode, P, C):
    L, st = y3d.lib(), ops.stream()
    ybuf, yv = _slot(P, C, C + 16, dt, float("nan"))
    yv.copy_(y)
    rbuf, rv = _slot(P, C, C + 24, dt, float("nan"))
    rv.copy_(r)
    zbuf, zv = _slot(P, C, C + 32, dt, float("nan"))
    L.bn_act_fwd(dt, yv.data_ptr(), ybuf.stride(0), sc.data_ptr(), sh.data_ptr(), act, res_mode, rv.data_ptr() if res_mode else None,
                 rbuf.stride(0), zv.data_ptr(), zbuf.stride(0), P, C, st)
    torch.cuda.synchronize()
    assert bool(zbuf[:, :8].isnan().all()) and bool(zbuf[:, 8 + C:].isnan().all()), "bn_act_fwd: a store left the z slot"
    return zv


BN_C = [32, 96, 512, 640, 1152, 2048]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("C", BN_C)
def test_bn_act_fwd_against_fp64(dt, C):
    """act 0 / 1 x res_mode 0 / 1 / 2, ragged P (one under 64), strided y / res / z, z in a NaN-filled wider buffer"""
    for P in (37, 1000 + C // 8):
        y, r, sc, sh, _ = _bn_inputs(dt, P, C, C + P + dt)
        for act in (0, 1):
            for res_mode in (0, 1, 2):
                z = _run_fwd(dt, y, r, sc, sh, act, res_mode, P, C)
                _, zr, ez = _fwd_ref(y.double(), sc.double(), sh.double(), act, res_mode, r.double())
                _check(f"bn_act_fwd dt={dt} C={C} P={P} act={act} res_mode={res_mode}", z.double(), zr, _store_tol(dt, zr, ez))


# ---- backward --------------------------------------------------------------------------------------------------------------------


def _bwd_case(dt, P, C, act, res_mode, train, seed, accumulate=0):
    """bn_act_bwd_reduce -> bn_bwd_finalize -> bn_act_bwd_apply against the fp64 backward of act(BN(y)) (+res) with the mean / invstd
    passed in; -> the outputs for the wide-slab comparison"""
    L, st = y3d.lib(), ops.stream()
    y, r, _, _, g = _bn_inputs(dt, P, C, seed)
    tdt = y.dtype
    dz = torch.randn(P, C, generator=g, device=DEV).to(tdt)
    y64 = y.double()
    mean = y64.mean(0).float()
    invstd = (1 / torch.sqrt(y64.var(0, unbiased=False) + 1e-3)).float()
    gamma = torch.rand(C, generator=g, device=DEV) + 0.5
    beta = torch.randn(C, generator=g, device=DEV)
    sc = gamma * invstd
    sh = beta - mean * sc
    ybuf, yv = _slot(P, C, C + 16, dt, float("nan"))
    yv.copy_(y)
    dbuf, dv = _slot(P, C, C + 24, dt, float("nan"))
    dv.copy_(dz)
    rbuf, rv = _slot(P, C, C + 8, dt, float("nan"))
    rv.copy_(r)
    rp = rv.data_ptr() if res_mode else None
    nblk = L.bn_bwd_blocks(P, C)
    part = torch.full((nblk, C, 2), float("nan"), device=DEV)
    L.bn_act_bwd_reduce(dt, yv.data_ptr(), ybuf.stride(0), dv.data_ptr(), dbuf.stride(0), rp, rbuf.stride(0), sc.data_ptr(), sh.data_ptr(),
                        mean.data_ptr(), invstd.data_ptr(), act, res_mode, part.data_ptr(), P, C, st)
    prior = torch.randn(2, C, generator=g, device=DEV) if accumulate else torch.full((2, C), float("nan"), device=DEV)
    dgb = prior.clone()
    mg = torch.full((2, C), float("nan"), device=DEV)
    L.bn_bwd_finalize(part.data_ptr(), nblk, C, P, dgb[0].data_ptr(), dgb[1].data_ptr(), accumulate, mg[0].data_ptr(), mg[1].data_ptr(), st)
    obuf, ov = _slot(P, C, C + 40, dt, float("nan"))
    qbuf, qv = _slot(P, C, C + 48, dt, float("nan"))
    L.bn_act_bwd_apply(dt, yv.data_ptr(), ybuf.stride(0), dv.data_ptr(), dbuf.stride(0), rp, rbuf.stride(0), sc.data_ptr(), sh.data_ptr(),
                       mean.data_ptr(), invstd.data_ptr(), mg[0].data_ptr(), mg[1].data_ptr(), act, res_mode, train, ov.data_ptr(),
                       obuf.stride(0), qv.data_ptr() if res_mode == 2 else None, qbuf.stride(0), P, C, st)
    torch.cuda.synchronize()
    tag = f"dt={dt} P={P} C={C} act={act} res_mode={res_mode} train={train} accumulate={accumulate}"
    assert bool(obuf[:, :8].isnan().all()) and bool(obuf[:, 8 + C:].isnan().all()), f"bwd_apply {tag}: a store left the dy slot"
    # fp64 reference from the values passed in
    sc64, sh64, mu64, is64, dz64 = sc.double(), sh.double(), mean.double(), invstd.double(), dz.double()
    r64 = r.double()
    u, _, eu = _fwd_ref(y64, sc64, sh64, 0, 2 if res_mode == 2 else 0, r64)
    if act:
        sg = torch.sigmoid(u)
        dact = sg * (1 + u * (1 - sg))
        gg = dz64 * dact
        eg = dz64.abs() * (2.0 ** -21 * (2 + u.abs()) ** 2 + 0.3 * eu) + U * gg.abs()
    else:
        gg, eg = dz64, torch.zeros_like(dz64)
    xh = (y64 - mu64) * is64
    exh = 2 * U * xh.abs() + U * y64.abs() * is64
    n = -(-P // nblk)
    s1, s2 = gg.sum(0), (gg * xh).sum(0)
    e1 = eg.sum(0) + n * U * gg.abs().sum(0)
    e2 = (eg * xh.abs() + gg.abs() * exh).sum(0) + n * U * (gg * xh).abs().sum(0)
    # partials folded: sum g, sum g * xhat
    pf = part.double().sum(0)
    _check(f"bn_act_bwd_reduce sum g {tag}", pf[:, 0], s1, e1 + 1e-30)
    _check(f"bn_act_bwd_reduce sum g*xhat {tag}", pf[:, 1], s2, e2 + 1e-30)
    pri = prior.double() if accumulate else 0.0
    base = torch.stack((s2, s1)) + pri
    _check(f"bn_bwd_finalize dgamma/dbeta {tag}", dgb.double(), base, torch.stack((e2, e1)) + U * base.abs() * 2 + 1e-30)
    m1, m2 = s1 / P, s2 / P
    em1, em2 = e1 / P + U * m1.abs(), e2 / P + U * m2.abs()
    _check(f"bn_bwd_finalize means {tag}", mg.double(), torch.stack((m1, m2)), torch.stack((em1, em2)) + 1e-30)
    if train:
        inner = gg - m1 - xh * m2
        e_in = eg + em1 + xh.abs() * em2 + m2.abs() * exh + 3 * U * (gg.abs() + m1.abs() + (xh * m2).abs())
    else:
        inner, e_in = gg, eg
    dy = sc64 * inner
    edy = sc64.abs() * e_in + U * dy.abs()
    _check(f"bn_act_bwd_apply dy {tag}", ov.double(), dy, _store_tol(dt, dy, edy))
    if train and P <= 4096:
        # the formula is the fp64 autograd of act(BN(y)) (+res) through the batch statistics (same eps)
        yy = y64.clone().requires_grad_(True)
        m = yy.mean(0)
        v = yy.var(0, unbiased=False)
        uu = (yy - m) / torch.sqrt(v + 1e-3) * gamma.double() + beta.double() + (r64 if res_mode == 2 else 0)
        zz = uu * torch.sigmoid(uu) if act else uu
        zz.backward(dz64)
        ga = yy.grad
        # the kernel's inputs are the fp32-rounded statistics: compare with a correspondingly loose relative bound
        assert float((ga - dy).abs().max()) <= 1e-4 * float(ga.abs().max()) + 1e-6, f"{tag}: formula differs from autograd"
    if res_mode == 2:
        _check(f"bn_act_bwd_apply dres {tag}", qv.double(), gg, _store_tol(dt, gg, eg))
    return ov.clone(), qv.clone() if res_mode == 2 else None, pf


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("C", [32, 96, 640, 1152])
def test_bn_backward_chain_against_fp64(dt, C):
    for i, (act, res_mode, train, acc) in enumerate([(1, 0, 1, 0), (0, 0, 1, 1), (1, 2, 1, 0), (1, 1, 0, 0), (0, 2, 0, 1), (1, 2, 0, 1)]):
        _bwd_case(dt, 45 if i % 2 else 1500 + C // 8, C, act, res_mode, train, seed=C + 31 * i + dt, accumulate=acc)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("C", [32, 96, 512, 2048])
def test_colsum_partials_against_fp64(dt, C):
    L, st = y3d.lib(), ops.stream()
    for P in (50, 3001):
        g = torch.Generator(device=DEV).manual_seed(C + P)
        x = torch.randn(P, C, generator=g, device=DEV) * 5 + 2
        buf, xv = _slot(P, C, C + 24, dt, float("nan"))
        xv.copy_(x)
        nblk = L.bn_bwd_blocks(P, C)
        part = torch.full((nblk, C, 2), float("nan"), device=DEV)
        L.colsum_partials(dt, xv.data_ptr(), buf.stride(0), part.data_ptr(), P, C, st)
        torch.cuda.synchronize()
        xs = xv.double()
        n = -(-P // nblk)
        ref = xs.sum(0)
        assert bool((part[:, :, 1] == 0).all()), f"colsum dt={dt} C={C} P={P}: second slot must be zero"
        _check(f"colsum dt={dt} C={C} P={P}", part[:, :, 0].double().sum(0), ref, n * U * xs.abs().sum(0) + 1e-30)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [512, 640, 1152, 2048])
def test_wide_slabs_bit_identical(C):
    """y3d_set_bn_wide_slabs 0 / 1: bn_act_fwd and bn_act_bwd_apply are element-wise, so bit-identical; the reduce pass stays in its
    bound either way"""
    L = y3d.lib()
    old = L.set_bn_wide_slabs(1)
    try:
        outs = []
        for wide in (0, 1):
            L.set_bn_wide_slabs(wide)
            y, r, sc, sh, _ = _bn_inputs(BF16, 1777, C, C)
            z = [_run_fwd(BF16, y, r, sc, sh, act, rm, 1777, C).clone() for act in (0, 1) for rm in (0, 1, 2)]
            b = [_bwd_case(BF16, 1777, C, 1, rm, tr, seed=C + rm) for rm in (0, 2) for tr in (1, 0)]
            outs.append((z, b))
        (z0, b0), (z1, b1) = outs
        for i, (a, b) in enumerate(zip(z0, z1)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"bn_act_fwd C={C} variant {i}: wide slabs change the result"
        for i, (a, b) in enumerate(zip(b0, b1)):
            assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)), f"bn_act_bwd_apply C={C} variant {i}: wide slabs change dy"
            if a[1] is not None:
                assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)), f"bn_act_bwd_apply C={C} variant {i}: dres"
    finally:
        L.set_bn_wide_slabs(old)
