"""The head projections through the C ABI against the host references of proj_attn_ref.py: csrc/proj_group.hip (y3d_proj_group_fwd,
_fwd_bn, _bwd_data, _bwd_weight, _bwd_weight_bn), csrc/proj_bn_mfma.hip (y3d_proj_group_fwd_bn_mfma, _bwd_weight_bn_mfma,
y3d_proj_group_bn_bwd modes 0 / 1) and the single-branch y3d_proj_fwd, y3d_proj_bwd_data, y3d_proj_bwd_weight, y3d_slab_reduce of
csrc/misc.hip.

What the kernels load decides the layouts (proj_attn_ref.group_layout).  The activations (x, y_pre) and their gradients (dx, dy of
mode 1) move as 16-byte chunks at channel offsets xoff + multiples of the chunk: every xoff, C and their pixel strides are multiples
of the chunk and the slices start 16-byte aligned.  The projected map and its gradient (y, out, dy, dout) are read and written
element by element: their strides (ysw = tot + 5, dsw = tot + 3) and column offsets are odd.  "strided": the branch slices are not
in ascending order, one slice in the middle of C and a chunk at its end are covered by no branch (their dx / dy / partials must
keep the sentinel), the forward lets two branches read one slice.  Every output lives in a sentinel-filled buffer with guard rows.

EXACT cases: integer activations, gradients, weights and biases with |.| <= 4; the BatchNorm forms with act = 0, scale in
{1/2, 1, 2} and integer shift (and integer mean, invstd a power of two, integer mean_g / mean_gx for y3d_proj_group_bn_bwd).  Every
product and every fp32 partial sum is a multiple of 1/4 far below 2^24 (65 537 pixels x 4 x 10), so any block, wave, lane or slab
order gives the exact sum and the store rounds ONCE: bit equality (up to the sign of zero) with the float64 reference rounded to
the storage type.  Weights are bf16-representable: the MFMA and VALU forms share the reference.

REAL-valued cases (act = 1, random scale / shift, bf16): bounds as tests/test_hip_bn_train.py builds them (u = 2^-24):
* u = y scale + shift: 3u (|y scale| + |shift|); t = silu(u) through v_exp_f32 / v_rcp_f32: et = 1.1 eu + 2^-21 (4 + |u|) |t|;
  silu'(u): 2^-21 (2 + |u|)^2 + 0.3 eu.
* the activation is ROUNDED to bf16 in the kernel and in the reference.  Where t is further than et from a bf16 rounding boundary
  both round alike (error 0); where it is not, the kernel may land on the neighbour: one bf16 ulp for that activation
  (proj_attn_ref.flip_ulp), times |w| (forward) or |dout| (weight gradient).
* fp32 sums of n terms in any order: n u sum |terms| (forward: n = cin + 8; weight / bias gradient and mode-0 partials: the pixels
  of a run + the rows folded behind it), one fp32 or bf16 store (_store_tol).
* the MFMA forms round W to bf16 as they load it: the reference rounds W the same way (round to nearest even: a truncating
  conversion would fail the "f32" weight cases, which are not bf16-representable; the "bf16" cases are).
* mode 1 takes mean_g / mean_gx from the float64 reference (rounded to fp32, and the reference uses those values)."""
import ctypes

import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32, Y3DError

import proj_attn_ref as R
from test_hip_attention import assert_exact, check_slot, flat_slot, in_rows, out_slot
from test_hip_bn_train import U, _check, _store_tol

DEV = "cuda"


def IA(v):
    return (ctypes.c_int * len(v))(*v)


def PV(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def dev32(ts):
    return [t.float().to(DEV).contiguous() for t in ts]


def covered(xoff, cin, C):
    m = torch.zeros(C, dtype=torch.bool)
    for o in xoff:
        m[o:o + cin] = True
    return m


def check_cols(buf, view, cov, what):
    """the covered columns of the (P, C) view written, its other columns and the rest of the buffer untouched"""
    cov = cov.to(view.device)
    assert not bool(R.untouched(view[:, cov]).any()), f"{what}: covered elements were never written"
    if bool((~cov).any()):
        assert bool(R.untouched(view[:, ~cov]).all()), f"{what}: a store reached a channel no branch covers"
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    sw = view.stride(0)
    r0, c0 = divmod(view.storage_offset(), sw)
    mask.view(-1, sw)[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    assert bool(R.untouched(buf)[mask].all()), f"{what}: a store left the output slice"


def grad_slots(couts, cin):
    dw = [flat_slot(co * cin) for co in couts]
    db = [flat_slot(co) for co in couts]
    return dw, db


def check_grads(dw, db, what):
    for buf, v in dw + db:
        check_slot(buf, v, what)


def exact_operands(P, C, couts, cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = R.ints((P, C), 4, g)
    ws = [R.ints((co, cin), 4, g) for co in couts]
    bs = [R.ints((co,), 4, g) for co in couts]
    dy = R.ints((P, sum(couts)), 4, g)
    scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    shift = R.ints((C,), 2, g)
    return x, ws, bs, dy, scale, shift, g


def _pg_id(c):
    return "-".join(("bf16" if v == BF16 else "f32") if i == 0 else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v)) for i, v in enumerate(c))


def _weight_grad_exact(L, st, entry, dt, nb, cin, xd, xsw, xoff, dyd, dsw, couts, P, bn, nblk, want_w, want_b, what):
    tot = sum(couts)
    sbuf, slab = flat_slot(nblk * tot * cin)
    bbuf, bslab = flat_slot(nblk * tot)
    dw, db = grad_slots(couts, cin)
    args = (nb, cin, xd.data_ptr(), xsw, IA(xoff), dyd.data_ptr(), dsw, IA(couts)) + bn + \
        (slab.data_ptr(), bslab.data_ptr(), PV([v for _, v in dw]), PV([v for _, v in db]), P, st)
    entry(*(((dt,) if dt is not None else ()) + args))
    torch.cuda.synchronize()
    check_slot(sbuf, slab, what + " slab")
    check_slot(bbuf, bslab, what + " bias slab")
    check_grads(dw, db, what)
    for br in range(nb):
        assert_exact(dw[br][1].double().cpu().view(couts[br], cin), want_w[br], f"{what} dw[{br}]")
        assert_exact(db[br][1].double().cpu(), want_b[br], f"{what} db[{br}]")
    # the slabs hold per-block partial sums of the same gradients
    ooff, _ = R.branch_offsets(couts)
    sl = slab.double().cpu().view(nblk, tot, cin).sum(0)
    for br in range(nb):
        assert_exact(sl[ooff[br]:ooff[br] + couts[br]], want_w[br], f"{what} slab rows of branch {br}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.PG_CASES, ids=_pg_id)
def test_group_projections_exact(case):
    dt, P, nb, couts, cin, lay = case
    L, st = y3d.lib(), ops.stream()
    tdt, ce, tot = R.TDT[dt], R.CE[dt], sum(couts)
    lf, lb = R.group_layout(nb, cin, couts, lay, dt, True), R.group_layout(nb, cin, couts, lay, dt, False)
    C, xsw, ysw, dsw = lf["C"], lf["xsw"], lf["ysw"], lf["dsw"]
    xo, yo, do = (ce, 2, 1) if lay == "strided" else (0, 0, 0)
    x, ws, bs, dy, scale, shift, _ = exact_operands(P, C, couts, cin, P + cin + nb)
    wd, bd = dev32(ws), dev32(bs)
    scd, shd = scale.float().to(DEV), shift.float().to(DEV)
    xd = in_rows(x, xsw, xo, tdt)
    dyd = in_rows(dy, dsw, do, tdt)
    act = R.bn_act(x, scale, shift, 0, tdt)
    assert torch.equal(act, x * scale[None, :] + shift[None, :])
    # forward, plain and with the folded BatchNorm
    for name, src, bn in (("proj_group_fwd", x, ()), ("proj_group_fwd_bn", act, (scd.data_ptr(), shd.data_ptr(), 0))):
        ybuf, y = out_slot(P, tot, ysw, yo, tdt)
        getattr(L, name)(dt, nb, cin, xd.data_ptr(), xsw, IA(lf["xoff"]), PV(wd), PV(bd), IA(couts), *bn, y.data_ptr(), ysw, P, st)
        torch.cuda.synchronize()
        check_slot(ybuf, y, f"{name} {case}")
        want = R.rnd(R.proj_fwd(src, ws, bs, lf["xoff"], comp=False)[0], tdt)
        assert_exact(y.double().cpu(), want, f"{name} {case}")
    # data gradient: distinct slices
    cov = covered(lb["xoff"], cin, C)
    dbuf, dx = out_slot(P, C, xsw, xo, tdt)
    L.proj_group_bwd_data(dt, nb, cin, dyd.data_ptr(), dsw, IA(lb["xoff"]), PV(wd), IA(couts), dx.data_ptr(), xsw, P, st)
    torch.cuda.synchronize()
    check_cols(dbuf, dx, cov, f"proj_group_bwd_data {case}")
    want = R.rnd(R.proj_bwd_data(dy, ws, lb["xoff"], C, comp=False)[0][:, cov], tdt)
    assert_exact(dx.double().cpu()[:, cov], want, f"proj_group_bwd_data {case}")
    # weight and bias gradients, plain and with the folded BatchNorm
    nblk = L.proj_group_blocks(P)
    for name, src, bn in (("proj_group_bwd_weight", x, ()), ("proj_group_bwd_weight_bn", act, (scd.data_ptr(), shd.data_ptr(), 0))):
        dw, db, _, _ = R.proj_bwd_weight(src, dy, lf["xoff"], couts, cin, comp=False)
        _weight_grad_exact(L, st, getattr(L, name), dt, nb, cin, xd, xsw, lf["xoff"], dyd, dsw, couts, P, bn, nblk, dw, db, f"{name} {case}")


def _pm_id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.PM_CASES, ids=_pm_id)
def test_mfma_projections_exact(case):
    P, nb, couts, cin, lay = case
    L, st = y3d.lib(), ops.stream()
    dt, tdt, tot = BF16, torch.bfloat16, sum(couts)
    lf, lb = R.group_layout(nb, cin, couts, lay, dt, True), R.group_layout(nb, cin, couts, lay, dt, False)
    C, ysw, osw, dsw, dysw = lf["C"], lf["xsw"], lf["ysw"], lf["dsw"], lf["dysw"]
    xo, yo, do = (8, 2, 1) if lay == "strided" else (0, 0, 0)
    y, ws, bs, dout, scale, shift, g = exact_operands(P, C, couts, cin, P + cin + nb + 1)
    wd, bd = dev32(ws), dev32(bs)
    scd, shd = scale.float().to(DEV), shift.float().to(DEV)
    yd = in_rows(y, ysw, xo, tdt)
    dd = in_rows(dout, dsw, do, tdt)
    act = R.bn_act(y, scale, shift, 0, tdt)
    # forward
    obuf, out = out_slot(P, tot, osw, yo, tdt)
    L.proj_group_fwd_bn_mfma(nb, cin, yd.data_ptr(), ysw, IA(lf["xoff"]), PV(wd), PV(bd), IA(couts), scd.data_ptr(), shd.data_ptr(), 0,
                             out.data_ptr(), osw, P, st)
    torch.cuda.synchronize()
    check_slot(obuf, out, f"proj_group_fwd_bn_mfma {case}")
    assert_exact(out.double().cpu(), R.rnd(R.proj_fwd(act, ws, bs, lf["xoff"], comp=False)[0], tdt), f"proj_group_fwd_bn_mfma {case}")
    # weight and bias gradient
    nblk = L.proj_group_bwd_weight_bn_mfma_blocks(P)
    dw, db, _, _ = R.proj_bwd_weight(act, dout, lf["xoff"], couts, cin, comp=False)
    _weight_grad_exact(L, st, L.proj_group_bwd_weight_bn_mfma, None, nb, cin, yd, ysw, lf["xoff"], dd, dsw, couts, P,
                       (scd.data_ptr(), shd.data_ptr(), 0), nblk, dw, db, f"proj_group_bwd_weight_bn_mfma {case}")
    # BatchNorm backward behind the projections: integer mean, invstd a power of two, integer mean_g / mean_gx
    mean = R.ints((C,), 2, g)
    invstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (C,), generator=g)]
    mg, mgx = R.ints((C,), 3, g), R.ints((C,), 2, g)
    cov = covered(lb["xoff"], cin, C)
    r = R.bn_bwd(y, dout, ws, lb["xoff"], scale, shift, mean, invstd, 0)
    med, isd, mgd, mgxd = (t.float().to(DEV) for t in (mean, invstd, mg, mgx))
    nrun = L.proj_group_bn_bwd_blocks(P)
    ppb = -(-(-(-P // nrun)) // 64) * 64
    pbuf, part = out_slot(nrun, 2 * C, 2 * C, 0, torch.float32)
    common = (nb, cin, yd.data_ptr(), ysw, IA(lb["xoff"]), dd.data_ptr(), dsw, PV(wd), IA(couts), scd.data_ptr(), shd.data_ptr(), med.data_ptr(),
              isd.data_ptr())
    L.proj_group_bn_bwd(0, *common, None, None, 0, part.data_ptr(), nrun, None, 0, P, C, st)
    torch.cuda.synchronize()
    cov2 = cov.repeat_interleave(2)
    check_cols(pbuf, part, cov2, f"proj_group_bn_bwd mode 0 {case}")
    got = part.double().cpu().view(nrun, C, 2)[:, cov]
    want = torch.zeros(nrun, int(cov.sum()), 2, dtype=torch.float64)  # a run that starts past P writes zeros
    for b in range(nrun):
        lo, hi = b * ppb, min(P, (b + 1) * ppb)
        if lo < hi:
            want[b, :, 0], want[b, :, 1] = r["g"][lo:hi][:, cov].sum(0), r["gx"][lo:hi][:, cov].sum(0)
    assert_exact(got, want, f"proj_group_bn_bwd mode 0 {case}")
    ybuf, dyo = out_slot(P, C, dysw, xo, tdt)
    L.proj_group_bn_bwd(1, *common, mgd.data_ptr(), mgxd.data_ptr(), 0, None, 0, dyo.data_ptr(), dysw, P, C, st)
    torch.cuda.synchronize()
    check_cols(ybuf, dyo, cov, f"proj_group_bn_bwd mode 1 {case}")
    assert_exact(dyo.double().cpu()[:, cov], R.rnd(R.bn_bwd_apply(r, scale, mg, mgx)[:, cov], tdt), f"proj_group_bn_bwd mode 1 {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.P1_CASES, ids=_pg_id)
def test_single_branch_projection_exact(case):
    dt, P, cin, cout, lay = case
    L, st = y3d.lib(), ops.stream()
    tdt, ce = R.TDT[dt], R.CE[dt]
    xsw, ysw, dsw = (cin + 2 * ce, cout + 5, cout + 3) if lay == "strided" else (cin, cout, cout)
    xo, yo, do = (ce, 2, 1) if lay == "strided" else (0, 0, 0)
    x, (w,), (b,), dy, _, _, g = exact_operands(P, cin, (cout,), cin, P + cin + cout)
    (wd,), (bd,) = dev32([w]), dev32([b])
    xd, dyd = in_rows(x, xsw, xo, tdt), in_rows(dy, dsw, do, tdt)
    for bias in (b, None):
        ybuf, y = out_slot(P, cout, ysw, yo, tdt)
        L.proj_fwd(dt, xd.data_ptr(), xsw, wd.data_ptr(), bd.data_ptr() if bias is not None else None, y.data_ptr(), ysw, P, cin, cout, st)
        torch.cuda.synchronize()
        check_slot(ybuf, y, f"proj_fwd {case}")
        want = R.proj_fwd(x, [w], [bias] if bias is not None else None, [0], comp=False)[0]
        assert_exact(y.double().cpu(), R.rnd(want, tdt), f"proj_fwd {case} bias={bias is not None}")
    dbuf, dx = out_slot(P, cin, xsw, xo, tdt)
    L.proj_bwd_data(dt, dyd.data_ptr(), dsw, wd.data_ptr(), dx.data_ptr(), xsw, P, cin, cout, st)
    torch.cuda.synchronize()
    check_slot(dbuf, dx, f"proj_bwd_data {case}")
    assert_exact(dx.double().cpu(), R.rnd(R.proj_bwd_data(dy, [w], [0], cin, comp=False)[0], tdt), f"proj_bwd_data {case}")
    nblk = L.proj_blocks(P)
    (dw,), (db,), _, _ = R.proj_bwd_weight(x, dy, [0], (cout,), cin, comp=False)
    for accumulate in (0, 1):
        sbuf, slab = flat_slot(nblk * cout * cin)
        bbuf, bslab = flat_slot(nblk * cout)
        gwb, gw = flat_slot(cout * cin)
        gbb, gb = flat_slot(cout)
        pw, pb = R.ints((cout * cin,), 100, g), R.ints((cout,), 100, g)
        if accumulate:
            gw.copy_(pw.float().to(DEV)), gb.copy_(pb.float().to(DEV))
        L.proj_bwd_weight(dt, xd.data_ptr(), xsw, dyd.data_ptr(), dsw, slab.data_ptr(), bslab.data_ptr(), gw.data_ptr(), gb.data_ptr(), accumulate,
                          P, cin, cout, st)
        torch.cuda.synchronize()
        for buf, v in ((sbuf, slab), (bbuf, bslab), (gwb, gw), (gbb, gb)):
            check_slot(buf, v, f"proj_bwd_weight {case} accumulate={accumulate}")
        assert_exact(gw.double().cpu().view(cout, cin), dw + (pw.view(cout, cin) if accumulate else 0), f"proj_bwd_weight dw {case} acc={accumulate}")
        assert_exact(gb.double().cpu(), db + (pb if accumulate else 0), f"proj_bwd_weight db {case} acc={accumulate}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.SR_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_slab_reduce_exact(case):
    nblk, n = case
    L, st = y3d.lib(), ops.stream()
    g = torch.Generator().manual_seed(nblk + n)
    slab, prior = R.ints((nblk, n), 1000, g), R.ints((n,), 1000, g)
    sd = slab.float().to(DEV)
    for accumulate in (0, 1):
        buf, out = flat_slot(n)
        if accumulate:
            out.copy_(prior.float().to(DEV))
        L.slab_reduce(sd.data_ptr(), out.data_ptr(), nblk, n, accumulate, st)
        torch.cuda.synchronize()
        check_slot(buf, out, f"slab_reduce {case}")
        assert_exact(out.double().cpu(), slab.sum(0) + (prior if accumulate else 0), f"slab_reduce {case} accumulate={accumulate}")


# ---------------------------------------------------------------------------------------------------------------- real-valued
def _act_ref(y, scale, shift):
    """float64 u, t = silu(u), their fp32 error bounds, the bf16 activation and the ulp it may be off by (module docstring)"""
    ysc = y * scale[None, :]
    u = ysc + shift[None, :]
    eu = 3 * U * (ysc.abs() + shift.abs()[None, :])
    t = R.silu(u)
    et = 1.1 * eu + 2.0 ** -21 * (4 + u.abs()) * t.abs()
    return u, eu, t.bfloat16().double(), R.flip_ulp(t, et)


def _cols(t, xoff, cin):
    return [t[:, o:o + cin] for o in xoff]


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.PR_CASES, ids=_pm_id)
def test_batchnorm_projections_against_float64(case):
    P, nb, couts, cin, wkind = case
    L, st = y3d.lib(), ops.stream()
    dt, tdt, tot = BF16, torch.bfloat16, sum(couts)
    lay = R.group_layout(nb, cin, couts, "strided", dt, False)
    C, ysw, osw, dsw, dysw, xoff = lay["C"], lay["xsw"], lay["ysw"], lay["dsw"], lay["dysw"], lay["xoff"]
    ooff, _ = R.branch_offsets(couts)
    g = torch.Generator().manual_seed(P + nb)
    y = (torch.randn(P, C, generator=g) * 2 + 0.5).bfloat16().double()
    dout = torch.randn(P, tot, generator=g).bfloat16().double()
    ws = [(torch.randn(co, cin, generator=g) * 0.3).float() for co in couts]
    if wkind == "bf16":
        ws = [w.bfloat16().float() for w in ws]
    else:
        assert not torch.equal(ws[0], ws[0].bfloat16().float())
    ws = [w.double() for w in ws]
    wm = [w.bfloat16().double() for w in ws]  # what the MFMA forms multiply by
    bs = [torch.randn(co, generator=g).float().double() for co in couts]
    y64 = y[:, :]
    mean = y64.mean(0).float().double()
    invstd = (1 / torch.sqrt(y64.var(0, unbiased=False) + 1e-3)).float().double()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double()
    scale = (gamma * invstd).float().double()
    shift = (beta - mean * scale).float().double()
    wd, bd = dev32(ws), dev32(bs)
    scd, shd, med, isd = (t.float().to(DEV) for t in (scale, shift, mean, invstd))
    yd, dd = in_rows(y, ysw, 8, tdt), in_rows(dout, dsw, 1, tdt)
    u, eu, a, ea = _act_ref(y, scale, shift)
    tag = f"{case}"
    # forward: VALU with W as given, MFMA with W rounded to bf16
    for name, wref, n in (("proj_group_fwd_bn", ws, cin + 8), ("proj_group_fwd_bn_mfma", wm, cin + 8)):
        obuf, out = out_slot(P, tot, osw, 2, tdt)
        args = (nb, cin, yd.data_ptr(), ysw, IA(xoff), PV(wd), PV(bd), IA(couts), scd.data_ptr(), shd.data_ptr(), 1, out.data_ptr(), osw, P, st)
        getattr(L, name)(*(((dt,) if name == "proj_group_fwd_bn" else ()) + args))
        torch.cuda.synchronize()
        check_slot(obuf, out, f"{name} {tag}")
        ref, refa = R.proj_fwd(a, wref, bs, xoff)
        flip, _ = R.proj_fwd(ea, [w.abs() for w in wref], None, xoff, comp=False)
        _check(f"{name} {tag}", out.double().cpu(), ref, _store_tol(dt, ref, n * U * refa + flip))
    # weight / bias gradients
    for name, mf in (("proj_group_bwd_weight_bn", False), ("proj_group_bwd_weight_bn_mfma", True)):
        nblk = L.proj_group_bwd_weight_bn_mfma_blocks(P) if mf else L.proj_group_blocks(P)
        n = -(-P // nblk) + 128 + nblk + 16
        sbuf, slab = flat_slot(nblk * tot * cin)
        bbuf, bslab = flat_slot(nblk * tot)
        dws, dbs = grad_slots(couts, cin)
        args = (nb, cin, yd.data_ptr(), ysw, IA(xoff), dd.data_ptr(), dsw, IA(couts), scd.data_ptr(), shd.data_ptr(), 1, slab.data_ptr(), bslab.data_ptr(),
                PV([v for _, v in dws]), PV([v for _, v in dbs]), P, st)
        getattr(L, name)(*(((dt,) if not mf else ()) + args))
        torch.cuda.synchronize()
        check_slot(sbuf, slab, f"{name} {tag} slab")
        check_slot(bbuf, bslab, f"{name} {tag} bias slab")
        check_grads(dws, dbs, f"{name} {tag}")
        dw, db, dwa, dba = R.proj_bwd_weight(a, dout, xoff, couts, cin)
        fl, _, _, _ = R.proj_bwd_weight(ea, dout.abs(), xoff, couts, cin, comp=False)
        for br in range(nb):
            _check(f"{name} {tag} dw[{br}]", dws[br][1].double().cpu().view(couts[br], cin), dw[br], _store_tol(F32, dw[br], n * U * dwa[br] + fl[br]))
            _check(f"{name} {tag} db[{br}]", dbs[br][1].double().cpu(), db[br], _store_tol(F32, db[br], n * U * dba[br]))
    # BatchNorm backward behind the projections (W rounded to bf16, at most 32 outputs per dz)
    r = R.bn_bwd(y, dout, wm, xoff, scale, shift, mean, invstd, 1)
    cov = covered(xoff, cin, C)
    sg = 1 / (1 + torch.exp(-u))
    da = sg * (1 + u * (1 - sg))
    edz = 32 * U * r["dz_abs"]
    eg = r["dz"].abs() * (2.0 ** -21 * (2 + u.abs()) ** 2 + 0.3 * eu) + U * r["g"].abs() + edz * da.abs()
    xh = r["xhat"]
    exh = 2 * U * xh.abs() + U * y.abs() * invstd[None, :]
    nrun = L.proj_group_bn_bwd_blocks(P)
    ppb = -(-(-(-P // nrun)) // 64) * 64
    n = ppb + 64
    pbuf, part = out_slot(nrun, 2 * C, 2 * C, 0, torch.float32)
    common = (nb, cin, yd.data_ptr(), ysw, IA(xoff), dd.data_ptr(), dsw, PV(wd), IA(couts), scd.data_ptr(), shd.data_ptr(), med.data_ptr(), isd.data_ptr())
    L.proj_group_bn_bwd(0, *common, None, None, 1, part.data_ptr(), nrun, None, 0, P, C, st)
    torch.cuda.synchronize()
    check_cols(pbuf, part, cov.repeat_interleave(2), f"proj_group_bn_bwd mode 0 {tag}")
    got = part.double().cpu().view(nrun, C, 2)[:, cov]
    nc = int(cov.sum())
    want, tol = torch.zeros(nrun, nc, 2, dtype=torch.float64), torch.zeros(nrun, nc, 2, dtype=torch.float64)
    e2 = eg * xh.abs() + r["g"].abs() * exh
    for b in range(nrun):
        lo, hi = b * ppb, min(P, (b + 1) * ppb)
        if lo < hi:
            sl = slice(lo, hi)
            want[b, :, 0], want[b, :, 1] = r["g"][sl][:, cov].sum(0), r["gx"][sl][:, cov].sum(0)
            tol[b, :, 0] = eg[sl][:, cov].sum(0) + n * U * r["g"][sl][:, cov].abs().sum(0)
            tol[b, :, 1] = e2[sl][:, cov].sum(0) + n * U * r["gx"][sl][:, cov].abs().sum(0)
    assert int((want[:, :, 0] == 0).all(1).sum()) == (63 if P == 8193 else 0), "runs that start past P"
    _check(f"proj_group_bn_bwd mode 0 {tag}", got, want, tol + U * want.abs() + 1e-30)
    m1 = (r["g"][:, cov].sum(0) / P).float().double()
    m2 = (r["gx"][:, cov].sum(0) / P).float().double()
    mg, mgx = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    mg[cov], mgx[cov] = m1, m2
    mgd, mgxd = mg.float().to(DEV), mgx.float().to(DEV)
    ybuf, dyo = out_slot(P, C, dysw, 8, tdt)
    L.proj_group_bn_bwd(1, *common, mgd.data_ptr(), mgxd.data_ptr(), 1, None, 0, dyo.data_ptr(), dysw, P, C, st)
    torch.cuda.synchronize()
    check_cols(ybuf, dyo, cov, f"proj_group_bn_bwd mode 1 {tag}")
    dy = R.bn_bwd_apply(r, scale, mg, mgx)
    e_in = eg + mgx.abs()[None, :] * exh + 3 * U * (r["g"].abs() + mg.abs()[None, :] + (xh * mgx[None, :]).abs())
    edy = scale.abs()[None, :] * e_in + U * dy.abs()
    _check(f"proj_group_bn_bwd mode 1 {tag}", dyo.double().cpu()[:, cov], dy[:, cov], _store_tol(dt, dy[:, cov], edy[:, cov]))


# ---------------------------------------------------------------------------------------------------------------- rejections
@pytest.mark.gpu
def test_projection_rejections_leave_outputs_untouched():
    """every call below is refused on the host (an error comes back, nothing is launched): the argument checks that
    y3d_proj_group_bwd_data / _bwd_weight / _bwd_weight_bn lacked (dtype, cin % chunk, dsw >= sum(couts)), the bias the forward needs,
    and the standing checks of the MFMA entries"""
    L, st = y3d.lib(), ops.stream()
    P, nb, cin, couts = 64, 2, 64, (3, 24)
    tot, C = sum(couts), 128
    xoff = [0, 64]
    x = torch.zeros(P, C, dtype=torch.float32, device=DEV)       # large enough for either dtype
    dy = torch.zeros(P, 64, dtype=torch.float32, device=DEV)
    ws = [torch.zeros(32, 128, device=DEV) for _ in range(nb)]
    bs = [torch.zeros(32, device=DEV) for _ in range(nb)]
    vec = torch.ones(C, device=DEV)
    outs = []

    def slot(n):
        buf, v = flat_slot(n)
        outs.append(buf)
        return v

    def refused(fn, *args):
        with pytest.raises(Y3DError):
            fn(*args)

    ybuf = slot(P * C)
    slab, bslab = slot(64 * tot * 128), slot(64 * tot)
    dws, dbs = [slot(32 * 128) for _ in range(nb)], [slot(32) for _ in range(nb)]
    part = slot(128 * C * 2)
    sc = (vec.data_ptr(), vec.data_ptr())

    def fwd(dt=BF16, cin=cin, b=PV(bs), ysw=tot, couts=couts):
        return (L.proj_group_fwd, dt, nb, cin, x.data_ptr(), C, IA(xoff), PV(ws), b, IA(couts), ybuf.data_ptr(), ysw, P, st)

    def bwd_data(dt=BF16, cin=cin, dsw=tot, couts=couts):
        return (L.proj_group_bwd_data, dt, nb, cin, dy.data_ptr(), dsw, IA(xoff), PV(ws), IA(couts), ybuf.data_ptr(), C, P, st)

    def bwd_w(dt=BF16, cin=cin, dsw=tot, bn=False, couts=couts):
        fn = L.proj_group_bwd_weight_bn if bn else L.proj_group_bwd_weight
        return (fn, dt, nb, cin, x.data_ptr(), C, IA(xoff), dy.data_ptr(), dsw, IA(couts)) + ((*sc, 1) if bn else ()) + \
            (slab.data_ptr(), bslab.data_ptr(), PV(dws), PV(dbs), P, st)

    def mf_fwd(cin=cin, xoff=xoff, couts=couts, osw=tot, ysw=C, b=PV(bs)):
        return (L.proj_group_fwd_bn_mfma, nb, cin, x.data_ptr(), ysw, IA(xoff), PV(ws), b, IA(couts), *sc, 1, ybuf.data_ptr(), osw, P, st)

    def mf_w(cin=cin, xoff=xoff, couts=couts, dsw=tot, ysw=C):
        return (L.proj_group_bwd_weight_bn_mfma, nb, cin, x.data_ptr(), ysw, IA(xoff), dy.data_ptr(), dsw, IA(couts), *sc, 1, slab.data_ptr(),
                bslab.data_ptr(), PV(dws), PV(dbs), P, st)

    def mf_bn(mode, cin=cin, xoff=xoff, couts=couts, dsw=tot, nblk=1, dysw=C, ysw=C):
        return (L.proj_group_bn_bwd, mode, nb, cin, x.data_ptr(), ysw, IA(xoff), dy.data_ptr(), dsw, PV(ws), IA(couts), *sc, *sc, *sc, 1,
                part.data_ptr(), nblk, ybuf.data_ptr(), dysw, P, C, st)

    assert L.proj_group_bn_bwd_blocks(P) == 1
    calls = [
        fwd(b=None), fwd(dt=2), fwd(cin=68), fwd(ysw=tot - 1), fwd(couts=(3, 25)), fwd(dt=F32, cin=66),
        bwd_data(dt=2), bwd_data(dt=-1), bwd_data(cin=68), bwd_data(dt=F32, cin=66), bwd_data(dsw=tot - 1), bwd_data(couts=(3, 25)),
        bwd_w(dt=2), bwd_w(cin=68), bwd_w(dt=F32, cin=66), bwd_w(dsw=tot - 1), bwd_w(couts=(0, 24)),
        bwd_w(dt=2, bn=True), bwd_w(cin=68, bn=True), bwd_w(dt=F32, cin=66, bn=True), bwd_w(dsw=tot - 1, bn=True),
        mf_fwd(cin=32), mf_fwd(cin=80), mf_fwd(xoff=[0, 68]), mf_fwd(couts=(3, 33)), mf_fwd(osw=tot - 1), mf_fwd(ysw=C + 4), mf_fwd(b=None),
        mf_w(cin=256), mf_w(xoff=[4, 64]), mf_w(couts=(33, 3)), mf_w(dsw=tot - 1), mf_w(ysw=C + 4),
        mf_bn(0, cin=32), mf_bn(1, cin=96), mf_bn(0, xoff=[0, 60]), mf_bn(0, xoff=[0, 72]), mf_bn(1, couts=(33, 1)), mf_bn(0, nblk=2), mf_bn(0, nblk=0),
        mf_bn(0, dsw=tot - 1), mf_bn(1, dsw=tot - 1), mf_bn(1, dysw=cin - 8), mf_bn(1, dysw=C + 4), mf_bn(2), mf_bn(0, ysw=C + 4),
    ]
    for c in calls:
        refused(*c)
    torch.cuda.synchronize()
    for buf in outs:
        assert bool(R.untouched(buf).all()), "a rejected call wrote to its outputs"
