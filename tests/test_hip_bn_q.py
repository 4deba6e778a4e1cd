"""y3d_bn_act_fwd_q (the BatchNorm + SiLU pass that also writes the MX fp8 copy of z) and y3d_bn_eval_scale (csrc/bn_act.hip).

* bn_act_fwd_q documents itself as y3d_bn_act_fwd plus "exactly what y3d_fp8_quantize_act makes of z": z is held to BIT equality with
  y3d_bn_act_fwd on the same arguments, (q, s) to BIT equality with y3d_fp8_quantize_act of that z (both are tested against their own
  references in test_hip_bn_train.py / test_hip_fp8.py).  y and z are channel slots of wider sentinel-filled buffers; the pitch bytes
  of s beyond C / 32 and everything behind q and s keep the sentinel;
* bn_eval_scale: scale = gamma / sqrtf(var + eps), shift = beta - mean * scale.  fp32 division and sqrtf are correctly rounded in this
  build and nothing contracts (-ffp-contract=off), so the float32 restatement is held to BIT equality; the float64 bound of
  stem_optim_ref.bn_eval_scale_bound (3 roundings on scale, 2 more on shift) is the backstop."""
import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, Y3DError

import stem_optim_ref as S
import tail_ref as R
from test_hip_eval_tail import assert_bits, check_guard, guarded  # check_guard: fp32 outputs only

DEV = "cuda"


def _slot(P, C, extra):
    buf = R.sentinel((P, C + extra), torch.bfloat16, DEV)
    return buf, buf[:, 8:8 + C]


def _inputs(P, C, seed):
    """y with ordinary values, whole 32-channel blocks whose activation is 0, exact zeros inside live blocks, and magnitudes from
    1e-30 to 1e30 (block scales at both ends of the E8M0 range; e4m3's 448 is exceeded by many orders before scaling)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    y = torch.randn(P, C, generator=g, device=DEV) * 3 + 1
    sc = torch.rand(C, generator=g, device=DEV) * 2 - 0.5
    sh = torch.randn(C, generator=g, device=DEV)
    sc[:32], sh[:32] = 0.0, 0.0             # block 0: activation exactly 0 everywhere
    y[:, 40] = 0.0
    sh[40] = 0.0                            # one zero inside a live block
    y[::3, 32:64] *= 1e4                    # beyond 448 within a block of ordinary values
    y[::5, C - 32:] = 1e30 * torch.sign(y[::5, C - 32:])
    sc[C - 32:] = sc[C - 32:].abs() * 0.5 + 0.25
    y[2::7, C - 20] = 1e-30                 # tiny next to huge
    if P > 4:
        y[4, :] = 500.0 * torch.sign(y[4, :])
    return y.to(torch.bfloat16), sc, sh


@pytest.mark.gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("P", [1, 31, 33, 1000])
@pytest.mark.parametrize("C", [64, 128, 192])
def test_bn_act_fwd_q_is_bn_act_fwd_plus_quantize_act(C, P, act):
    L, st = y3d.lib(), ops.stream()
    y, sc, sh = _inputs(P, C, C + P + act)
    ybuf, yv = _slot(P, C, 16)
    yv.copy_(y)
    pitch = L.fp8_scale_pitch(C)
    assert pitch >= C // 32 and pitch % 4 == 0
    what = f"bn_act_fwd_q C={C} P={P} act={act}"
    # the two-pass form
    zrbuf, zr = _slot(P, C, 32)
    L.bn_act_fwd(BF16, yv.data_ptr(), ybuf.stride(0), sc.data_ptr(), sh.data_ptr(), act, 0, None, 0, zr.data_ptr(), zrbuf.stride(0), P, C, st)
    qrbuf, qr = guarded((P, C), torch.uint8)
    srbuf, sr = guarded((P, pitch), torch.uint8)
    L.fp8_quantize_act(zr.data_ptr(), zrbuf.stride(0), P, C, qr.data_ptr(), sr.data_ptr(), st)
    # the fused pass
    zbuf, z = _slot(P, C, 40)
    qbuf, q = guarded((P, C), torch.uint8)
    sbuf, s = guarded((P, pitch), torch.uint8)
    L.bn_act_fwd_q(yv.data_ptr(), ybuf.stride(0), sc.data_ptr(), sh.data_ptr(), act, z.data_ptr(), zbuf.stride(0), q.data_ptr(), s.data_ptr(),
                   P, C, st)
    torch.cuda.synchronize()
    assert bool(R.untouched(zbuf[:, :8]).all()) and bool(R.untouched(zbuf[:, 8 + C:]).all()), f"{what}: a store left the z slot"
    assert bool(z.isfinite().all()) and bool((z[:, :32] == 0).all()) and float(z.float().abs().max()) > 1e29
    assert_bits(z.contiguous(), zr.contiguous(), what + " z")
    assert bool(R.untouched(qbuf[q.numel():]).all()), f"{what}: a store went past the end of q"
    assert_bits(q, qr, what + " q")
    nb = C // 32
    assert_bits(s[:, :nb].contiguous(), sr[:, :nb].contiguous(), what + " s")
    assert bool(R.untouched(s[:, nb:]).all()), f"{what}: the pitch bytes of s were written"
    assert bool(R.untouched(sbuf[s.numel():]).all()), f"{what}: a store went past the end of s"
    # every code and scale byte was written: 0xA5 is a legitimate code, so a second run starts from the complementary fill
    q2 = torch.full((P, C), 0x5A, dtype=torch.uint8, device=DEV)
    s2 = torch.full((P, pitch), 0x5A, dtype=torch.uint8, device=DEV)
    L.bn_act_fwd_q(yv.data_ptr(), ybuf.stride(0), sc.data_ptr(), sh.data_ptr(), act, z.data_ptr(), zbuf.stride(0), q2.data_ptr(), s2.data_ptr(),
                   P, C, st)
    torch.cuda.synchronize()
    assert_bits(q2, qr, what + " q (second fill)")
    assert_bits(s2[:, :nb].contiguous(), sr[:, :nb].contiguous(), what + " s (second fill)")
    assert not bool((q[:, :32] != 0).any()), f"{what}: the all-zero block must quantise to zero codes"


@pytest.mark.gpu
def test_bn_act_fwd_q_rejected_arguments():
    L, st = y3d.lib(), ops.stream()
    P = 8
    ybuf, yv = _slot(P, 192, 16)
    zbuf, z = _slot(P, 192, 16)
    sc, sh = torch.ones(192, device=DEV), torch.zeros(192, device=DEV)
    q = R.sentinel((P * 192 + 16,), torch.uint8, DEV)
    s = R.sentinel((P * 8,), torch.uint8, DEV)

    def call(C=64, yp=yv.data_ptr(), zp=z.data_ptr(), qp=q.data_ptr(), sp=s.data_ptr(), ysw=ybuf.stride(0)):
        L.bn_act_fwd_q(yp, ysw, sc.data_ptr(), sh.data_ptr(), 1, zp, zbuf.stride(0), qp, sp, P, C, st)

    for kw in (dict(C=32), dict(C=96), dict(C=160), dict(C=68), dict(yp=yv.data_ptr() + 2), dict(zp=z.data_ptr() + 4), dict(qp=q.data_ptr() + 4),
               dict(qp=None), dict(sp=None), dict(ysw=ybuf.stride(0) + 4)):
        with pytest.raises(Y3DError):
            call(**kw)
    torch.cuda.synchronize()
    for buf in (zbuf, q, s):
        assert bool(R.untouched(buf).all()), "a rejected call wrote to an output"


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_eval_scale_bit_for_bit(C):
    L, st = y3d.lib(), ops.stream()
    rng = np.random.default_rng(C)
    gamma = (rng.standard_normal(C) * 1.5).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    mean = (rng.standard_normal(C) * 4).astype(np.float32)
    var = (rng.random(C) ** 4 * 10).astype(np.float32)
    var[::5] = 0.0        # eps alone under the root
    var[1::7] = 1e-12
    if C > 3:
        gamma[3], mean[2] = 0.0, 0.0
    worst = 0.0
    for eps in (1e-3, 1e-5):
        dev = [torch.from_numpy(a).to(DEV) for a in (gamma, beta, mean, var)]
        bs, sc = guarded((C,), torch.float32)
        bh, sh = guarded((C,), torch.float32)
        L.bn_eval_scale(C, *(d.data_ptr() for d in dev), eps, sc.data_ptr(), sh.data_ptr(), st)
        torch.cuda.synchronize()
        what = f"bn_eval_scale C={C} eps={eps}"
        check_guard(bs, sc, what + " scale")
        check_guard(bh, sh, what + " shift")
        r64 = S.bn_eval_scale_f64(gamma, beta, mean, var, eps)
        tol = S.bn_eval_scale_bound(gamma, beta, mean, var, eps)
        for got, ref, t, name in ((sc, r64[0], tol[0], "scale"), (sh, r64[1], tol[1], "shift")):
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert (err <= t).all(), f"{what} {name}: {float((err / t).max()):.3g} x the float64 bound"
            worst = max(worst, float((err / t).max()))
        r32 = S.bn_eval_scale_f32(gamma, beta, mean, var, eps)
        assert_bits(sc, torch.from_numpy(r32[0]), what + " scale")
        assert_bits(sh, torch.from_numpy(r32[1]), what + " shift")
    print(f"bn_eval_scale C={C}: largest error {worst:.3g} x the float64 bound")
