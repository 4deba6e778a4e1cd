"""GPU: the foreground depth map loss (csrc/fgdm_loss.hip, loss.ForegroundDepthMapLoss) against the float64 restatement of the
reference (tests/depth_map_ref.py): targets exactly, loss and gradient element by element, fp32 / bf16, contiguous / channels_last."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import has_gpu

import depth_map_ref as R
import yolov10_3d_amd as y3d
from yolov10_3d_amd import loss as PL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV = "cuda"
ARGS = SimpleNamespace(min_depth_threshold=R.DMIN, max_depth_threshold=R.DMAX)
CASES = R.loss_cases()

# The yardstick: the reference's formula run in float32 on the CPU (torch) against the float64 restatement, over CASES, as
# tests/test_depth_map_ref_host.py::test_float32_yardstick measures it: loss |a - ref| / |ref|, gradient max |a - ref| / max |ref|.
F32_LOSS_DIST = 2.63e-7
F32_GRAD_DIST = 9.27e-7
# The kernel may sum in another, equally valid order, which can double a float32 error: four times the yardstick, as the attention tests
LOSS_TOL = 4 * F32_LOSS_DIST  # 1.05e-6
GRAD_TOL = 4 * F32_GRAD_DIST  # 3.71e-6


def bf16_half_ulp(v):
    """half a bfloat16 ulp of every value (8 significand bits): 2^(floor(log2 |v|) - 8), the most the final rounding of a bfloat16
    gradient value can move it; relative to the value it lies between 2^-9 (below a power of two) and 2^-8 (just above one)"""
    _, e = np.frexp(np.abs(v))  # |v| = m * 2^e, m in [0.5, 1)
    return np.where(v == 0, 0.0, np.ldexp(1.0, e - 9))


@pytest.fixture(scope="module")
def refs():
    """float64 restatement of every case, on its float32 logits and on their bfloat16 rounding; computed once"""
    out = {}
    for c in CASES:
        zb = torch.from_numpy(c["z"]).bfloat16().float().numpy()
        out[c["name"]] = {torch.float32: R.fgdm_loss_ref(c["z"], c["maps"], c["num_bins"]),
                          torch.bfloat16: R.fgdm_loss_ref(zb, c["maps"], c["num_bins"])}
    return out


def run(case, dtype, channels_last, upstream=None, **kw):
    z = torch.from_numpy(case["z"]).to(DEV).to(dtype)
    if channels_last:
        z = z.contiguous(memory_format=torch.channels_last)
    z.requires_grad_(True)
    maps = torch.from_numpy(case["maps"]).to(DEV)
    crit = PL.ForegroundDepthMapLoss(ARGS, num_bins=case["num_bins"], **kw)
    loss = crit(z, maps)
    tgt = PL.FgdmLossFn.last_targets
    if upstream is None:
        loss.backward()
    else:
        (loss * upstream).backward()
    torch.cuda.synchronize()
    return loss, z, tgt


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_loss_gradient_and_targets(case, dtype, channels_last, refs):
    ref_loss, ref_grad, ref_t = refs[case["name"]][dtype]
    loss, z, tgt = run(case, dtype, channels_last)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert z.grad.dtype == dtype and z.grad.stride() == z.stride()
    assert (tgt.cpu().numpy() == ref_t).all()
    got_loss, got = float(loss.detach()), z.grad.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got_loss) and np.isfinite(got).all()
    dl = abs(got_loss - ref_loss) / abs(ref_loss)
    err = np.abs(got - ref_grad)
    print(f"{case['name']} {dtype} nhwc={channels_last}: loss distance {dl:.3e}, gradient distance {err.max() / np.abs(ref_grad).max():.3e}")
    assert dl <= LOSS_TOL
    tol = GRAD_TOL * np.abs(ref_grad).max()
    if dtype == torch.bfloat16:
        tol = tol + bf16_half_ulp(ref_grad)
    assert (err <= tol).all(), f"gradient off by {float((err - tol).max()):.3e} beyond the bound"


def test_same_bits_on_every_run():
    c = CASES[0]
    a, za, _ = run(c, torch.float32, False)
    b, zb, _ = run(c, torch.float32, False)
    assert a.view(torch.int32).item() == b.view(torch.int32).item()
    assert torch.equal(za.grad, zb.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_scales_the_stored_gradient(dtype):
    c = CASES[0]
    _, z1, _ = run(c, dtype, False)
    _, z2, _ = run(c, dtype, False, upstream=2.5)
    assert torch.equal(z2.grad.float(), (z1.grad.float() * 2.5).to(dtype).float())


def test_float64_maps_and_other_parameters():
    """a float64 map (the reference's dtype) bins as its float64 values; gamma 0, gamma 1.5 and other weights follow the restatement"""
    c = CASES[4]  # the bin edges
    m64 = c["maps"].astype(np.float64) + 1e-9  # not float32 values: an edge depth moves to the upper side
    z = torch.from_numpy(c["z"]).to(DEV).requires_grad_(True)
    loss = PL.ForegroundDepthMapLoss(ARGS, num_bins=c["num_bins"])(z, torch.from_numpy(m64).to(DEV))
    ref_loss, _, ref_t = R.fgdm_loss_ref(c["z"], m64, c["num_bins"])
    assert (PL.FgdmLossFn.last_targets.cpu().numpy() == ref_t).all()
    assert abs(float(loss.detach()) - ref_loss) <= LOSS_TOL * abs(ref_loss)
    c = CASES[0]
    for kw in (dict(gamma=0.0), dict(gamma=1.5, alpha=0.5), dict(fg_weight=3.0, bg_weight=0.5)):
        ref_loss, ref_grad, _ = R.fgdm_loss_ref(c["z"], c["maps"], c["num_bins"], **kw)
        loss, z, _ = run(c, torch.float32, False, **kw)
        assert abs(float(loss.detach()) - ref_loss) <= LOSS_TOL * abs(ref_loss), kw
        assert R.rel_max(z.grad.cpu().numpy(), ref_grad) <= GRAD_TOL, kw


def test_refusals_before_any_launch():
    c = CASES[0]
    crit = PL.ForegroundDepthMapLoss(ARGS)
    z = torch.from_numpy(c["z"])
    maps = torch.from_numpy(c["maps"])
    PL.FgdmLossFn.last_targets = None
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        crit(z, maps)  # logits on the host
    zd, md = z.to(DEV), maps.to(DEV)
    with pytest.raises(ValueError, match="channels"):
        crit(zd[:, :80], md)
    with pytest.raises(ValueError, match="H // 16"):
        crit(zd[:, :, :2], md)
    with pytest.raises(ValueError, match="H // 16"):
        crit(zd, md[:, :, :64])
    with pytest.raises(ValueError, match="floating"):
        crit(zd, md.to(torch.int32))
    with pytest.raises(y3d.Y3DError, match="float32 or bfloat16"):
        crit(zd.half(), md)
    with pytest.raises(ValueError, match="gamma"):
        PL.ForegroundDepthMapLoss(ARGS, gamma=0.5)
    with pytest.raises(ValueError, match="num_bins"):
        PL.ForegroundDepthMapLoss(ARGS, num_bins=256)
    assert PL.FgdmLossFn.last_targets is None  # nothing ran
    # a model carries its args
    assert PL.ForegroundDepthMapLoss(SimpleNamespace(args=ARGS)).dmax == R.DMAX
