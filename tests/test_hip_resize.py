"""GPU: the bilinear resize kernels of csrc/resize.hip (ops.resize_bilinear / ops.resize_bilinear_adjoint) against the float64 rule of
tests/depth_predictor_ref.py (`bil_matrix`: ATen's align_corners=False indices and weights in float32, the interpolation in float64).

Bound: 2 float32 ulps of the largest input for float32 maps, 1 bfloat16 ulp of the largest input for bfloat16 maps (the kernel computes
in float32 and rounds once), forward and adjoint alike."""
import numpy as np
import pytest
import torch

from conftest import has_gpu

import depth_predictor_ref as R
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import Y3DError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV = "cuda"
SIZES = (((3, 5), (6, 10)), ((3, 4), (5, 7)), ((1, 1), (2, 2)), ((7, 4), (13, 7)))
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]


def ulp(v, dtype):
    """one unit in the last place of |v| in `dtype`"""
    _, e = np.frexp(abs(float(v)))
    return float(np.ldexp(1.0, e - 1 - (23 if dtype == torch.float32 else 7)))


def bound(largest, dtype):
    return (2 if dtype == torch.float32 else 1) * ulp(largest, dtype)


def draw(shape, dtype, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return x.bfloat16().float() if dtype == torch.bfloat16 else x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 128])
@pytest.mark.parametrize("src,dst", SIZES, ids=IDS)
def test_forward_and_adjoint(src, dst, C, dtype):
    x, cot = draw((2, C, *src), dtype, 1), draw((2, C, *dst), dtype, 2)
    y = ops.resize_bilinear(ops.to_nhwc(x.to(DEV), dtype), dst)
    dx = ops.resize_bilinear_adjoint(ops.to_nhwc(cot.to(DEV), dtype, dense=True), src)
    assert y.shape == (2, C, *dst) and dx.shape == (2, C, *src) and y.dtype == dtype and dx.dtype == dtype and ops.is_nhwc(y) and ops.is_nhwc(dx)
    ef = float((y.float().cpu().double() - R.resize(x.double(), dst)).abs().max())
    eb = float((dx.float().cpu().double() - R.resize_adj(cot.double(), src)).abs().max())
    bf, bb = bound(x.abs().max(), dtype), bound(cot.abs().max(), dtype)
    print(f"{src}->{dst} C {C} {dtype}: forward {ef:.3e} (bound {bf:.3e}), adjoint {eb:.3e} (bound {bb:.3e})")
    assert ef <= bf and eb <= bb


@pytest.mark.parametrize("src,dst", SIZES, ids=IDS)
def test_impulses_at_the_borders(src, dst):
    """an impulse at every corner and edge centre of the input (forward) and of the output (adjoint): the support of the result is the
    rule's, exactly - an index clamped wrongly at a border moves or drops a value - and the values are the rule's weights"""
    ry, rx = R.bil_matrix(src[0], dst[0]), R.bil_matrix(src[1], dst[1])

    def spots(h, w):
        return sorted({(i, j) for i in (0, h // 2, h - 1) for j in (0, w // 2, w - 1)})

    for (i, j) in spots(*src):
        x = torch.zeros(1, 8, *src)
        x[0, :, i, j] = 1.0
        y = ops.resize_bilinear(ops.to_nhwc(x.to(DEV), torch.float32), dst).cpu().double()[0, 0].numpy()
        want = np.outer(ry[:, i], rx[:, j])
        assert np.array_equal(y != 0, want != 0), f"forward support of an impulse at {(i, j)}"
        assert np.abs(y - want).max() <= 2.0 ** -23
    for (i, j) in spots(*dst):
        c = torch.zeros(1, 8, *dst)
        c[0, :, i, j] = 1.0
        dx = ops.resize_bilinear_adjoint(ops.to_nhwc(c.to(DEV), torch.float32, dense=True), src).cpu().double()[0, 0].numpy()
        want = np.outer(ry[i], rx[j])
        assert np.array_equal(dx != 0, want != 0), f"adjoint support of an impulse at {(i, j)}"
        assert np.abs(dx - want).max() <= 2.0 ** -23


def test_strided_input_same_bits_and_refusals():
    x = draw((2, 16, 7, 4), torch.bfloat16, 3).to(DEV).bfloat16()
    wide = ops.nhwc_empty(2, 32, 7, 4, torch.bfloat16, DEV)
    wide.fill_(9.0)
    wide[:, 8:24].copy_(x)
    a = ops.resize_bilinear(ops.to_nhwc(x, torch.bfloat16), (13, 7))
    b = ops.resize_bilinear(wide[:, 8:24], (13, 7))  # a channel slice of a wider map: explicit pixel stride
    assert torch.equal(a, b) and torch.equal(a, ops.resize_bilinear(ops.to_nhwc(x, torch.bfloat16), (13, 7)))
    y = ops.ResizeBilinearFn.apply(ops.to_nhwc(x, torch.bfloat16).requires_grad_(True), (13, 7))
    assert y.requires_grad
    with pytest.raises(Y3DError, match="no CPU fallback"):
        ops.resize_bilinear(torch.zeros(1, 8, 3, 3), (6, 6))
    with pytest.raises(Y3DError, match="multiple of 8"):
        ops.resize_bilinear(ops.to_nhwc(torch.zeros(1, 4, 3, 3, device=DEV), torch.float32), (6, 6))
