"""Host: the fp8 data gradient's interface, its weight-layout convention and the scale-folding identity (no GPU).

The GPU tests (test_hip_fp8_dgrad.py) compare y3d_fp8_pack_weight_dgrad's bytes against `fp8_dgrad_ref.pack_dgrad_ref`; here that
restatement is itself pinned against torch.nn.grad.conv2d_input on integer data in float64."""
import os
import re

import pytest
import torch

from conftest import ROOT
from fp8_dgrad_ref import e4m3_value, multiply_out, pack_dgrad_ref
from oracle import restate as RS  # the checker

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib, ops

NEW = ("y3d_fp8_quantize_grad", "y3d_fp8_pack_weight_dgrad", "y3d_conv3x3_fp8_dgrad_ok", "y3d_conv3x3_fp8_dgrad")


def test_header_declares_the_entry_points_and_the_switch_follows_the_fp8_modes():
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "y3d.h")).read(), flags=re.S)
    protos = _lib.parse_header()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/y3d.h"
        assert name in protos
        assert hasattr(y3d.lib()._dll, name), f"{name} is not exported"
    assert len(protos["y3d_conv3x3_fp8_dgrad"][1]) == 16 and len(protos["y3d_conv3x3_fp8_dgrad_ok"][1]) == 6
    assert ops.fp8_dgrad() is False and y3d.fp8_dgrad() is False  # default off
    try:
        with pytest.raises(ValueError):
            ops.set_fp8_dgrad(True)  # no fp8 convolutions
        y3d.set_weight_quant("fp8")
        with pytest.raises(ValueError):
            y3d.set_fp8_dgrad(True)  # fp8 weights alone are not enough
        y3d.set_fp8_conv(True)
        y3d.set_fp8_dgrad(True)
        assert ops.fp8_dgrad() is True
        y3d.set_fp8_conv(False)
        assert ops.fp8_dgrad() is False, "switching the fp8 convolutions off must clear the data-gradient switch"
        y3d.set_fp8_conv(True)
        y3d.set_fp8_dgrad(True)
        y3d.set_weight_quant(None)
        assert ops.fp8_dgrad() is False, "switching the fp8 weights off must clear the data-gradient switch"
    finally:
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)


def test_geometry_rule_is_the_forward_rule_with_the_roles_swapped():
    L = y3d.lib()
    ok = L.conv3x3_fp8_dgrad_ok
    assert ok(32, 80, 80, 128, 2048, 1) and ok(32, 80, 80, 2048, 2048, 16) and ok(4, 20, 20, 128, 128, 1) and ok(5, 4, 8, 16, 128, 1)
    assert not ok(4, 20, 20, 96, 96, 1) and not ok(4, 20, 20, 128, 64, 1) and not ok(4, 20, 20, 256, 128, 2)
    assert not ok(4, 3, 8, 128, 128, 1) and not ok(4, 4, 7, 128, 128, 1), "maps smaller than 4 x 8 are refused"
    for B, H, W, Cin, Cout, g in [(2, 16, 24, 320, 256, 1), (1, 8, 16, 384, 96, 2), (3, 12, 40, 1024, 1024, 8), (2, 24, 24, 128, 2048, 1), (2, 9, 9, 136, 128, 1)]:
        assert bool(ok(B, H, W, Cin, Cout, g)) == bool(L.conv3x3_fp8_ok(B, H, W, Cout, Cin, g))


@pytest.mark.parametrize("case", [(2, 8, 12, 1, 0, None), (1, 8, 16, 2, 0, None), (2, 32, 32, 16, 0, None), (2, 4, 24, 1, 8, 20)],
                         ids=["g1", "g2", "g16", "window"])
def test_pack_restatement_multiplied_out_is_the_data_gradient(case):
    B, Cin, Cout, g, lo, hi = case
    hi = Cout if hi is None else hi
    torch.manual_seed(Cin + Cout + g)
    H, W = 5, 7
    w = torch.randint(-4, 5, (Cout, Cin // g, 3, 3)).double()
    dy = torch.randint(-3, 4, (B, Cout, H, W)).double()
    packed = pack_dgrad_ref(w.numpy(), g, lo, hi)
    assert packed.shape == (g, Cin // g, 9, (hi - lo) // g)
    want = torch.nn.grad.conv2d_input((B, Cin, H, W), w[lo:hi], dy[:, lo:hi], 1, 1, 1, g)
    got = multiply_out(dy[:, lo:hi], packed)
    assert torch.equal(got, want)
    # a permutation of the bytes: nothing is lost or duplicated
    idx = torch.arange(Cout * (Cin // g) * 9).reshape(Cout, Cin // g, 3, 3).numpy()
    p = pack_dgrad_ref(idx, g, lo, hi).reshape(-1)
    assert len(set(p.tolist())) == p.size == (hi - lo) * (Cin // g) * 9


@pytest.mark.parametrize("groups", [1, 4])
def test_power_of_two_row_scales_fold_exactly_into_dy(groups):
    """dx = sum_c dy[c] * (scale_c * value(code_c)) = sum_c (dy[c] * scale_c) * value(code_c): exact term by term when scale_c is a power of two"""
    torch.manual_seed(3 + groups)
    B, Cin, Cout, H, W = 2, 16, 32, 6, 9
    w = torch.randn(Cout, Cin // groups, 3, 3) * torch.exp2(torch.randint(-10, 3, (Cout, 1, 1, 1)).float())
    codes, scale, w_eff = RS.fp8w_quantize(w)
    assert torch.equal(torch.exp2(torch.log2(scale).round()), scale), "the fp8w row scales are powers of two"
    val = e4m3_value(codes.numpy()).reshape(w.shape)
    assert torch.equal(val * scale.double().view(-1, 1, 1, 1), w_eff.double())
    dy = (torch.randn(B, Cout, H, W) * torch.exp(torch.randn(B, 1, H, W) * 2) * 1e-4).to(torch.bfloat16).double()
    a = torch.nn.grad.conv2d_input((B, Cin, H, W), w_eff.double(), dy, 1, 1, 1, groups)
    b = torch.nn.grad.conv2d_input((B, Cin, H, W), val, dy * scale.double().view(1, -1, 1, 1), 1, 1, 1, groups)
    # every product is the same real number on both sides (a power of two moved from one factor to the other); the float64 sums see the
    # same terms in the same order
    assert torch.equal(a, b)
    # and through the packed layout
    c = multiply_out(dy * scale.double().view(1, -1, 1, 1), e4m3_value(pack_dgrad_ref(codes.numpy(), groups)).numpy())
    assert torch.allclose(c, a, rtol=1e-12, atol=0)
