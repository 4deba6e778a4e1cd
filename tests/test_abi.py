"""CPU: the C-ABI library loads and exports every symbol include/y3d.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib


def test_header_parses_and_library_exports_every_symbol():
    protos = _lib.parse_header()
    assert len(protos) >= 35
    src = open(os.path.join(ROOT, "include", "y3d.h")).read()
    declared = set(re.findall(r"\b(y3d_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", src, flags=re.S)))
    assert declared == set(protos), declared ^ set(protos)
    assert os.path.exists(_lib.LIB_PATH), "liby3d_hip.so missing: run __graft_entry__.build()"
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(dll, name), f"{name} declared in y3d.h but not exported"


def test_host_side_helpers_without_gpu():
    L = y3d.lib()
    assert L.abi_version() == 1
    assert L.conv_stat_blocks(32, 80, 80) == 1600
    assert L.conv_kpad(_lib.BF16, 27) == 32 and L.conv_kpad(_lib.F32, 27) == 28
    assert 1 <= L.conv2d_wgrad_splits(_lib.BF16, 32, 80, 80, 128, 128, 1, 3, 3) <= 256


def route_codes():
    """{name: code} of the Y3D_ROUTE_* enum, read from the header (the codes have no second definition)"""
    src = open(os.path.join(ROOT, "include", "y3d.h")).read()
    return {k: int(v) for k, v in re.findall(r"\bY3D_ROUTE_(\w+)\s*=\s*(\d+)", src)}


def test_conv2d_route_of_known_shapes():
    L, R = y3d.lib(), route_codes()
    bf, f32 = _lib.BF16, _lib.F32
    FWD, DGRAD, WGRAD = 0, 1, 2
    RAW, PART, AFF, RES, BIAS = 0, 1, 2, 3, 4
    cases = [
        # (dtype, op, epi, B, H, W, Cin, Cout, groups, k, stride, pad) -> route
        ((bf, FWD, AFF, 32, 80, 80, 2048, 2048, 16, 3, 1, 1), "WIDE3_16"),   # the roofline launch: 16 x (128 -> 128) @80x80
        ((bf, FWD, PART, 32, 80, 80, 2048, 2048, 16, 3, 1, 1), "WIDE3_16"),
        ((bf, DGRAD, RAW, 32, 80, 80, 2048, 2048, 16, 3, 1, 1), "WIDE3_16"),
        ((bf, FWD, AFF, 32, 40, 40, 2048, 2048, 16, 3, 1, 1), "FLAT"),
        ((bf, FWD, AFF, 32, 40, 40, 128, 128, 1, 3, 1, 1), "TILE8"),         # 120 persistent tiles: the 256-pixel tiles fill the chip
        ((f32, FWD, AFF, 32, 80, 80, 128, 128, 1, 3, 1, 1), "TILE16"),
        ((bf, FWD, AFF, 4, 80, 80, 64, 64, 1, 3, 1, 1), "SMALL"),
        ((bf, FWD, RES, 4, 80, 80, 64, 64, 1, 3, 1, 1), "SMALL"),
        ((bf, FWD, BIAS, 4, 80, 80, 64, 64, 1, 3, 1, 1), "GENERIC"),          # no bias epilogue on the narrow kernel
        ((bf, FWD, AFF, 32, 640, 640, 8, 16, 1, 3, 2, 1), "SMALL_S2"),
        ((bf, FWD, AFF, 32, 80, 80, 128, 128, 1, 1, 1, 0), "STREAM1X1"),
        ((bf, FWD, AFF, 1600, 5, 5, 512, 896, 1, 3, 1, 0), "GENERIC"),        # the sparse head's unpadded patch conv
        ((bf, DGRAD, RAW, 32, 80, 80, 64, 128, 1, 3, 2, 1), "S2_DGRAD"),
        ((bf, WGRAD, RAW, 4, 80, 80, 64, 64, 1, 3, 1, 1), "WGRAD_SMALL"),
        ((bf, WGRAD, RAW, 32, 80, 80, 128, 128, 1, 3, 1, 1), "WGRAD_TILE"),
        ((bf, WGRAD, RAW, 32, 80, 80, 128, 256, 1, 1, 1, 0), "WGRAD_STREAM1X1"),
        ((f32, WGRAD, RAW, 32, 80, 80, 128, 128, 1, 3, 1, 1), "GENERIC"),
    ]
    for (dt, op, epi, B, H, W, Cin, Cout, g, k, s, p), want in cases:
        got = L.conv2d_route(dt, op, epi, B, H, W, Cin, Cout, g, k, k, s, p)
        name = {v: n for n, v in R.items()}.get(got, got)
        assert got == R[want], f"route of {(dt, op, epi, B, H, W, Cin, Cout, g, k, s, p)}: {name}, expected {want}"
    # refusals: a residual epilogue only on the narrow kernel; channels the 16-byte chunks cannot carry; a bad op
    assert L.conv2d_route(bf, FWD, RES, 4, 80, 80, 128, 128, 1, 3, 3, 1, 1) < 0
    assert L.conv2d_route(bf, FWD, AFF, 4, 80, 80, 12, 16, 1, 3, 3, 1, 1) < 0 and "multiple" in L.last_error()
    assert L.conv2d_route(bf, 3, 0, 4, 80, 80, 64, 64, 1, 3, 3, 1, 1) < 0
    # the A/B knobs take their kernels out of the choice
    old = L.set_tile_kernels(0)
    try:
        assert L.conv2d_route(bf, FWD, AFF, 32, 80, 80, 2048, 2048, 16, 3, 3, 1, 1) == R["GENERIC"]
    finally:
        L.set_tile_kernels(old)
    old = L.set_stream1x1(0)
    try:
        assert L.conv2d_route(bf, FWD, AFF, 4, 80, 80, 64, 64, 1, 3, 3, 1, 1) == R["TILE16"]  # (the narrow kernel shares the knob)
        assert L.conv2d_route(bf, FWD, AFF, 32, 80, 80, 128, 128, 1, 1, 1, 1, 0) == R["GENERIC"]
    finally:
        L.set_stream1x1(old)


def test_invalid_arguments_raise_python_exceptions():
    L = y3d.lib()
    with pytest.raises(y3d.Y3DError, match="dtype"):
        L.conv2d_fwd(7, None, 0, 0, 0, 1, 8, 8, 8, None, None, None, 8, 8, 8, 8, 1, 3, 3, 1, 1, None, None)
    with pytest.raises(y3d.Y3DError, match="multiple"):
        L.conv2d_fwd(_lib.BF16, None, 0, 0, 0, 1, 8, 8, 3, None, None, None, 8, 8, 8, 8, 1, 3, 3, 1, 1, None, None)
    with pytest.raises(y3d.Y3DError, match="unsupported head dims"):
        L.attn_fwd(_lib.F32, None, 0, None, 0, None, 1, 4, 1, 16, 32, 1.0, None)


def test_no_cpu_fallback():
    """no value of the path is ever computed on the host: the kernel wrappers raise for host tensors, and a MODULE handed one (the
    reference constructor's stride probe, nn/tasks.py:300-310) answers with a meta tensor - a shape without data"""
    import torch
    from yolov10_3d_amd import modules as M, ops
    m = M.Conv(8, 8, 3)
    x = torch.randn(1, 8, 4, 4)
    with pytest.raises(y3d.Y3DError):
        ops.ConvBNActFn.apply(x, m.conv.weight, m.bn.weight, m.bn.bias, None, 0, m)
    with pytest.raises(y3d.Y3DError):
        ops.conv_bn_act_eval(x, m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var, 3, 1, 1, 1, True, 1e-3)
    y = m(x)
    assert y.device.type == "meta" and tuple(y.shape) == (1, 8, 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        y.cpu()  # "Cannot copy out of meta tensor; no data!"


def test_no_kernel_needs_scratch():
    """Every HIP kernel of the library compiles without scratch (register spills / run-time indexed private arrays).  In the LDS-DMA
    pipelines (conv3x3_wide3, conv3x3_fp8, conv3x3_wgrad_tile, conv3x3_tile) a scratch reload is followed by `s_waitcnt vmcnt(0)`, which drains the
    prefetch of the next tile (conv3x3_wide3.hip header).  The numbers are the compiler's own resource report
    (`-Rpass-analysis=kernel-resource-usage`), recorded by csrc/build.py at every compile."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("y3d_build", os.path.join(ROOT, "yolov10-3d_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    usage = mod.resource_usage()
    hip = [s for s in mod.sources() if s.endswith(".hip")]
    assert set(hip) <= set(usage), f"no resource report for {set(hip) - set(usage)}"
    n = 0
    bad = []
    for src, kernels in usage.items():
        for name, u in kernels.items():
            n += 1
            if u.get("scratch", 0) != 0:
                bad.append((src, name, u))
    assert n >= 150, f"only {n} kernels reported"
    assert not bad, f"kernels with scratch: {bad}"
    # the headline kernel keeps its two-waves-per-SIMD register budget
    wide = {k: v for k, v in usage["conv3x3_wide3.hip"].items() if "conv3x3_wide3_kernel" in k}
    assert len(wide) == 4 and all(v["vgprs"] <= 256 for v in wide.values()), wide
    # ... and the fp8 MFMA kernel (245 registers with the accumulators tied through inline asm; the builtin form spilled 900 dwords)
    f8 = {k: v for k, v in usage["conv3x3_fp8.hip"].items() if "conv3x3_fp8_kernel" in k}
    assert len(f8) == 2 and all(v["vgprs"] <= 256 and v["scratch"] == 0 for v in f8.values()), f8
