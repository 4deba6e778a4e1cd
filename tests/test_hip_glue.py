"""The NHWC graph glue (csrc/misc.hip) kernel by kernel against the host references of tail_ref.py: y3d_maxpool_fwd / _bwd,
y3d_upsample2x_fwd / _bwd, y3d_copy2d, y3d_add2d, y3d_nchw_to_nhwc, y3d_nhwc_to_nchw - all to BIT equality.

* layout "strided": every input is a row / column crop and channel slice of a wider buffer holding other values (distinct batch,
  row and pixel strides), every output a channel slice of a wider sentinel-filled buffer, as SPPF, C2f, PSA and the cross-layer
  concat placement of ops.py use the kernels; layout "dense": pixel stride == C;
* every output buffer is pre-filled with a sentinel and has guard space behind it: everything that must be written was written,
  the neighbour channels on both sides of the slice and the guard still hold the sentinel;
* gradients and sums use operands whose fp32 accumulation is exact, so the result must equal the exact value rounded ONCE to the
  storage type.
tests/test_tail_ref_host.py pins the references and checks from these case lists that they still reach every path."""
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32

import tail_ref as R
from test_hip_eval_tail import CE, TDT, _ids, assert_bits

DEV = "cuda"
MISC_CAP = 4096 * 256  # misc.hip ew_grid: at most 4 096 blocks of 256 threads


def out_slice(P, C, dt, lay):
    """(buffer, (P, C) view): a sentinel-filled [P][C + 2 chunks] buffer with the slice one chunk in ("strided") or [P][C]
    ("dense"), plus a guard behind it"""
    ce = CE[dt]
    sw = C + 2 * ce if lay == "strided" else C
    buf = R.sentinel(P * sw + 256, TDT[dt], DEV)
    off = ce if lay == "strided" else 0
    return buf, buf[:P * sw].view(P, sw)[:, off:off + C]


def check_slice(buf, view, what):
    """everything inside the slice written, everything else in the buffer untouched"""
    assert not bool(R.untouched(view).any()), f"{what}: {int(R.untouched(view).sum())} elements were never written"
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    P, C = view.shape
    sw = view.stride(0)
    mask[:P * sw].view(P, sw)[:, view.storage_offset():view.storage_offset() + C] = False
    assert bool(R.untouched(buf)[mask].all()), f"{what}: a store left the output slice"


def in_map(x, lay, dt, gen):
    """device copy of the host (B, H, W, C) tensor: dense, or a crop + channel slice with three distinct strides"""
    B, H, W, C = x.shape
    if lay == "dense":
        return x.to(DEV).contiguous()
    ce = CE[dt]
    buf = (torch.randn(B, H + 1, W + 2, C + 2 * ce, generator=gen) * 7).to(x.dtype)
    buf[:, 1:, 1:1 + W, ce:ce + C] = x
    v = buf.to(DEV)[:, 1:, 1:1 + W, ce:ce + C]
    assert v.stride(0) != H * v.stride(1) and v.stride(1) != W * v.stride(2) and v.stride(2) != C
    return v


def in_rows(x, extra, gen):
    """device copy of the host (P, C) tensor as the channel slice [extra, extra + C) of a [P][C + 2 * extra] buffer of other values"""
    P, C = x.shape
    buf = (torch.randn(P, C + 2 * extra, generator=gen) * 7).to(x.dtype)
    buf[:, extra:extra + C] = x
    return buf.to(DEV)[:, extra:extra + C]


def grid_values(shape, gen, step, dtype):
    return (torch.round(torch.randn(shape, generator=gen) / step) * step).to(dtype)


# ---------------------------------------------------------------------------------------------------------------- max pool
# (dtype, B, H, W, C, k, values, layout); k > map on (1, 1) and (2, 7)
MP_CASES = [
    (BF16, 2, 1, 1, 8, 3, "grid", "strided"),
    (F32, 2, 1, 1, 4, 15, "neginf", "strided"),
    (BF16, 2, 2, 7, 16, 5, "grid", "dense"),
    (F32, 2, 2, 7, 72, 9, "neginf", "strided"),
    (BF16, 2, 2, 7, 72, 15, "grid", "strided"),
    (BF16, 2, 13, 17, 72, 5, "neginf", "strided"),
    (F32, 2, 13, 17, 16, 3, "grid", "strided"),
    (BF16, 1, 13, 17, 8, 9, "nan", "strided"),
    (F32, 1, 13, 17, 4, 15, "grid", "dense"),
    (BF16, 2, 20, 20, 16, 5, "grid", "strided"),
    (F32, 2, 20, 20, 72, 5, "neginf", "strided"),
    (BF16, 1, 20, 20, 8, 15, "neginf", "strided"),
    (F32, 1, 20, 20, 16, 9, "nan", "strided"),
    (BF16, 2, 20, 20, 72, 3, "grid", "dense"),
]


def mp_input(case):
    """values on a grid of 1/4 (most windows hold several maxima); "neginf": a fifth of the entries -inf and the top-left k x k block
    of the even channels all -inf (windows of -inf only, on the border and inside); "nan": a sprinkling of NaNs as well"""
    dt, B, H, W, C, k, val, lay = case
    gen = torch.Generator().manual_seed(H * W + C + k)
    x = grid_values((B, H, W, C), gen, 0.25, TDT[dt])
    if val in ("neginf", "nan"):
        x[torch.rand(B, H, W, C, generator=gen) < 0.2] = float("-inf")
        x[:, :k, :k, ::2] = float("-inf")
    if val == "nan":
        x[torch.rand(B, H, W, C, generator=gen) < 0.03] = float("nan")
    dy = torch.randint(-3, 4, (B, H, W, C), generator=gen).to(TDT[dt])
    return x, dy, gen


def assert_bits_nan(got, want, what):
    """bit equality where the expected value is a number, a NaN (any payload) where it is a NaN"""
    got, want = got.cpu(), want.cpu()
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), f"{what}: NaNs are not where the reference has them"
    assert_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", MP_CASES, ids=_ids(MP_CASES))
def test_maxpool_forward_argmax_backward_exact(case):
    """forward bit-equal (NaN propagates), arg-max = the first maximum in row-then-column scan order (the last NaN; the first
    in-map tap of a window of -inf only, as ATen), backward = the exact sum of integer gradients rounded once; through the C ABI
    with slices on both sides and through ops.MaxPoolFn"""
    dt, B, H, W, C, k, val, lay = case
    L, st = y3d.lib(), ops.stream()
    x, dy, gen = mp_input(case)
    y_ref, a_ref = R.maxpool_fwd(x, k)
    dx_ref = R.rnd(R.maxpool_bwd(dy.double(), a_ref, k), TDT[dt]).to(TDT[dt])
    P = B * H * W
    xd = in_map(x, lay, dt, gen)
    ybuf, y = out_slice(P, C, dt, lay)
    abuf = R.sentinel(P * C + 256, torch.uint8, DEV)
    L.maxpool_fwd(dt, xd.data_ptr(), xd.stride(0), xd.stride(1), xd.stride(2), y.data_ptr(), y.stride(0), abuf.data_ptr(), B, H, W, C, k, st)
    torch.cuda.synchronize()
    check_slice(ybuf, y, "maxpool_fwd y")
    assert bool(R.untouched(abuf[P * C:]).all()), "maxpool_fwd: a store went past the end of argmax"
    assert_bits_nan(y.reshape(B, H, W, C), y_ref, f"maxpool_fwd {case}")
    assert_bits(abuf[:P * C].view(B, H, W, C), a_ref, f"maxpool argmax {case}")
    dyd = in_rows(dy.reshape(P, C), CE[dt] if lay == "strided" else 0, gen)
    dbuf, dx = out_slice(P, C, dt, lay)
    L.maxpool_bwd(dt, dyd.data_ptr(), dyd.stride(0), abuf.data_ptr(), dx.data_ptr(), dx.stride(0), B, H, W, C, k, st)
    torch.cuda.synchronize()
    check_slice(dbuf, dx, "maxpool_bwd dx")
    assert_bits(dx.reshape(B, H, W, C), dx_ref, f"maxpool_bwd {case}")
    # the autograd function SPPF uses
    old = ops.compute_dtype()
    y3d.set_compute_dtype(TDT[dt])
    try:
        xa = xd.permute(0, 3, 1, 2).detach().requires_grad_(True)
        ya = ops.MaxPoolFn.apply(xa, k)
        ya.backward(dy.to(DEV).permute(0, 3, 1, 2))
        torch.cuda.synchronize()
    finally:
        y3d.set_compute_dtype(old)
    assert_bits_nan(ya.detach().permute(0, 2, 3, 1), y_ref, f"MaxPoolFn forward {case}")
    assert_bits(xa.grad.permute(0, 2, 3, 1), dx_ref, f"MaxPoolFn backward {case}")


# ---------------------------------------------------------------------------------------------------------------- upsample
# (dtype, B, H, W, C, layout)
UP_CASES = [
    (BF16, 2, 1, 1, 8, "strided"),
    (F32, 2, 1, 1, 72, "strided"),
    (BF16, 2, 3, 5, 72, "strided"),
    (F32, 2, 3, 5, 4, "dense"),
    (BF16, 2, 3, 5, 16, "dense"),
    (F32, 2, 20, 20, 16, "strided"),
    (BF16, 2, 20, 20, 72, "strided"),
    (F32, 1, 20, 20, 72, "strided"),
    (BF16, 1, 20, 20, 8, "strided"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", UP_CASES, ids=_ids(UP_CASES))
def test_upsample2x_forward_backward_exact(case):
    """forward bit-equal to y[h][w] = x[h // 2][w // 2]; backward on integer gradients up to 200 (exact in bf16, their sums of
    four are not) = the exact sum rounded once; dy is a crop + slice with distinct batch, row and pixel strides"""
    dt, B, H, W, C, lay = case
    L, st = y3d.lib(), ops.stream()
    gen = torch.Generator().manual_seed(H * W + C)
    x = (torch.randn(B, H, W, C, generator=gen) * 3).to(TDT[dt])
    dy = torch.randint(-200, 201, (B, 2 * H, 2 * W, C), generator=gen).to(TDT[dt])
    dx_ref = R.rnd(R.upsample2x_bwd(dy.double()), TDT[dt]).to(TDT[dt])
    xd = in_map(x, lay, dt, gen)
    ybuf, y = out_slice(B * 4 * H * W, C, dt, lay)
    L.upsample2x_fwd(dt, xd.data_ptr(), xd.stride(0), xd.stride(1), xd.stride(2), y.data_ptr(), y.stride(0), B, H, W, C, st)
    torch.cuda.synchronize()
    check_slice(ybuf, y, "upsample2x_fwd")
    assert_bits(y.reshape(B, 2 * H, 2 * W, C), R.upsample2x_fwd(x), f"upsample2x_fwd {case}")
    dyd = in_map(dy, lay, dt, gen)
    dbuf, dx = out_slice(B * H * W, C, dt, lay)
    L.upsample2x_bwd(dt, dyd.data_ptr(), dyd.stride(0), dyd.stride(1), dyd.stride(2), dx.data_ptr(), dx.stride(0), B, H, W, C, st)
    torch.cuda.synchronize()
    check_slice(dbuf, dx, "upsample2x_bwd")
    assert_bits(dx.reshape(B, H, W, C), dx_ref, f"upsample2x_bwd {case}")
    old = ops.compute_dtype()
    y3d.set_compute_dtype(TDT[dt])
    try:
        xa = xd.permute(0, 3, 1, 2).detach().requires_grad_(True)
        ya = ops.Upsample2xFn.apply(xa)
        ya.backward(dyd.permute(0, 3, 1, 2))
        torch.cuda.synchronize()
    finally:
        y3d.set_compute_dtype(old)
    assert_bits(ya.detach().permute(0, 2, 3, 1), R.upsample2x_fwd(x), f"Upsample2xFn forward {case}")
    assert_bits(xa.grad.permute(0, 2, 3, 1), dx_ref, f"Upsample2xFn backward {case}")


# ---------------------------------------------------------------------------------------------------------------- copy2d / add2d
# (dtype, P, C, layout); strided: every operand has its own pixel stride
CP_CASES = [
    (BF16, 1, 8, "strided"),
    (F32, 1, 24, "strided"),
    (BF16, 77, 24, "strided"),
    (F32, 77, 4, "strided"),
    (BF16, 77, 520, "strided"),
    (F32, 77, 520, "dense"),
    (F32, 1, 520, "strided"),
    (BF16, 349600, 24, "strided"),  # 1 048 800 chunks: past the 4 096-block cap
]


def cp_chunks(case):
    dt, P, C, lay = case
    return P * (C // CE[dt])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CP_CASES, ids=_ids(CP_CASES))
def test_copy2d_bit_equal(case):
    """a [P][C] slice copied into a slice of another pixel stride with sentinel channels on both sides"""
    dt, P, C, lay = case
    gen = torch.Generator().manual_seed(P + C)
    x = (torch.randn(P, C, generator=gen) * 3).to(TDT[dt])
    xd = in_rows(x, 2 * CE[dt] if lay == "strided" else 0, gen)
    buf, y = out_slice(P, C, dt, lay)
    assert lay == "dense" or len({xd.stride(0), y.stride(0), C}) == 3
    y3d.lib().copy2d(dt, xd.data_ptr(), xd.stride(0), y.data_ptr(), y.stride(0), P, C, ops.stream())
    torch.cuda.synchronize()
    check_slice(buf, y, "copy2d")
    assert_bits(y, x, f"copy2d {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CP_CASES, ids=_ids(CP_CASES))
def test_add2d_exact_out_of_place_and_in_place(case):
    """operands on the grid k / 64, |k| <= 512, stored in the storage type: every fp32 sum is exact, the result is the exact sum
    rounded once; out of place with three distinct pixel strides, and in place (y aliasing a) as ops.py calls it"""
    dt, P, C, lay = case
    L, st = y3d.lib(), ops.stream()
    gen = torch.Generator().manual_seed(P + C + 1)
    a = (torch.randint(-512, 513, (P, C), generator=gen).double() / 64).to(TDT[dt])
    b = (torch.randint(-512, 513, (P, C), generator=gen).double() / 64).to(TDT[dt])
    want = R.rnd(a.double() + b.double(), TDT[dt]).to(TDT[dt])
    ad = in_rows(a, 2 * CE[dt] if lay == "strided" else 0, gen)
    bd = in_rows(b, 3 * CE[dt] if lay == "strided" else 0, gen)
    buf, y = out_slice(P, C, dt, lay)
    assert lay == "dense" or len({ad.stride(0), bd.stride(0), y.stride(0), C}) == 4
    L.add2d(dt, ad.data_ptr(), ad.stride(0), bd.data_ptr(), bd.stride(0), y.data_ptr(), y.stride(0), P, C, st)
    torch.cuda.synchronize()
    check_slice(buf, y, "add2d")
    assert_bits(y, want, f"add2d {case}")
    ibuf, ia = out_slice(P, C, dt, lay)
    ia.copy_(a.to(DEV))
    L.add2d(dt, ia.data_ptr(), ia.stride(0), bd.data_ptr(), bd.stride(0), ia.data_ptr(), ia.stride(0), P, C, st)
    torch.cuda.synchronize()
    check_slice(ibuf, ia, "add2d in place")
    assert_bits(ia, want, f"add2d in place {case}")


# ---------------------------------------------------------------------------------------------------------------- layout
# (dtype, B, C, H, W, Cpad, layout of the NHWC side of nhwc_to_nchw)
NH_CASES = [
    (BF16, 2, 1, 5, 7, 1, "strided"),
    (F32, 2, 3, 5, 7, 3, "dense"),
    (BF16, 2, 3, 7, 9, 8, "strided"),
    (F32, 2, 5, 5, 7, 8, "strided"),
    (BF16, 2, 5, 7, 9, 16, "dense"),
    (F32, 2, 1, 3, 5, 16, "strided"),
    (BF16, 2, 5, 5, 7, 5, "strided"),
    (F32, 2, 3, 7, 9, 16, "strided"),
    (BF16, 1, 1, 7, 9, 8, "dense"),
]


def special_f32(n, gen):
    """randn with, up front, values whose bf16 rounding is decided by the tie rule or the range: exact halfway cases towards an
    even and an odd neighbour, just above / below halfway, +-0, +-inf, the largest finite fp32, the smallest normal"""
    x = torch.randn(n, generator=gen) * 3
    sp = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 0.0, -0.0,
          float("inf"), float("-inf"), torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max, 2.0 ** -126, 255.5, 256.5]
    m = min(n, len(sp))
    x[:m] = torch.tensor(sp[:m], dtype=torch.float32)
    return x[torch.randperm(n, generator=gen)] if n > len(sp) else x


@pytest.mark.gpu
@pytest.mark.parametrize("case", NH_CASES, ids=_ids(NH_CASES))
def test_layout_conversions_bit_equal(case):
    """NCHW fp32 -> NHWC storage type with zero padding lanes (the bf16 rounding equals torch's on the CPU, ties, signed zeros,
    infinities and the overflow of the largest fp32 included) and back from a channel slice"""
    dt, B, C, H, W, Cpad, lay = case
    L, st = y3d.lib(), ops.stream()
    gen = torch.Generator().manual_seed(C * 100 + H * W + Cpad)
    x = special_f32(B * C * H * W, gen).view(B, C, H, W)
    n = B * H * W * Cpad
    buf = R.sentinel(n + 256, TDT[dt], DEV)
    L.nchw_to_nhwc(dt, x.to(DEV).data_ptr(), buf.data_ptr(), B, C, H, W, Cpad, st)
    torch.cuda.synchronize()
    assert bool(R.untouched(buf[n:]).all()) and not bool(R.untouched(buf[:n]).any())
    assert_bits(buf[:n].view(B, H, W, Cpad), R.nchw_to_nhwc(x, Cpad, TDT[dt]), f"nchw_to_nhwc {case}")
    xs = x.permute(0, 2, 3, 1).to(TDT[dt]).contiguous()
    xd = in_rows(xs.reshape(-1, C), 3 if lay == "strided" else 0, gen)
    m = B * C * H * W
    obuf = R.sentinel(m + 256, torch.float32, DEV)
    L.nhwc_to_nchw(dt, xd.data_ptr(), xd.stride(0), obuf.data_ptr(), B, C, H, W, st)
    torch.cuda.synchronize()
    assert bool(R.untouched(obuf[m:]).all()) and not bool(R.untouched(obuf[:m]).any())
    assert_bits(obuf[:m].view(B, C, H, W), R.nhwc_to_nchw(xs), f"nhwc_to_nchw {case}")
