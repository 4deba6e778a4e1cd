"""y3d_attn_fwd / y3d_attn_bwd (csrc/attn.hip) through the C ABI against the host references of proj_attn_ref.py, on every route:
"f32" the fp32 VALU kernels, "valu" the bf16 VALU kernels with the tile kernels switched off, "fallback" the bf16 VALU kernels
reached through the entry points' own alignment test, "mfma" the bf16 MFMA kernels; head dims 32/64 and 36/72.

Which route a call takes is decided on the host (attn.hip, y3d_attn_fwd / y3d_attn_bwd): MFMA iff bf16, tile kernels on, qsw % 4 ==
osw % 4 == 0 (backward: dsw and gsw too), qkv 16-byte and out (dout, dqkv) 8-byte aligned; `takes_mfma` restates that and every
case asserts it.  What the kernels load decides the layouts: the VALU kernels read and write element by element (any stride and
address); the MFMA kernels read 16-byte (8-byte at the kd = 36 tail) pieces of the q | k | v, out and dout rows and write 8-byte
pieces, all at offsets that are multiples of 4 elements from row starts that are multiples of 4 elements; dv_extra, lse and delta
are read and written element by element on every route.  Layouts: "dense" - every pixel stride equals its width; "strided" - every
operand is a column slice of a wider buffer (qsw = W + 8, osw = O + 8, dsw = O + 16, esw = O + 3, gsw = W + 24).  The fallback
route is reached with qsw = W + 10 ("strided": not a multiple of 4) or a qkv address 4 bytes off a 16-byte boundary ("dense").

Every output (out, lse, delta, dqkv) lives in a sentinel-filled buffer with guard rows before and after: everything inside the
slice was written, nothing outside was touched.

EXACT cases (proj_attn_ref.attn_exact): keys are distinct +-1 vectors, q_i = 64 k_pi(i), scale = 1, v / dout / dv_extra integers.
Scores are integers up to 2048 (kd = 32) / 2304 (kd = 36): without the max subtraction exp overflows to inf.  The winner leads by
>= 128 and exp(-128) = 0 in fp32, so p is exactly one-hot, the sum exactly 1, and every route must return out_i = v_pi(i),
lse_i = 64 kd, delta_i = dout_i . out_i, dq = dk = 0, dv_j = dout_{pi^-1(j)} + dv_extra_j BIT for bit (up to the sign of zero).
pi differs per (image, head) and moves every query, so a wrong key, query, head or image index, a key permuted inside an MFMA
k-step or a row misplaced in a swizzled LDS image returns another row's integers.

REAL-valued cases: bf16-representable randn inputs (and q, k times 4: peaked p), scale = kd^-0.5, element-wise bounds against
float64.  With A the companion of a quantity (the same sum over |terms|, proj_attn_ref.attn_fwd / attn_bwd):
* fp32 part, every route: 4 x d_q x A, d_q = the largest |float32 restatement - float64| / A over the cases, measured on the CPU
  (proj_attn_ref.attn_f32_distance; the factor 4 is for __expf and another summation order).  lse and delta are fp32 outputs of
  fp32 sums on every route: that is their whole bound, plus one fp32 rounding of the result.  The backward reads the forward output
  and lse the test passes in (the float64 forward rounded to bf16 / fp32), the reference reads the same numbers: the rounding of
  the stored `out` that delta sees is in the reference, not in the bound.
* stores: out, dq, dk, dv are rounded once to the storage type: half a bf16 ulp of the result (fp32: 2^-24 relative).
* MFMA operands: the forward rounds e = exp(s - max) to bf16 for O = P V (the row sum uses the unrounded e), the backward rounds
  dS (dQ, dK) and P (dV).  One rounding of x costs up to half_ulp_bf16(x), between 2^-9 |x| and 2^-8 |x|, so the term is
  sum_j half_ulp_bf16(x_ij) |y_j| (the companions `out_rnd`, `dqkv_rnd`), NOT a flat 2^-9 A: with p peaked the exact statement of
  the kernel already leaves 2^-9 A (tests/test_proj_attn_ref_host.py shows it).
* MFMA `out` is also held to the kernel's own statement out_pr = sum_j bf16(e_ij) v_j / sum_j e_ij within the fp32 part, the store
  and the roundings that an error of 4 d_e on e can flip (those within that distance of a bf16 rounding boundary: one bf16 ulp of e
  each).  This bound is below a quarter of the old tests' 2e-2 max|ref| on every element of every case (host test)."""
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32, Y3DError

import proj_attn_ref as R

DEV = "cuda"
G = 3  # guard rows


def out_slot(rows, width, sw, off, tdt):
    """(buffer, (rows, width) view at column `off` of rows of pitch `sw`), sentinel everywhere, G guard rows before and after"""
    buf = R.sentinel((rows + 2 * G) * sw, tdt, DEV)
    return buf, buf.view(rows + 2 * G, sw)[G:G + rows, off:off + width]


def flat_slot(n):
    buf = R.sentinel(n + 2 * 64, torch.float32, DEV)
    return buf, buf[64:64 + n]


def check_slot(buf, view, what):
    assert not bool(R.untouched(view).any()), f"{what}: {int(R.untouched(view).sum())} elements were never written"
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    if view.dim() == 1:
        o = view.storage_offset()
        mask[o:o + view.numel()] = False
    else:
        sw = view.stride(0)
        r0, c0 = divmod(view.storage_offset(), sw)
        mask.view(-1, sw)[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    assert bool(R.untouched(buf)[mask].all()), f"{what}: a store left the output slice"


def in_rows(x, sw, off, tdt, shift=0):
    """device copy of the host (rows, width) tensor as columns [off, off + width) of a buffer of pitch sw holding other values;
    `shift` moves the whole buffer by that many elements off its allocation"""
    rows, width = x.shape
    flat = (torch.randn(rows * sw + 64) * 3).to(tdt)
    v = flat[shift:shift + rows * sw].view(rows, sw)
    v[:, off:off + width] = x.to(tdt)
    return flat.to(DEV)[shift:shift + rows * sw].view(rows, sw)[:, off:off + width]


def layout(route, lay, W, O):
    """-> dict name -> (pixel stride, column offset) for qkv, out, dout, extra, dqkv, and the element shift of the qkv buffer"""
    if lay == "dense":
        d = {"qkv": (W, 0), "out": (O, 0), "dout": (O, 0), "extra": (O, 0), "dqkv": (W, 0)}
        return d, (2 if route == "fallback" else 0)
    d = {"qkv": (W + (10 if route == "fallback" else 8), 8), "out": (O + 8, 8), "dout": (O + 16, 8), "extra": (O + 3, 1), "dqkv": (W + 24, 8)}
    return d, 0


def takes_mfma(dt, tile, strides, ptrs, ptr_qkv):
    """the route test of y3d_attn_fwd (strides qsw, osw; addresses out) / y3d_attn_bwd (+ dsw, gsw; dout, dqkv)"""
    return dt == BF16 and bool(tile) and all(s % 4 == 0 for s in strides) and ptr_qkv % 16 == 0 and all(p % 8 == 0 for p in ptrs)


def run_attn(route, lay, a, B, N, nh, kd, hd, scale, out_in, lse_in, extras):
    """forward, then one backward per entry of `extras` (None or the dv_extra tensor) from `out_in` / `lse_in`; -> out, lse and a
    list of (dqkv, delta), all float64 on the host"""
    L, st = y3d.lib(), ops.stream()
    dt = F32 if route == "f32" else BF16
    tdt = R.TDT[dt]
    W, O = nh * (2 * kd + hd), nh * hd
    lo, shift = layout(route, lay, W, O)
    rows = B * N
    old = L.get_tile_kernels()
    L.set_tile_kernels(0 if route == "valu" else 1)
    try:
        tile = L.get_tile_kernels()
        qkv = in_rows(a["qkv"].reshape(rows, W), *lo["qkv"], tdt, shift)
        obuf, out = out_slot(rows, O, *lo["out"], tdt)
        lbuf, lse = flat_slot(B * nh * N)
        assert takes_mfma(dt, tile, (qkv.stride(0), out.stride(0)), (out.data_ptr(),), qkv.data_ptr()) == (route == "mfma")
        L.attn_fwd(dt, qkv.data_ptr(), qkv.stride(0), out.data_ptr(), out.stride(0), lse.data_ptr(), B, N, nh, kd, hd, scale, st)
        torch.cuda.synchronize()
        check_slot(obuf, out, f"attn_fwd out {route} {lay}")
        check_slot(lbuf, lse, f"attn_fwd lse {route} {lay}")
        oin = in_rows(out_in.reshape(rows, O), *lo["out"], tdt)
        dout = in_rows(a["dout"].reshape(rows, O), *lo["dout"], tdt)
        lin = lse_in.float().to(DEV).contiguous()
        back = []
        for ex in extras:
            exd = in_rows(ex.reshape(rows, O), *lo["extra"], tdt) if ex is not None else None
            gbuf, g = out_slot(rows, W, *lo["dqkv"], tdt)
            dbuf, delta = flat_slot(B * nh * N)
            assert takes_mfma(dt, tile, (qkv.stride(0), oin.stride(0), dout.stride(0), g.stride(0)),
                              (oin.data_ptr(), dout.data_ptr(), g.data_ptr()), qkv.data_ptr()) == (route == "mfma")
            L.attn_bwd(dt, qkv.data_ptr(), qkv.stride(0), oin.data_ptr(), oin.stride(0), dout.data_ptr(), dout.stride(0),
                       exd.data_ptr() if ex is not None else None, exd.stride(0) if ex is not None else 0, lin.data_ptr(), delta.data_ptr(),
                       g.data_ptr(), g.stride(0), B, N, nh, kd, hd, scale, st)
            torch.cuda.synchronize()
            check_slot(gbuf, g, f"attn_bwd dqkv {route} {lay}")
            check_slot(dbuf, delta, f"attn_bwd delta {route} {lay}")
            back.append((g.double().cpu().reshape(B, N, W), delta.double().cpu().reshape(B, nh, N)))
    finally:
        L.set_tile_kernels(old)
    return out.double().cpu().reshape(B, N, O), lse.double().cpu().reshape(B, nh, N), back


def assert_exact(got, want, what):
    """bit equality of the stored numbers up to the sign of zero: the widening to float64 is one to one, a NaN equals nothing"""
    ne = ~(got == want)
    if bool(ne.any()):
        i = tuple(ne.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ; first at {i}: got {float(got[i])!r}, expected {float(want[i])!r}")


def _ax_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.AX_CASES, ids=_ax_id)
def test_attention_exact(case):
    route, kd, hd, B, N, nh, lay = case
    a = R.attn_exact(B, N, nh, kd, hd, True)
    out, lse, back = run_attn(route, lay, a, B, N, nh, kd, hd, 1.0, a["out"], a["lse"], [None, a["dv_extra"]])
    assert_exact(out, a["out"], f"out {case}")
    assert_exact(lse, a["lse"], f"lse {case}")
    g0 = a["dqkv"].clone()
    R.blocks(g0, nh, kd, hd)["dv"].sub_(R.heads(a["dv_extra"], nh, hd))  # without dv_extra
    for (g, delta), want, tag in zip(back, (g0, a["dqkv"]), ("no dv_extra", "dv_extra")):
        assert_exact(delta, a["delta"], f"delta {case} {tag}")
        got, ref = R.blocks(g, nh, kd, hd), R.blocks(want, nh, kd, hd)
        for q in ("dq", "dk", "dv"):
            assert_exact(got[q].contiguous(), ref[q].contiguous(), f"{q} {case} {tag}")
        assert float(got["dq"].abs().max()) == 0 and float(got["dk"].abs().max()) == 0


def _check(what, got, ref, tol):
    err = (got - ref).abs()
    bad = ~(err <= tol)
    print(f"{what}: largest error / bound {float((err / tol).max()):.3f}")
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: got {float(got[i])!r} "
                             f"expected {float(ref[i])!r} bound {float(tol[i]):.3g}")


AR_RUNS = [(route, c, "strided" if (i + r) % 2 == 0 else "dense") for r, route in enumerate(R.AX_ROUTES) for i, c in enumerate(R.AR_CASES)]


@pytest.mark.gpu
@pytest.mark.parametrize("run", AR_RUNS, ids=lambda r: f"{r[0]}-{_ax_id(r[1])}-{r[2]}")
def test_attention_against_float64(run):
    route, case, lay = run
    kd, hd, kind, N = case
    a = R.attn_real(case)
    d = R.attn_f32_distance()
    out, lse, back = run_attn(route, lay, a, 1, N, R.AR_NH, kd, hd, a["scale"], a["out_in"], a["lse_in"], [a["dv_extra"]])
    g, delta = back[0]
    got = {"out": out, "lse": lse, "delta": delta, **R.blocks(g, R.AR_NH, kd, hd)}
    kind_of = "mfma" if route == "mfma" else ("f32" if route == "f32" else "valu")
    for q in R.QUANT:
        _check(f"{q} {route} {case}", got[q], a["ref"][q], R.attn_bound(kind_of, q, a["ref"][q], a["comp"][q], a["crnd"][q], d))
    if route == "mfma":
        pr, tol = R.attn_bound_mfma_out(case)
        _check(f"out against the kernel's own statement {case}", out, pr, tol)


@pytest.mark.gpu
def test_attention_rejections_leave_outputs_untouched():
    """a bad dtype and unsupported head dims are refused on the host: an error comes back and nothing is launched"""
    L, st = y3d.lib(), ops.stream()
    B, N, nh = 1, 16, 1
    for dt, kd, hd in ((2, 32, 64), (-1, 36, 72), (BF16, 32, 72), (BF16, 36, 64), (F32, 16, 32), (BF16, 64, 128), (F32, 0, 0)):
        W, O = nh * (2 * max(kd, 36) + max(hd, 72)), nh * max(hd, 72)
        qkv = torch.zeros(B * N, W, dtype=torch.float32, device=DEV)
        obuf, out = out_slot(B * N, O, O, 0, torch.float32)
        lbuf, lse = flat_slot(B * nh * N)
        gbuf, g = out_slot(B * N, W, W, 0, torch.float32)
        dbuf, delta = flat_slot(B * nh * N)
        with pytest.raises(Y3DError):
            L.attn_fwd(dt, qkv.data_ptr(), W, out.data_ptr(), O, lse.data_ptr(), B, N, nh, kd, hd, 1.0, st)
        with pytest.raises(Y3DError):
            L.attn_bwd(dt, qkv.data_ptr(), W, qkv.data_ptr(), O, qkv.data_ptr(), O, None, 0, qkv.data_ptr(), delta.data_ptr(), g.data_ptr(), W,
                       B, N, nh, kd, hd, 1.0, st)
        torch.cuda.synchronize()
        for buf in (obuf, lbuf, gbuf, dbuf):
            assert bool(R.untouched(buf).all()), f"dtype {dt} kd {kd} hd {hd}: a rejected call wrote to its outputs"
