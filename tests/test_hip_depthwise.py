"""The depth-wise family (csrc/dwconv.hip) against fp64 torch: forward (+ BatchNorm partial sums), the eval form with the folded
BatchNorm + SiLU (+ residual, res_mode 0 / 1 / 2), the data gradient and the weight gradient (slabs + reduce, accumulate 0 / 1).

* operands: x, dy in {0, +-1} and integer weights in [-127, 127]: every fp32 accumulation is exact, so the forward and data
  gradient must equal the exact result rounded ONCE to the storage type (bf16: sums above 256 do round), the BatchNorm partials
  and the weight gradient must equal the exact sums;
* the BatchNorm partials are fp32 sums over a block's pixels (a chain of ceil(px_per_block / PT) per thread, then PT rows):
  exact while a block's sums stay below 2^24, within (ceil(px_per_block / PT) + PT) * 2^-24 of the sum of |terms| beyond;
* the eval form is z = act(rnd(acc) * scale + shift (+ res, mode 2)) (+ res, mode 1), held to the eval-epilogue bound of
  test_hip_eval_epilogues.py.  Half of the channels get a shift that cancels rnd(acc) * scale at one pixel, so the bound sees
  whether the epilogue starts from the rounded depth-wise result;
* geometries: 3x3 s1 / s2 on even and odd maps, 7x7 (C2fCIB), 5x5 (the runtime-tap K = 0 kernels), partial and several 64-channel
  slabs, B = 32 at 80x80 (M > 131 072: the forward's 2 048-block and the weight gradient's 1 024-block caps lengthen the blocks),
  a channel slice of a wider input (xsw > C), bf16 and fp32."""
import pytest
import torch
import torch.nn.functional as F

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32

from test_hip_eval_epilogues import bound

DEV = "cuda"

# (dtype, B, C, H, W, k, stride, xslice): xslice = extra channels of the input buffer the conv reads a slice of
CASES = [
    (BF16, 2, 64, 20, 20, 3, 1, 0),
    (BF16, 3, 80, 21, 21, 3, 1, 0),
    (BF16, 2, 320, 40, 40, 3, 2, 0),      # SCDown: stride-2 depth-wise on an even map
    (BF16, 2, 128, 41, 41, 3, 2, 16),     # odd map 41 -> 21, channel-slice input
    (BF16, 3, 640, 20, 20, 7, 1, 0),      # C2fCIB large kernel
    (BF16, 2, 80, 20, 20, 7, 1, 32),
    (BF16, 2, 64, 13, 17, 5, 1, 0),       # K = 0 runtime-tap kernels
    (BF16, 2, 80, 15, 15, 5, 2, 0),
    (BF16, 32, 80, 80, 80, 3, 1, 0),      # M = 204 800 > 131 072 (the 2D head's cv3 depth-wise conv at 80x80, X width)
    (BF16, 32, 64, 80, 80, 3, 2, 0),      # SCDown's data gradient from 80x80: M = 204 800 input pixels
    (F32, 2, 64, 21, 21, 3, 1, 0),
    (F32, 2, 80, 41, 41, 3, 2, 8),
    (F32, 2, 128, 20, 20, 7, 1, 0),
    (F32, 2, 320, 13, 17, 5, 1, 0),
]
IDS = ["{}-B{}-C{}-{}x{}-k{}s{}-x{}".format("bf16" if c[0] == BF16 else "f32", *c[1:]) for c in CASES]


def test_case_list_reaches_every_instantiation():
    """CPU: the depth-wise kernels do not go through y3d_conv2d_route, so the list states its own coverage: the K = 3 / 7 / 0
    instantiations (dwconv.hip: DW_LAUNCH: 3x3 and 7x7 square filters are compiled in, any other runs the runtime-tap loops) in
    both dtypes, the stride-2 data-gradient branch on even and odd maps, M past both block caps, a channel slice, partial slabs"""
    kk = {(dt, k if k in (3, 7) else 0) for dt, B, C, H, W, k, s, xs in CASES}
    assert kk == {(dt, k) for dt in (BF16, F32) for k in (3, 7, 0)}, kk
    s2 = {H % 2 for dt, B, C, H, W, k, s, xs in CASES if k == 3 and s == 2}
    assert s2 == {0, 1}
    M = [B * ((H + 2 * (k // 2) - k) // s + 1) ** 2 for dt, B, C, H, W, k, s, xs in CASES if H == W]
    assert max(M) > 2048 * 64 and max(M) > 1024 * 128
    assert any(xs for *_, xs in CASES) and any(C % 64 for dt, B, C, *_ in CASES) and any(C > 256 for dt, B, C, *_ in CASES)


def _rnd(t, dt):
    return t.to(torch.bfloat16).double() if dt == BF16 else t.double()


def _operands(dt, B, C, H, W, k, s, xs, seed):
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (B, C, H, W), generator=gen).float()
    w = torch.randint(-127, 128, (C, 1, k, k), generator=gen).float()
    dy = torch.randint(-1, 2, (B, C, Ho, Wo), generator=gen).float() * (torch.rand(B, C, Ho, Wo, generator=gen) < 0.5)
    return x, w, dy, p, Ho, Wo, gen


def _nhwc(t, dt, extra=0):
    """device NHWC copy of an NCHW host tensor in the storage type, optionally as a channel slice of a wider buffer"""
    B, C, H, W = t.shape
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    buf = torch.full((B, H, W, C + extra), float("nan"), dtype=tdt, device=DEV)
    v = buf[..., extra // 2:extra // 2 + C]
    v.copy_(t.permute(0, 2, 3, 1).to(DEV))
    return v.permute(0, 3, 1, 2), buf


def _pixel_strides(v):
    return v.stride(0), v.stride(2), v.stride(3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dw_forward_partials_and_gradients_exact(case):
    dt, B, C, H, W, k, s, xs = case
    L, st = y3d.lib(), ops.stream()
    x, w, dy, p, Ho, Wo, gen = _operands(*case, seed=B * C + H + 10 * k + s)
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    xd, _ = _nhwc(x, dt, xs)
    wd = w.to(DEV).contiguous()
    wp = torch.empty(k * k * C, dtype=torch.float32, device=DEV)
    L.dw_pack_weight(wd.data_ptr(), wp.data_ptr(), C, k, k, st)
    # forward + BatchNorm partials
    M = B * Ho * Wo
    nblk = L.dw_blocks(M)
    part = torch.full((nblk, C, 2), float("nan"), dtype=torch.float32, device=DEV)
    ybuf = torch.full((B, Ho, Wo, C + 16), float("nan"), dtype=tdt, device=DEV)
    y = ybuf[..., 8:8 + C]
    L.dwconv2d_fwd(dt, xd.data_ptr(), *_pixel_strides(xd), B, H, W, C, wp.data_ptr(), y.data_ptr(), ybuf.stride(2), Ho, Wo, k, k, s, p,
                   part.data_ptr(), st)
    # data gradient (dx written into a channel slot too)
    dyd, _ = _nhwc(dy, dt)
    dxbuf = torch.full((B, H, W, C + 16), float("nan"), dtype=tdt, device=DEV)
    dx = dxbuf[..., 8:8 + C]
    L.dwconv2d_bwd_data(dt, dyd.data_ptr(), *_pixel_strides(dyd), B, Ho, Wo, C, wp.data_ptr(), dx.data_ptr(), dxbuf.stride(2), H, W, k, k, s, p, st)
    # weight gradient: slabs filled with NaN (every slot the reduce reads must be written), then accumulate onto a known gradient
    nb = L.dw_wgrad_blocks(M)
    slab = torch.full((nb * k * k * C,), float("nan"), dtype=torch.float32, device=DEV)
    dW = torch.full((C, 1, k, k), float("nan"), dtype=torch.float32, device=DEV)
    L.dwconv2d_bwd_weight(dt, xd.data_ptr(), *_pixel_strides(xd), B, H, W, C, dyd.data_ptr(), dyd.stride(3), Ho, Wo, k, k, s, p,
                          slab.data_ptr(), dW.data_ptr(), 0, st)
    dW0 = dW.clone()
    base = torch.randint(-1000, 1000, (C, 1, k, k), generator=gen).float().to(DEV)
    dWa = base.clone()
    slab.fill_(float("nan"))
    L.dwconv2d_bwd_weight(dt, xd.data_ptr(), *_pixel_strides(xd), B, H, W, C, dyd.data_ptr(), dyd.stride(3), Ho, Wo, k, k, s, p,
                          slab.data_ptr(), dWa.data_ptr(), 1, st)
    torch.cuda.synchronize()

    xg, wg, dyg = x.double(), w.double(), dy.double()
    acc = F.conv2d(xg, wg, stride=s, padding=p, groups=C)
    y_ref = _rnd(acc.float(), dt)
    yk = y.permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(yk, y_ref), f"forward: {int((yk != y_ref).sum())} of {yk.numel()} outputs differ"
    assert bool(ybuf[..., :8].isnan().all()) and bool(ybuf[..., 8 + C:].isnan().all()), "forward store left the output slot"
    part_ref = torch.stack((y_ref.sum((0, 2, 3)), (y_ref ** 2).sum((0, 2, 3))), 1)
    pk = part.double().sum(0).cpu()
    PT = 256 // (64 // (8 if dt == BF16 else 4))
    chain = -(-(-(-M // nblk)) // PT) + PT
    part_tol = chain * 2.0 ** -24 * torch.stack((y_ref.abs().sum((0, 2, 3)), (y_ref ** 2).sum((0, 2, 3))), 1)
    assert bool(((pk - part_ref).abs() <= part_tol).all()), f"BatchNorm partial sums differ: {float((pk - part_ref).abs().max())}"
    if float((y_ref ** 2).sum((0, 2, 3)).max()) < 2 ** 24:
        assert torch.equal(pk, part_ref), "BatchNorm partial sums differ (all partial sums below 2^24: exact)"
    dx_ref = _rnd(torch.nn.grad.conv2d_input(x.shape, wg, dyg, stride=s, padding=p, groups=C).float(), dt)
    dxk = dx.permute(0, 3, 1, 2).double().cpu()
    assert torch.equal(dxk, dx_ref), f"data gradient: {int((dxk != dx_ref).sum())} of {dxk.numel()} differ"
    assert bool(dxbuf[..., :8].isnan().all()) and bool(dxbuf[..., 8 + C:].isnan().all()), "data-gradient store left the slot"
    dW_ref = torch.nn.grad.conv2d_weight(xg, w.shape, dyg, stride=s, padding=p, groups=C)
    assert float(dW_ref.abs().max()) < 2 ** 24
    assert torch.equal(dW0.double().cpu(), dW_ref), "weight gradient differs"
    assert torch.equal(dWa.double().cpu(), dW_ref + base.double().cpu()), "weight gradient (accumulate = 1) differs"


@pytest.mark.gpu
@pytest.mark.parametrize("res_mode", [0, 1, 2])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("case", [c for c in CASES if c[6] == 1 or c[2] <= 128], ids=lambda c: IDS[CASES.index(c)])
def test_dw_eval_affine_against_fp64(case, act, res_mode):
    dt, B, C, H, W, k, s, xs = case
    L, st = y3d.lib(), ops.stream()
    x, w, dy, p, Ho, Wo, gen = _operands(*case, seed=7 * C + H + k + 3 * res_mode + act)
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    xd, _ = _nhwc(x, dt, xs)
    wd = w.to(DEV).contiguous()
    wp = torch.empty(k * k * C, dtype=torch.float32, device=DEV)
    L.dw_pack_weight(wd.data_ptr(), wp.data_ptr(), C, k, k, st)
    acc = F.conv2d(x.double(), w.double(), stride=s, padding=p, groups=C)
    a = _rnd(acc.float(), dt)  # the depth-wise result as the pre-BatchNorm tensor would store it
    scale = (0.05 + 1.95 * torch.rand(C, generator=gen)).float()
    shift = torch.randn(C, generator=gen).float()
    # odd channels: cancel a * scale at one pixel whose exact sum is not a bf16 value (where there is one)
    flat = a.permute(1, 0, 2, 3).reshape(C, -1)
    exact = acc.permute(1, 0, 2, 3).reshape(C, -1)
    for c in range(1, C, 2):
        cand = (exact[c] != flat[c]).nonzero()
        j = int(cand[0]) if len(cand) else int(flat[c].abs().argmax())
        shift[c] = float(-(flat[c, j] * scale[c].double()))
    r = torch.randint(-4, 5, (B, C, Ho, Wo), generator=gen).float() / 4
    rd, _ = _nhwc(r, dt, 16)
    zbuf = torch.full((B, Ho, Wo, C + 16), float("nan"), dtype=tdt, device=DEV)
    z = zbuf[..., 8:8 + C]
    sd, hd = scale.to(DEV), shift.to(DEV)
    L.dwconv2d_fwd_affine(dt, xd.data_ptr(), *_pixel_strides(xd), B, H, W, C, wp.data_ptr(), sd.data_ptr(), hd.data_ptr(), act, res_mode,
                          rd.data_ptr() if res_mode else None, rd.stride(3) if res_mode else 0, z.data_ptr(), zbuf.stride(2), Ho, Wo, k, k, s, p, st)
    torch.cuda.synchronize()
    assert bool(zbuf[..., :8].isnan().all()) and bool(zbuf[..., 8 + C:].isnan().all()), "eval store left the output slot"
    sc, sh = scale.double().view(1, C, 1, 1), shift.double().view(1, C, 1, 1)
    rr = r.double() if res_mode else torch.zeros_like(a)
    u = a * sc + sh + (rr if res_mode == 2 else 0)
    t = u * torch.sigmoid(u) if act else u
    ref = t + (rr if res_mode == 1 else 0)
    zk = z.permute(0, 3, 1, 2).double().cpu()
    err = (zk - ref).abs()
    tol = bound(dt, ref, t, rr, u, a * sc, (sh.abs() + (rr.abs() if res_mode == 2 else 0)).expand_as(u))
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{case} act={act} res_mode={res_mode}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: "
                             f"z={float(zk[i])!r} ref={float(ref[i])!r} acc={float(acc[i])} tol={float(tol[i]):.3g}")
