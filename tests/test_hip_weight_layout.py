"""The weight-layout kernels: the multi-tensor pack (csrc/conv_gemm.hip: mt_pack_w_kernel, layouts 0 / 1 / 2), the depth-wise
filters' place in the forward pack registry (ops._PackRegistry), and the split-K weight-gradient folds (wgrad_reduce_kernel,
dw_wgrad_reduce_kernel).

* packs: ONE multi-tensor call over a table of weights (forward, data-gradient and depth-wise layouts mixed) against the
  single-tensor entry points, bit for bit, bf16 and fp32, with the destinations pre-filled with NaN so that an unwritten
  padding element shows.  The table has Cg_pad > Cg, grouped weights, a 1x1, a tensor of 5.4 chunks, and is run with the
  registry's 16384-element chunks and with 256-element chunks (rows longer than a chunk: most chunks then own no row);
* registry: a depth-wise Conv's packed filter follows the fused optimizer (WEIGHT_EPOCH) and an in-place torch write, and the
  backward of a step reads the buffer its forward read;
* folds, exact: integer slabs (|v| <= 8, at most 256 splits: every partial sum is far below 2^24, so any order is exact)
  against the float64 sum;
* folds, order: random slabs against the fp32 host emulation of the documented order (wgrad_fold_ref.py), one case per
  kernel variant (16 / 8 split lanes: the flat mapping; 2 / 1: the row-owning one; and the depth-wise fold), bit for bit."""
import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import modules as M, ops
from yolov10_3d_amd._lib import BF16, F32

import wgrad_fold_ref as R

DEV = "cuda"

# (Cout, Cg, k, G): Cg input channels per group
PACK_TABLE = [(16, 8, 3, 1), (24, 40, 3, 1), (32, 16, 1, 1), (64, 8, 3, 2), (32, 3, 3, 1), (16, 12, 3, 1), (136, 72, 3, 1)]
DW_TABLE = [(40, 3), (72, 7)]  # (C, k)


def test_fold_reference_is_exact_on_integers():
    """CPU: the emulation itself - on integer slabs its fp32 sums equal the float64 sums, for every lane count"""
    rng = np.random.default_rng(0)
    for nsplit in (1, 3, 8, 33, 64, 256):
        slab = rng.integers(-8, 9, size=(nsplit, 4, 9, 8)).astype(np.float32)
        want = slab.astype(np.float64).sum(0).transpose(0, 2, 1)
        assert np.array_equal(R.wgrad_fold(slab, 8).astype(np.float64), want)
        assert np.array_equal(R.dw_fold(slab.reshape(nsplit, 9, 32)).astype(np.float64), slab.astype(np.float64).sum(0).reshape(9, 32).T)
    big = 136 * 9 * 72  # the table's large tensor: several of the registry's chunks, and no whole number of them
    assert (136, 72, 3, 1) in PACK_TABLE and big > 5 * ops._PackRegistry.CHUNK and big % ops._PackRegistry.CHUNK
    assert [R.split_lanes(n, s) for n, s in ((65536, 64), (65537, 64), (1048576, 32), (1048577, 32), (100, 8), (100, 7))] == [16, 8, 8, 2, 2, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [16384, 256])
@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "f32"])
def test_mt_pack_one_call_matches_single_tensor_entry_points(dt, chunk):
    L, st = y3d.lib(), ops.stream()
    tdt, ce = (torch.bfloat16, 8) if dt == BF16 else (torch.float32, 4)
    g = torch.Generator().manual_seed(5)
    ents, descs, ct, co = [], [], [], []

    def add(w, n, geo, mode, ref, dst_dtype):
        dst = torch.full((n,), float("nan"), dtype=dst_dtype, device=DEV)
        ents.append((w, ref, dst, mode))
        descs.extend([w.data_ptr(), dst.data_ptr(), *geo, mode])
        for j in range((n + chunk - 1) // chunk):
            ct.append(len(ents) - 1)
            co.append(j)

    for Cout, Cg, k, G in PACK_TABLE:
        taps = k * k
        w = torch.randn(Cout, Cg, k, k, generator=g).to(DEV)
        cgp = (Cg + ce - 1) // ce * ce
        n = Cout * taps * cgp
        ref = torch.empty(n, dtype=tdt, device=DEV)
        L.pack_weight_fwd(dt, w.data_ptr(), ref.data_ptr(), Cout, Cg, cgp, k, k, st)
        add(w, n, (Cout, Cg, cgp, taps, taps * cgp), 0, ref, tdt)
        cn = Cout // G
        kpad = L.conv_kpad(dt, taps * cn)
        n = G * Cg * kpad
        ref = torch.empty(n, dtype=tdt, device=DEV)
        L.pack_weight_dgrad(dt, w.data_ptr(), ref.data_ptr(), Cout, Cg, G, k, k, st)
        add(w, n, (G, cn, Cg, taps, kpad), 1, ref, tdt)
    for C, k in DW_TABLE:
        taps = k * k
        w = torch.randn(C, 1, k, k, generator=g).to(DEV)
        ref = torch.empty(taps * C, dtype=torch.float32, device=DEV)
        L.dw_pack_weight(w.data_ptr(), ref.data_ptr(), C, k, k, st)
        add(w, taps * C, (1, C, 1, taps, taps * C), 2, ref, torch.float32)
    t_desc = torch.tensor(descs, dtype=torch.int64, device=DEV)
    t_ct = torch.tensor(ct, dtype=torch.int32, device=DEV)
    t_co = torch.tensor(co, dtype=torch.int32, device=DEV)
    L.mt_pack_weights(dt, t_desc.data_ptr(), t_ct.data_ptr(), t_co.data_ptr(), len(ct), chunk, st)
    torch.cuda.synchronize()
    for i, (w, ref, dst, mode) in enumerate(ents):
        bits = torch.int16 if dst.dtype == torch.bfloat16 else torch.int32
        assert not torch.isnan(dst.float()).any(), (i, mode, tuple(w.shape), "unwritten elements")
        assert torch.equal(dst.view(bits), ref.view(bits)), (i, mode, tuple(w.shape))


def _tap_major(w):
    C = w.shape[0]
    return w.detach().reshape(C, -1).t().contiguous().flatten()


@pytest.mark.gpu
def test_depthwise_filters_live_in_the_forward_pack_registry():
    from yolov10_3d_amd.optim import FusedSGD
    y3d.set_compute_dtype(torch.bfloat16)
    L = y3d.lib()
    torch.manual_seed(3)
    C, k = 40, 3
    m = M.Conv(C, C, k, g=C).to(DEV).train()
    opt = FusedSGD([{"params": list(m.parameters())}], lr=0.1, momentum=0.9, nesterov=True)
    x = torch.randn(2, C, 12, 12, device=DEV)
    calls = {"dw_pack_weight": [], "dwconv2d_fwd": [], "dwconv2d_bwd_data": [], "mt_pack_weights": []}
    saved = {name: getattr(L, name) for name in calls}

    def spy(name):
        def f(*a):
            calls[name].append(a)
            return saved[name](*a)
        return f

    def entry():
        w = m.conv.weight
        return ops.PACK_FWD.entries[(w.data_ptr(), (1, C, 1, k * k, k * k * C, BF16), 2)]

    def step():
        for v in calls.values():
            v.clear()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        fwd_buf = calls["dwconv2d_fwd"][-1][9]
        assert fwd_buf == entry()["dst"].data_ptr()
        packed = entry()["dst"].clone()  # (what the forward read)
        y.float().sum().backward()
        assert calls["dwconv2d_bwd_data"][-1][9] == fwd_buf, "the backward read another buffer than the forward"
        return packed

    for name in calls:
        setattr(L, name, spy(name))
    try:
        p0 = step()
        assert torch.equal(p0, _tap_major(m.conv.weight))
        assert len(calls["dw_pack_weight"]) == 1  # an unknown weight is packed on its own, once: the backward looked it up
        w_old = m.conv.weight.detach().clone()
        opt.step()  # writes the weights through raw pointers and moves WEIGHT_EPOCH
        p1 = step()
        assert not torch.equal(m.conv.weight.detach(), w_old)
        assert torch.equal(p1, _tap_major(m.conv.weight))
        assert len(calls["dw_pack_weight"]) == 0 and len(calls["mt_pack_weights"]) == 1  # refreshed by the multi-tensor launch
        with torch.no_grad():
            m.conv.weight.mul_(0.5)  # a torch-side write: only the tensor's version counter moves
        p2 = step()
        assert torch.equal(p2, _tap_major(m.conv.weight)) and not torch.equal(p2, p1)
        assert len(calls["dw_pack_weight"]) == 1 and len(calls["mt_pack_weights"]) == 0
        p3 = step()  # nothing changed: nothing is packed
        assert torch.equal(p3, p2) and not calls["dw_pack_weight"] and not calls["mt_pack_weights"]
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)


# (Ctot, Cg, Cg_real, taps); the last: rows of 27 floats (the padded stem), so the 16-byte stores start off a 16-byte boundary
FOLD_SHAPES = [(8, 8, 8, 9), (16, 16, 12, 9), (24, 8, 8, 1), (16, 8, 3, 9)]
FOLD_CASES = [(ns, *s, acc) for s in FOLD_SHAPES for ns in (1, 3, 8, 33, 64, 256) for acc in (0, 1)]
# the few-slabs branch at 2048 rows; a row longer than the fold's LDS image (9216 floats: split into channel runs); 100 taps x 64
# channels (no split fits the image: the flat mapping)
FOLD_CASES += [(ns, *s, acc) for s in [(2048, 8, 8, 9)] for ns in (3,) for acc in (0, 1)]
FOLD_CASES += [(ns, *s, acc) for s in [(2, 1024, 1024, 9), (4, 64, 64, 100)] for ns in (3, 9) for acc in (0, 1)]


def _int_tensor(gen, *shape):
    return torch.randint(-8, 9, shape, generator=gen).float()


@pytest.mark.gpu
@pytest.mark.parametrize("nsplit,Ctot,Cg,Cg_real,taps,acc", FOLD_CASES, ids=["ns{}-{}x{}({})x{}-acc{}".format(*c) for c in FOLD_CASES])
def test_wgrad_fold_exact(nsplit, Ctot, Cg, Cg_real, taps, acc):
    L, st = y3d.lib(), ops.stream()
    gen = torch.Generator().manual_seed(nsplit * 131 + Ctot)
    slab = _int_tensor(gen, nsplit, Ctot, taps, Cg)
    grad0 = _int_tensor(gen, Ctot, Cg_real, taps)
    want = slab.double().sum(0)[:, :, :Cg_real].permute(0, 2, 1) + (grad0.double() if acc else 0)
    sd = slab.to(DEV)
    # (the gradient sits between two guard rows: a fold that writes the channel padding, or past its rows, shows)
    buf = torch.full((Ctot + 2, Cg_real, taps), 777.0, device=DEV)
    buf[1:-1] = grad0.to(DEV) if acc else float("nan")
    L.wgrad_fold(sd.data_ptr(), nsplit, Ctot, taps, Cg, Cg_real, buf[1].data_ptr(), acc, st)
    torch.cuda.synchronize()
    assert torch.equal(buf[1:-1].cpu().double(), want)
    assert bool((buf[0] == 777.0).all()) and bool((buf[-1] == 777.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("nsplit", [70, 37, 11, 5], ids=["SL16", "SL8", "SL2", "SL1"])
def test_wgrad_fold_keeps_the_documented_order(nsplit):
    L, st = y3d.lib(), ops.stream()
    Ctot, Cg, Cg_real, taps = 16, 16, 12, 9
    assert R.split_lanes(Ctot * taps * Cg, nsplit) == {70: 16, 37: 8, 11: 2, 5: 1}[nsplit]
    gen = torch.Generator().manual_seed(nsplit)
    slab = torch.randn(nsplit, Ctot, taps, Cg, generator=gen)
    grad0 = torch.randn(Ctot, Cg_real, taps, generator=gen)
    for acc in (0, 1):
        want = R.wgrad_fold(slab.numpy(), Cg_real, grad0.numpy() if acc else None)
        sd, out = slab.to(DEV), grad0.to(DEV).clone()
        L.wgrad_fold(sd.data_ptr(), nsplit, Ctot, taps, Cg, Cg_real, out.data_ptr(), acc, st)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), acc


@pytest.mark.gpu
@pytest.mark.parametrize("C,taps,nblk", [(40, 9, 5), (72, 49, 17), (40, 9, 70)])
def test_dw_wgrad_fold_exact_and_in_order(C, taps, nblk):
    L, st = y3d.lib(), ops.stream()
    gen = torch.Generator().manual_seed(C + nblk)
    for acc in (0, 1):
        slab = _int_tensor(gen, nblk, taps, C)
        grad0 = _int_tensor(gen, C, taps)
        want = slab.double().sum(0).t() + (grad0.double() if acc else 0)
        buf = torch.full((C + 2, taps), 777.0, device=DEV)
        buf[1:-1] = grad0.to(DEV) if acc else float("nan")
        sd = slab.to(DEV)
        L.dw_wgrad_fold(sd.data_ptr(), nblk, C, taps, buf[1].data_ptr(), acc, st)
        torch.cuda.synchronize()
        assert torch.equal(buf[1:-1].cpu().double(), want), acc
        assert bool((buf[0] == 777.0).all()) and bool((buf[-1] == 777.0).all())
        # random values: the documented order, bit for bit
        slab = torch.randn(nblk, taps, C, generator=gen)
        want = R.dw_fold(slab.numpy(), grad0.numpy() if acc else None)
        sd, out = slab.to(DEV), grad0.to(DEV).clone()
        L.dw_wgrad_fold(sd.data_ptr(), nblk, C, taps, out.data_ptr(), acc, st)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), acc
