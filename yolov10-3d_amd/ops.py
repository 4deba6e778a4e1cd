"""Autograd glue between torch tensors and the y3d C ABI (include/y3d.h).

PyTorch is plumbing here (device memory, streams, the autograd tape); every forward/backward body
below is a sequence of liby3d_hip.so launches on the current HIP stream.  Tensors keep the logical
NCHW shape of the reference's modules but live in NHWC ("channels last") memory in the compute
dtype (bf16 by default, fp32 for the parity mode).
"""
from __future__ import annotations

import ctypes
import os
from collections import namedtuple

import torch

from . import mt
from ._lib import BF16, F32, Y3DError, lib

_COMPUTE_DTYPE = torch.bfloat16


def set_compute_dtype(dt: torch.dtype):
    """torch.bfloat16 (performance mode) or torch.float32 (parity mode, exact-f32 MFMA)."""
    global _COMPUTE_DTYPE
    if dt not in (torch.bfloat16, torch.float32):
        raise ValueError("compute dtype must be torch.bfloat16 or torch.float32")
    _COMPUTE_DTYPE = dt


def compute_dtype() -> torch.dtype:
    return _COMPUTE_DTYPE


def code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float32:
        return F32
    raise Y3DError(f"unsupported tensor dtype {dt}")


def ce(dt: torch.dtype) -> int:
    return 8 if dt == torch.bfloat16 else 4


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_gpu(x: torch.Tensor):
    if not x.is_cuda:
        raise Y3DError("the y3d HIP path needs tensors on a HIP device (there is no CPU fallback)")


def nhwc_empty(B, C, H, W, dtype, device):
    """logical (B,C,H,W), memory (B,H,W,C)"""
    return torch.empty((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


# ---- output placement: a producer writes its result straight into a channel slice of its consumer's concat buffer ----------------
# (C2f / SPPF / Upsample -> Concat: the reference's torch.cat, block.py:236 / :176, conv.py:404, becomes a no-op instead of one copy per
# input; every kernel on this path takes a pixel stride, so a channel slice of a wider NHWC buffer is an ordinary operand.)
PLACEMENT = True  # tests flip it for A/B comparisons against copying
EVAL_LEVEL_STREAMS = True  # captured eval forward: one hipGraph branch per detection level (modules.v10Detect3d.inference_forward_feat)
_LEVEL_STREAMS: list = []


def level_streams(n: int):
    while len(_LEVEL_STREAMS) < n:
        _LEVEL_STREAMS.append(torch.cuda.Stream())
    return _LEVEL_STREAMS[:n]
_PLACE = None


class place:
    """`with place(buf, off): y = producer(x)` - the next output tensor of matching batch / spatial shape and dtype allocated by a
    kernel wrapper inside the block is `buf[:, off:off + C]` instead of a fresh tensor (consumed by the first match)."""

    def __init__(self, buf, off):
        self.t = (buf, off) if buf is not None else None

    def __enter__(self):
        global _PLACE
        self.prev, _PLACE = _PLACE, self.t

    def __exit__(self, *a):
        global _PLACE
        _PLACE = self.prev


# cross-layer placement (round 3): a Concat row of the yaml also takes the output of an EARLIER row (the backbone / neck skips: layers 4,
# 6, 10, 13 of the v10 tables).  tasks._predict_once opens `place_final(buf, off)` around that earlier row; the row's module hands the
# slot to its LAST kernel with `final_place()` (C2f / C2fCIB / PSA: the closing 1x1 conv), so the skip is written where the concat will
# read it - 13 -> 8 member copies per forward, 157 -> 33 MB.  A module that never calls final_place() leaves the slot unused (the concat
# copies that member as before).
_PLACE_FINAL = None


class place_final:
    def __init__(self, buf, off):
        self.t = (buf, off) if buf is not None else None

    def __enter__(self):
        global _PLACE_FINAL
        self.prev, _PLACE_FINAL = _PLACE_FINAL, self.t

    def __exit__(self, *a):
        global _PLACE_FINAL
        _PLACE_FINAL = self.prev


def final_place():
    """`with ops.final_place(): return last_op(...)` inside a module: the pending cross-layer slot (if any) becomes the placement of that op"""
    global _PLACE_FINAL
    t, _PLACE_FINAL = _PLACE_FINAL, None
    return place(*(t or (None, 0)))


def concat_buffer(x, C, H=None, W=None):
    """the buffer a group of producers will fill for a channel concat of C channels at x's batch / spatial size, or None"""
    dtype = _COMPUTE_DTYPE
    if not PLACEMENT or not x.is_cuda or C % ce(dtype) != 0:
        return None
    buf = nhwc_empty(x.shape[0], C, x.shape[2] if H is None else H, x.shape[3] if W is None else W, dtype, x.device)
    _CONCAT_BASE[buf.data_ptr()] = (C, buf)
    return buf


# addresses of the live concat buffers: ConcatFn only trusts "already in place" for slices of a buffer made by concat_buffer (a PSA
# block concatenates a slice of its cv1 output with a NEW tensor: that slice has the right strides too, and filling "its" buffer would
# overwrite the other half, which the backward still needs).  An entry dies with its ConcatFn; a model forward starts from none.
# The entry HOLDS its buffer: while an address is in the table the memory behind it cannot be freed and handed to another tensor, so
# "address + channel count match" cannot be a coincidence (a buffer nobody consumed lives until the next reset_placement).
_CONCAT_BASE = {}


# gradient placement (the mirror image of `place` for the backward pass): SplitChannelsFn hands channel slices of one map to several
# consumers; a consumer whose backward ends in a data-gradient kernel writes that gradient straight into ITS slice of one shared
# gradient buffer, and SplitChannelsFn.backward returns the buffer instead of concatenating the pieces (0.8 ms per step on the M head).
# key: (address, channels) of a slice as the consumer receives it -> (holder dict, channel offset)
_GRAD_SLOT = {}


def grad_slot(x):
    """the slice of the shared gradient buffer that belongs to input `x` of a consumer (a view made by SplitChannelsFn), or None"""
    ent = _GRAD_SLOT.get((x.data_ptr(), x.shape[1]))
    if ent is None:
        return None
    holder, off = ent
    if holder["shape"] != (x.shape[0], x.shape[2], x.shape[3]) or holder["dtype"] != x.dtype:
        return None
    return holder, off, x.shape[1]


def grad_slot_tensor(slot):
    """materialise (once) the shared buffer of a slot and return this consumer's slice of it"""
    holder, off, w = slot
    if holder["buf"] is None:
        B, H, W = holder["shape"]
        holder["buf"] = nhwc_empty(B, holder["C"], H, W, holder["dtype"], holder["device"])
    return holder["buf"][:, off:off + w]


def reset_placement():
    global _PLACE, _PLACE_FINAL
    _PLACE = None
    _PLACE_FINAL = None
    _CONCAT_BASE.clear()
    _GRAD_SLOT.clear()
    _FP8_ACT.clear()


def out_tensor(B, C, H, W, dtype, device):
    """nhwc_empty, or the placement slice if one is pending and fits"""
    global _PLACE
    if _PLACE is not None:
        buf, off = _PLACE
        if (buf.dtype == dtype and buf.shape[0] == B and buf.shape[2] == H and buf.shape[3] == W and off + C <= buf.shape[1]
                and off % ce(dtype) == 0 and C % ce(dtype) == 0 and buf.device == device):
            _PLACE = None
            return buf[:, off:off + C]
    return nhwc_empty(B, C, H, W, dtype, device)


def is_nhwc(x: torch.Tensor) -> bool:
    return x.dim() == 4 and (x.stride(1) == 1 or x.shape[1] == 1)


def px_dense(x: torch.Tensor) -> bool:
    """element (b,h,w,c) at ((b*H + h)*W + w) * stride(3) + c  (size-1 dims may carry arbitrary strides)"""
    B, C, H, W = x.shape
    sw = x.stride(3)
    return is_nhwc(x) and sw >= C and (H == 1 or x.stride(2) == W * sw) and (B == 1 or x.stride(0) == H * W * sw)


def to_nhwc(x: torch.Tensor, dtype=None, dense=False) -> torch.Tensor:
    """Return x as an NHWC tensor of the compute dtype, 16-byte aligned; copies only when needed."""
    dtype = dtype or _COMPUTE_DTYPE
    c = ce(dtype)
    ok = (x.dtype == dtype and is_nhwc(x) and x.data_ptr() % 16 == 0 and x.stride(0) % c == 0 and x.stride(2) % c == 0
          and x.stride(3) % c == 0 and (not dense or px_dense(x)))
    if ok:
        return x
    B, C, H, W = x.shape
    out = nhwc_empty(B, C, H, W, dtype, x.device)
    out.copy_(x)
    return out


def s3(x):
    return x.stride(0), x.stride(2), x.stride(3)


def _f32(n, device):
    return torch.empty(n, dtype=torch.float32, device=device)


class KernelTimer:
    """Live per-launch timing of selected kernels with HIP events on the launch stream (bench.py's roofline leg).
    `want(key)` decides which launches are bracketed; results: {key: [ms, ...]}."""

    def __init__(self, want):
        self.want = want
        self.pending = []

    def bracket(self, key, fn):
        if not self.want(key):
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.pending.append((key, a, b))
        return r

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for key, a, b in self.pending:
            out.setdefault(key, []).append(a.elapsed_time(b))
        return out


TIMER = None  # set by bench.py

# Parameters, BatchNorm running statistics and EMA weights are written by HIP kernels through raw pointers, which torch's tensor
# version counters do not see.  Every such writer bumps this epoch, and the eval-path cache of packed / folded weights keys on it.
PARAM_EPOCH = 0


def bump_param_epoch():
    global PARAM_EPOCH
    PARAM_EPOCH += 1


WEIGHT_EPOCH = 0  # bumped by the raw-pointer writers of PARAMETERS only (optimizer step): the packed training weights key on it


def bump_weight_epoch():
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1
    bump_param_epoch()


class _WeightRegistry:
    """what the registries of per-weight device copies below share: the hipGraph lifetime rules, and when an entry is refreshed or dropped
    (nobody looked it up for KEEP epochs: re-pointed / freed parameters)"""

    KEEP = 4

    def __init__(self):
        self.entries, self.epoch, self.tables = {}, None, None
        # A hipGraph capture (graph.GraphedTrainStep) bakes in the ADDRESSES of the descriptor tables and of the buffers it looked up:
        # both must outlive the graph.  Tables used while capturing are kept here for good (a later multi-tensor launch with more entries
        # - a second model in the process - builds new tables and would otherwise free the ones the graph's launch still reads: it then
        # follows whatever "pointers" the reused memory holds), entries looked up while capturing are never evicted.
        self.captured_tables = []

    def _hold_tables(self):
        """before a launch that reads self.tables"""
        if torch.cuda.is_current_stream_capturing() and not any(t is self.tables for t in self.captured_tables):
            self.captured_tables.append(self.tables)

    def _revisit(self, e, now, ver, refresh_all):
        """the bookkeeping of a lookup that found entry `e`.  `now`: the epoch its copy has to be of; `refresh_all()`: the registry's
        multi-tensor launch, returning the entries it covered.  -> True when `e` was changed through torch since its copy was made
        (load_state_dict, init, broadcast, torch.optim): the caller refreshes it on its own."""
        e["seen"] = WEIGHT_EPOCH
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            e["pinned"] = True
        if self.epoch != now:
            self.epoch = now
            # (not while a hipGraph is being captured: dropping entries changes the table key, and rebuilding the descriptor tables is a
            # host-to-device copy, which a capture does not allow - entries of a model that is gone wait for the next eager step)
            stale = [] if capturing else [k for k, v in self.entries.items() if WEIGHT_EPOCH - v["seen"] > self.KEEP and not v.get("pinned")]
            for k in stale:
                del self.entries[k]
            for v in refresh_all():
                v["ver"] = None  # refreshed from memory: whatever version the tensor has now is the copied one
        changed = e["ver"] is not None and e["ver"] != ver
        e["ver"] = ver
        return changed


class _PackRegistry(_WeightRegistry):
    """Packed compute-dtype copies of the conv weights for the training step, refreshed by ONE multi-tensor launch per step
    (`y3d_mt_pack_weights`) instead of one tiny launch per conv and direction (S-3D: 113 launches of ~5 us + their gaps).

    A weight is identified by (address, geometry, layout); its packed buffer is persistent.  The first lookup after the weights changed
    (WEIGHT_EPOCH moved: the fused optimizer wrote them) repacks every registered weight of that dtype from whatever its address holds
    now; a weight changed through torch (in-place op: its `_version` moved) is repacked on its own; an unknown weight is packed on its
    own and registered.

    `mode` is the layout of the registry's weights (0: forward, 1: data gradient).  The depth-wise filters (layout 2: tap-major fp32,
    what `y3d_dw_pack_weight` writes) are entries of the FORWARD registry with a layout of their own: they ride in its launch, and the
    backward of a step finds the buffer its forward used."""

    DW = 2

    CHUNK = mt.CHUNK

    def __init__(self, mode):
        super().__init__()
        self.mode = mode

    def _pack_one(self, e):
        L, st = lib(), stream()
        a, b, c, taps, kpad, dt = e["geo"]
        k = int(round(taps ** 0.5))
        if e["mode"] == self.DW:
            L.dw_pack_weight(e["src"], e["dst"].data_ptr(), b, k, k, st)
        elif e["mode"] == 0:
            L.pack_weight_fwd(dt, e["src"], e["dst"].data_ptr(), a, b, c, k, k, st)
        else:
            L.pack_weight_dgrad(dt, e["src"], e["dst"].data_ptr(), a * b, c, a, k, k, st)

    def _pack_all(self, dt):
        ents = [e for e in self.entries.values() if e["geo"][5] == dt]
        if not ents:
            return ents
        dev = ents[0]["dst"].device
        key = tuple(id(e) for e in ents)
        if self.tables is None or self.tables[0] != (key, dt):
            desc, sizes = [], []
            for e in ents:
                a, b, c, taps, kpad, _ = e["geo"]
                sizes.append(a * kpad if e["mode"] == 0 else a * c * kpad)
                desc += [e["src"], e["dst"].data_ptr(), a, b, c, taps, kpad, e["mode"]]
            ct, co = mt.chunk_map(sizes, self.CHUNK)
            self.tables = ((key, dt), torch.tensor(desc, dtype=torch.int64, device=dev), torch.tensor(ct, dtype=torch.int32, device=dev),
                           torch.tensor(co, dtype=torch.int32, device=dev), len(ct))
        _, desc, ct, co, n = self.tables
        self._hold_tables()
        lib().mt_pack_weights(dt, desc.data_ptr(), ct.data_ptr(), co.data_ptr(), n, self.CHUNK, stream())
        return ents

    def lookup(self, w32, src_ptr, geo, dtype, ver=None, mode=None):
        """geo = (a, b, c, taps, Kpad, dt) as y3d_mt_pack_weights; src_ptr: address of the (sub)tensor to pack -> packed tensor.
        `mode`: the layout when it is not the registry's own (DW: dtype is torch.float32, dt the compute dtype whose launch it joins).
        `ver`: the torch-side version token of the weights (default: w32's own counter).  A stacked weight passes the counters of
        its per-branch Parameters: they are re-pointed at slices of the flat tensor with `.data =`, which shares storage but NOT the
        version counter, so torch-side writers (torch.optim, load_state_dict, init, broadcast) move only the Parameters' counters."""
        mode = self.mode if mode is None else mode
        key = (src_ptr, geo, mode)
        ver = w32._version if ver is None else ver
        e = self.entries.get(key)
        if e is None:
            a, b, c, taps, kpad, dt = geo
            n = a * kpad if mode == 0 else a * c * kpad
            # "keep": the registry re-reads `src` at every epoch, so the storage behind it must outlive the entry
            e = {"src": src_ptr, "geo": geo, "mode": mode, "dst": torch.empty(n, dtype=dtype, device=w32.device), "ver": ver,
                 "seen": WEIGHT_EPOCH, "keep": w32}
            self.entries[key] = e
            self._pack_one(e)
        elif self._revisit(e, (WEIGHT_EPOCH, geo[5]), ver, lambda: self._pack_all(geo[5])):
            self._pack_one(e)
        return e["dst"]


class _QuantRegistry(_WeightRegistry):
    """fp8 (e4m3fn, per-output-channel power-of-two scale) shadows of the conv weights — the `fp8w` weight mode (csrc/fp8w.hip).

    For every registered fp32 master weight (identified by address + shape) it keeps `w_eff` (fp32, what the kernels pack and
    multiply: exactly representable in bf16), the 1-byte codes and the scales.  All shadows are refreshed by ONE multi-tensor
    launch the first time a weight is looked up after the fused optimizer moved the weight epoch; a weight changed through torch
    (its version token moved) is refreshed on its own.  `lookup` returns (w_eff, token): the token stands in for the master's
    version in the pack registries' and the eval caches' keys (the shadow's own counter never moves)."""

    def _run(self, ents):
        dev = ents[0]["weff"].device
        key = tuple(id(e) for e in ents)
        if self.tables is None or self.tables[0] != key:
            desc, rb, r = [], [], 0
            for e in ents:
                rows, K = e["shape"]
                desc += [e["src"], e["weff"].data_ptr(), e["codes"].data_ptr(), e["scale"].data_ptr(), rows, K]
                rb.append(r)
                r += rows
            self.tables = (key, torch.tensor(desc, dtype=torch.int64, device=dev), torch.tensor(rb, dtype=torch.int32, device=dev), len(ents), r)
        _, desc, rb, nt, nrows = self.tables
        self._hold_tables()
        lib().mt_fp8w_quantize(desc.data_ptr(), rb.data_ptr(), nt, nrows, stream())
        return ents

    def _run_one(self, e):
        tb, self.tables = self.tables, None  # a table of its own: the one over all entries stays for the next epoch
        self._run([e])
        self.tables = tb

    def lookup(self, w32, ver=None):
        ver = w32._version if ver is None else ver
        rows, K = w32.shape[0], w32[0].numel()
        key = (w32.data_ptr(), rows, K)
        e = self.entries.get(key)
        if e is None:
            dev = w32.device
            e = {"src": w32.data_ptr(), "shape": (rows, K), "keep": w32, "weff": torch.empty(w32.shape, dtype=torch.float32, device=dev),
                 "codes": torch.empty((rows, K), dtype=torch.uint8, device=dev), "scale": torch.empty(rows, dtype=torch.float32, device=dev),
                 "ver": ver, "count": 0, "seen": WEIGHT_EPOCH}
            self.entries[key] = e
            self._run_one(e)
        elif self._revisit(e, WEIGHT_EPOCH, ver, lambda: self._run(list(self.entries.values()))):
            e["count"] += 1  # the master was written through torch since the shadow was made
            self._run_one(e)
        self.last = e  # (the entry of the weight just looked up: the fp8 MFMA path packs its codes, fp8_weight)
        return e["weff"], (WEIGHT_EPOCH, e["count"])


PACK_FWD, PACK_DGRAD, QUANT = _PackRegistry(0), _PackRegistry(1), _QuantRegistry()


def _dw_packed(w32, C, k, dtype, ver):
    """the tap-major fp32 copy of a depth-wise filter for a training step: from the forward pack registry, or packed on the spot"""
    if PACK_CACHE:
        return PACK_FWD.lookup(w32, w32.data_ptr(), (1, C, 1, k * k, k * k * C, code(dtype)), torch.float32, ver, _PackRegistry.DW)
    wp = _f32(k * k * C, w32.device)
    lib().dw_pack_weight(w32.data_ptr(), wp.data_ptr(), C, k, k, stream())
    return wp


def _fwd_packed(w32, Cout, Cin_g, Cg_pad, k, dtype, ver=None, registry=False):
    """the K-contiguous compute-dtype rows of a dense / grouped conv weight (Cin_g channels per group, rows padded to Cg_pad): from the
    forward pack registry when the caller asks for it (`registry`: the weights of a training step), or packed on the spot"""
    dt = code(dtype)
    if registry and PACK_CACHE:
        return PACK_FWD.lookup(w32, w32.data_ptr(), (Cout, Cin_g, Cg_pad, k * k, k * k * Cg_pad, dt), dtype, ver)
    wp = torch.empty(Cout * k * k * Cg_pad, dtype=dtype, device=w32.device)
    lib().pack_weight_fwd(dt, w32.data_ptr(), wp.data_ptr(), Cout, Cin_g, Cg_pad, k, k, stream())
    return wp


def _dgrad_packed(w32, src, co, Cin_g, g, k, dtype, ver=None, registry=False):
    """the data-gradient layout of the `co` output channels of w32 that start at address `src`: from the data-gradient pack registry
    when the caller asks for it, or packed on the spot"""
    dt = code(dtype)
    kp = lib().conv_kpad(dt, k * k * (co // g))
    if registry and PACK_CACHE:
        return PACK_DGRAD.lookup(w32, src, (g, co // g, Cin_g, k * k, kp, dt), dtype, ver)
    wpd = torch.empty(Cin_g * g * kp, dtype=dtype, device=w32.device)
    lib().pack_weight_dgrad(dt, src, wpd.data_ptr(), co, Cin_g, g, k, k, stream())
    return wpd


WEIGHT_QUANT = None  # None | "fp8": conv (+BatchNorm) weights as e4m3fn codes with per-output-channel power-of-two scales


def set_weight_quant(mode):
    """None (default) or "fp8": BASELINE configs[4].  Applies to the weights of Conv modules (dense / grouped convs followed by
    BatchNorm: 99 % of the parameters); depth-wise filters and the heads' final 1x1 projections (with bias) stay in full precision."""
    global WEIGHT_QUANT
    if mode not in (None, "fp8"):
        raise ValueError("weight quantisation mode must be None or 'fp8'")
    WEIGHT_QUANT = mode
    if mode is None:
        set_fp8_dgrad(False)
    bump_param_epoch()


def weight_quant():
    return WEIGHT_QUANT


# ---- fp8 MFMA convolutions (csrc/conv3x3_fp8.hip; BASELINE configs[4]) ------------------------------------------------------------
# With `set_weight_quant("fp8")` AND `set_fp8_conv(True)` the forward of every bf16 3x3 stride-1 Conv whose geometry the kernel serves
# (y3d_conv3x3_fp8_ok: the head's two 3x3 layers at the S / B / L / X widths) runs on v_mfma_scale_f32_16x16x128_f8f6f4: e4m3 weight
# codes (the fp8w quantiser's) x e4m3 activations with one E8M0 scale per (pixel, 32 channels).  The activation's fp8 copy comes from its
# producer when that is a BatchNorm + SiLU pass told to write one (`want_fp8_copy`: y3d_bn_act_fwd_q), else from y3d_fp8_quantize_act.
# Weight gradients stay on the bf16 kernels (x and w_eff in bf16: straight-through); so do the data gradients unless `set_fp8_dgrad(True)`:
# then the data gradient of every layer whose forward took the fp8 kernel and whose swapped geometry it serves (y3d_conv3x3_fp8_dgrad_ok)
# runs on the same kernel - dy with the weight's power-of-two row scales folded in, MX-quantised, x the SAME e4m3 codes with the taps flipped.
FP8_CONV = False
FP8_DGRAD = False
_FP8_WANT = False
_FP8_ACT = {}  # address of a bf16 activation -> (q, s, shape, z): the fp8 copy its producer wrote; dropped at the next forward


def set_fp8_conv(on: bool):
    global FP8_CONV
    if on and WEIGHT_QUANT != "fp8":
        raise ValueError('set_fp8_conv(True) needs set_weight_quant("fp8"): the kernel multiplies the fp8w quantiser\'s codes')
    FP8_CONV = bool(on)
    if not on:
        set_fp8_dgrad(False)
    bump_param_epoch()


def fp8_conv():
    return FP8_CONV


def set_fp8_dgrad(on: bool):
    """opt-in: data gradients of the fp8 MFMA convolutions in fp8 (e4m3 / MX) as well.  Needs `set_fp8_conv(True)`; switching the fp8
    convolutions or the fp8 weights off switches it off too."""
    global FP8_DGRAD
    if on and not FP8_CONV:
        raise ValueError("set_fp8_dgrad(True) needs set_fp8_conv(True): the data gradient follows the layers whose forward runs in fp8")
    FP8_DGRAD = bool(on)


def fp8_dgrad():
    return FP8_DGRAD


class want_fp8_copy:
    """`with want_fp8_copy(): z = conv_bn_act(...)`: the BatchNorm + SiLU pass inside also writes the fp8 copy of z (when fp8 convolutions
    are on and the tensor qualifies); the next fp8 convolution that takes z as its input picks it up"""

    def __enter__(self):
        global _FP8_WANT
        self.prev, _FP8_WANT = _FP8_WANT, FP8_CONV
        return self

    def __exit__(self, *a):
        global _FP8_WANT
        _FP8_WANT = self.prev


def fp8_input(xin):
    """(q (B, H, W, C) e4m3 codes, s (B, H, W, C / 32) E8M0 bytes) of the bf16 NHWC activation `xin`: the producer's copy, or a quantising pass"""
    B, C, H, W = xin.shape
    ent = _FP8_ACT.pop(xin.data_ptr(), None)
    if ent is not None and ent[2] == (B, C, H, W):
        return ent[0], ent[1]
    if not px_dense(xin):
        xin = to_nhwc(xin, torch.bfloat16, dense=True).contiguous(memory_format=torch.channels_last)
    q = torch.empty(B, H, W, C, dtype=torch.uint8, device=xin.device)
    s = torch.empty(B, H, W, lib().fp8_scale_pitch(C), dtype=torch.uint8, device=xin.device)
    lib().fp8_quantize_act(xin.data_ptr(), xin.stride(3), B * H * W, C, q.data_ptr(), s.data_ptr(), stream())
    return q, s


def fp8_weight(ent, Cg):
    """(wq (rows, 9, Cg) bytes, ws (rows,) E8M0 bytes) of a quantised 3x3 weight (a _QuantRegistry entry), repacked when its codes changed"""
    tok = (WEIGHT_EPOCH, ent["count"])
    hit = ent.get("wq")
    if hit is None or hit[0] != tok:
        rows = ent["shape"][0]
        dev = ent["codes"].device
        wq = hit[1] if hit is not None else torch.empty(rows, 9, Cg, dtype=torch.uint8, device=dev)
        ws = hit[2] if hit is not None else torch.empty(rows, dtype=torch.uint8, device=dev)
        lib().fp8_pack_weight_fwd(ent["codes"].data_ptr(), ent["scale"].data_ptr(), rows, Cg, wq.data_ptr(), ws.data_ptr(), stream())
        hit = ent["wq"] = (tok, wq, ws)
    return hit[1], hit[2]


def fp8_weight_dgrad(ent, Cin, g, lo, hi):
    """(wq [g][Cin / g][9 flipped][(hi - lo) / g] bytes, ws (Cin,) unit E8M0 bytes) of a quantised 3x3 weight for its data gradient over the
    output channels [lo, hi); cached per window in the _QuantRegistry entry and repacked (into the same storage) when its codes changed"""
    tok = (WEIGHT_EPOCH, ent["count"])
    cache = ent.setdefault("wqd", {})
    hit = cache.get((g, lo, hi))
    if hit is None or hit[0] != tok:
        Cout = ent["shape"][0]
        dev = ent["codes"].device
        wq = hit[1] if hit is not None else torch.empty(g, Cin // g, 9, (hi - lo) // g, dtype=torch.uint8, device=dev)
        ws = hit[2] if hit is not None else torch.empty(Cin, dtype=torch.uint8, device=dev)
        lib().fp8_pack_weight_dgrad(ent["codes"].data_ptr(), Cout, Cin, g, lo, hi, wq.data_ptr(), ws.data_ptr(), stream())
        hit = cache[(g, lo, hi)] = (tok, wq, ws)
    return hit[1], hit[2]


PROJ_BN_MFMA = True  # BatchNorm backward of the second head layer recomputing dz on MFMA (tests flip it: materialised path)
STEM_FUSED = True  # the stem in one pass (tests flip it: im2col + dense conv)
PACK_CACHE = True  # weight packs through the registry (one multi-tensor launch per step)
DW_EVAL_FUSED = True  # eval depth-wise conv: folded BatchNorm + SiLU + residual in the conv's epilogue (tests flip it: conv + bn_act_fwd)


# ------------------------------------------------------------------------------------------------------
# Conv (dense / grouped / depth-wise) + BatchNorm + SiLU + residual
# ------------------------------------------------------------------------------------------------------
def conv_bn_act_eval(x, w, gamma, beta, rm, rv, k, s, p, g, act, eps, cache=None, ver=None):
    """eval-mode act(bn(conv(x))) on explicit (possibly stacked / sliced) tensors; no autograd.  `cache`: a dict owned by the
    caller that keeps the packed weights + folded BatchNorm scale/shift until a parameter changes; `ver`: version token of the
    tensors behind a stacked view (StackedConvs.ver)"""
    z, _, _ = _cba_forward(x, ConvCall(w32=w, g32=gamma, b32=beta, rm=rm, rv=rv, k=k, s=s, p=p, g=g, act=act, eps=eps, cache=cache, ver=ver))
    return z


_IDENT = {}  # (channels, device) -> (ones, zeros): gamma / running variance and beta / running mean of an identity BatchNorm


def _identity_bn(C, device):
    ident = _IDENT.get((C, device))
    if ident is None:
        ident = _IDENT[(C, device)] = (torch.ones(C, dtype=torch.float32, device=device), torch.zeros(C, dtype=torch.float32, device=device))
    return ident


def conv_bias_act_eval(x, w, bias, k, s, p, g, act, res, res_mode, cache):
    """act(conv(x) + bias) (+res): a Conv after the reference's BaseModel.fuse() (nn/tasks.py:187-192, conv.py:124-126), run as the eval
    sequence with an IDENTITY BatchNorm - gamma 1, running mean 0, running variance 1, eps 0: scale exactly 1, shift exactly the bias -
    so the folded model goes through the same kernels (affine conv epilogue, residual forms) as the unfolded eval path."""
    _require_gpu(x)
    ones, zeros = _identity_bn(w.shape[0], w.device)
    with torch.no_grad():
        z, _, _ = _cba_forward(x, ConvCall(w32=_w32(w), g32=ones, b32=bias.detach().float(), rm=zeros, rv=ones, k=k, s=s, p=p, g=g, act=act,
                                           res=res, res_mode=res_mode, cache=cache))
    return z


def _cache_put(cache, key, value):
    """insert into an eval cache (keys carry PARAM_EPOCH at [1]), dropping what older epochs left behind"""
    for old in [q for q in cache if q[1] != PARAM_EPOCH]:
        del cache[old]
    cache[key] = value


def _eval_consts(call, kind, dtype, Cin_g, Cg_pad, Cout):
    """eval-mode constants of one conv, cached in `call.cache` (a dict owned by the module / stack) until a parameter or buffer changes:
    the packed weights (kind "dense": K-contiguous compute-dtype rows; "dw": tap-major fp32 rows) and the folded BatchNorm
    (scale, shift) pair.  A steady-state eval forward launches neither packing nor bn_eval_scale kernels."""
    cache, w32, g32, b32, rm, rv, ver, k, g, eps = call.cache, call.w32, call.g32, call.b32, call.rm, call.rv, call.ver, call.k, call.g, call.eps
    L, st, dev = lib(), stream(), w32.device
    vkey = ver[1] if ver is not None else (w32._version, g32._version, b32._version, rm._version, rv._version)
    key = (kind, PARAM_EPOCH, w32.data_ptr(), g32.data_ptr(), rm.data_ptr(), vkey, dtype, k, g, Cg_pad, Cout, float(eps))
    hit = cache.get(key) if cache is not None else None
    if hit is None:
        if kind == "dw":
            wp = _f32(k * k * Cout, dev)
            L.dw_pack_weight(w32.data_ptr(), wp.data_ptr(), Cout, k, k, st)
        else:
            wp = _fwd_packed(w32, Cout, Cin_g, Cg_pad, k, dtype)
        ss = _f32(2 * Cout, dev).view(2, Cout)
        L.bn_eval_scale(Cout, g32.data_ptr(), b32.data_ptr(), rm.data_ptr(), rv.data_ptr(), eps, ss[0].data_ptr(), ss[1].data_ptr(), st)
        hit = (wp, ss, w32)  # w32 kept alive: its address is part of the key
        if cache is not None:  # owned by the module / stack, so it dies with the tensors it describes
            _cache_put(cache, key, hit)
    return hit[0], hit[1]


def _timed(key, launch):
    if TIMER is not None:
        TIMER.bracket(key, launch)
    else:
        launch()


# What the forward of one conv + BatchNorm + activation decided and its backward needs.  Cin_k: input channels as the kernels see them (Cin
# padded to whole 16-byte chunks); wver: version token of the weights as packed (stacked views / fp8 shadows carry their identity outside
# the tensor's own counter); fp8_entry: the quantiser entry whose codes the fp8 MFMA forward multiplied (None on every other path: the
# fp8 data gradient follows it); stem: the conv ran as a K = 32 GEMM over im2col rows of the image (dW is mapped back, no dx).
ConvPlan = namedtuple("ConvPlan", "B Cin Cin_k H W Cout Ho Wo k s p g dw res_mode training dtype act wver fp8_entry stem", defaults=(False,))


# What one conv + BatchNorm + activation forward is asked to do: fp32 weight and BatchNorm tensors, geometry, activation, residual
# (res_mode 1: act(bn(conv)) + res, 2: act(bn(conv) + res)) and BatchNorm mode.  cache: the dict of eval constants owned by the module /
# stack (None: nothing is kept); bn_apply False: the consumer applies BatchNorm + activation itself and gets the pre-BatchNorm tensor;
# ver = (weights token, all-tensors token) of a stacked view (StackedConvs) or an fp8 shadow, None for tensors with counters of their own.
ConvCall = namedtuple("ConvCall", "w32 g32 b32 rm rv k s p g act res res_mode training eps momentum cache bn_apply ver",
                      defaults=(None, 0, False, 0.0, 0.0, None, True, None))


def _module_call(m, **fields):
    """the ConvCall of Conv module `m` (kernel, stride, padding, activation, BatchNorm mode and constants); `fields`: the tensors, the
    groups and whatever else the caller sets"""
    return ConvCall(k=m.k, s=m.s, p=m.p, act=m.has_act, training=m.training, eps=m.eps, momentum=m.momentum, **fields)


def _wver(call):
    return call.ver[0] if call.ver is not None else None


def _cba_forward(x, call):
    """conv -> BN statistics -> BN apply + SiLU (+res).  Returns (z, plan, saved) with everything the backward needs."""
    _require_gpu(x)
    dtype = _COMPUTE_DTYPE
    B, Cin, H, W = x.shape
    w32, k, s, p, g = call.w32, call.k, call.s, call.p, call.g
    dw = g > 1 and g == Cin and g == w32.shape[0]
    qent = None
    if WEIGHT_QUANT and not dw:
        # fp8w mode: the kernels pack and multiply the fp8-valued shadow of the weight; the master keeps receiving the gradient
        w32, qtok = QUANT.lookup(w32, _wver(call))
        qent = QUANT.last
        rest = call.ver[1] if call.ver is not None else (call.g32._version, call.b32._version, call.rm._version, call.rv._version)
        call = call._replace(w32=w32, ver=((qtok,), (qtok,) + rest))
    Cout, Cg_w, kh, kw = w32.shape
    assert kh == k and kw == k and Cin // g == Cg_w, "Conv: weight shape does not match input"
    if Cin == 3 and k == 3 and s == 2 and p == 1 and g == 1 and not x.requires_grad:
        return _stem_forward(x, call)
    # ---- input: NHWC compute dtype; a channel count that is no whole number of 16-byte chunks is padded while converting from NCHW fp32
    c = ce(dtype)
    if Cin % c != 0:
        if g != 1:
            raise Y3DError(f"grouped conv with {Cin} channels is not 16-byte chunkable")
        Cin_k = (Cin + c - 1) // c * c
        xin = nhwc_empty(B, Cin_k, H, W, dtype, x.device)
        lib().nchw_to_nhwc(code(dtype), x.float().contiguous().data_ptr(), xin.data_ptr(), B, Cin, H, W, Cin_k, stream())
    else:
        xin = to_nhwc(x, dtype)
    if dw:
        return _dw_forward(xin, call)
    return _dense_forward(xin, call, Cin, qent, True)


def _stem_image(x):
    """-> (tensor, hwc): uint8 (the dataset's bytes: /255 happens in the kernel) NCHW, or NHWC (hwc = 1) when channels-last; else NCHW fp32"""
    if x.dtype == torch.uint8:
        hwc = int(not x.is_contiguous() and x.permute(0, 2, 3, 1).is_contiguous())
        return (x if (hwc or x.is_contiguous()) else x.contiguous()), hwc
    return x.float().contiguous(), 0


def _stem_forward(x, call):
    """the stem (3 -> Cout, 3x3, stride 2) as a dense 1x1 conv with K = 32 over the im2col rows of the image (27 window values + 5 zeros
    per output pixel); as a 9-tap conv over an 8-channel-padded image the MFMA tiles were 86 % padding.  dW is mapped back in _conv_backward."""
    L, st, dtype, dev = lib(), stream(), _COMPUTE_DTYPE, x.device
    dt = code(dtype)
    w32, act, res_mode, training, cache = call.w32, call.act, call.res_mode, call.training, call.cache
    B, _, H, W = x.shape
    Cout = w32.shape[0]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    wkey = ("stemcol", PARAM_EPOCH, w32.data_ptr(), call.ver[0] if call.ver is not None else w32._version)
    wcol = cache.get(wkey) if (cache is not None and not training) else None
    if wcol is None:
        wcol = torch.zeros(Cout, 32, dtype=torch.float32, device=dev)
        wcol[:, :27] = w32.detach().permute(0, 2, 3, 1).reshape(Cout, 27)  # column (r*3+q)*3+ci
        if cache is not None and not training:  # eval: the im2col form of the stem weight is a constant of the forward
            _cache_put(cache, wkey, wcol)
    call = call._replace(w32=wcol.view(Cout, 32, 1, 1), k=1, s=1, p=0, g=1, bn_apply=True)  # the 1x1 form over 32 im2col channels
    fused = dtype == torch.bfloat16 and Cout % 16 == 0 and 16 <= Cout <= 80 and STEM_FUSED and x.dtype in (torch.uint8, torch.float32)
    if fused and not training and not res_mode:
        # eval: gather + MFMA + folded BatchNorm + SiLU in one pass over the image (csrc/stem_fused.hip); no column tensor
        _, ss = _eval_consts(call, "dense", dtype, 32, 32, Cout)
        xs, hwc = _stem_image(x)
        mode = 1 + hwc if xs.dtype == torch.uint8 else 0
        ye = out_tensor(B, Cout, Ho, Wo, dtype, dev)
        _timed(("conv_eval", dt, B, H, W, 3, Cout, 3, 2, 1, 1),
               lambda: L.stem_conv_eval(xs.data_ptr(), mode, wcol.data_ptr(), ss[0].data_ptr(), ss[1].data_ptr(), int(act), ye.data_ptr(), ye.stride(3),
                                        B, H, W, Cout, st))
        return ye, None, None
    xcol = nhwc_empty(B, 32, Ho, Wo, dtype, dev)
    xs, hwc = _stem_image(x)
    # wcol is built from the already quantised stem weight and repacked per call: no quantiser entry, no version token, no pack registry
    call = call._replace(ver=None)
    if fused and training:
        # training: the same one-pass kernel writes the raw conv output, the BatchNorm partials and - its own B operand - the column
        # tensor the weight gradient reads; the two-step form wrote the column tensor and read it back (im2col 167 us + conv 146 us)
        mode = 1 + hwc if xs.dtype == torch.uint8 else 0
        rows = L.stem_conv_train_rows(B, H, W)
        ypre = nhwc_empty(B, Cout, Ho, Wo, dtype, dev)
        part = _f32(rows * Cout * 2, dev)
        _timed(("conv_fwd", dt, B, H, W, 3, Cout, 3, 2, 1),
               lambda: L.stem_conv_train(xs.data_ptr(), mode, wcol.data_ptr(), ypre.data_ptr(), ypre.stride(3), xcol.data_ptr(), part.data_ptr(), B, H, W, Cout, st))
        z, plan, saved = _bn_act_tail(xcol, ypre, part, rows, None, call, 32, None, None)
    else:
        if xs.dtype == torch.uint8:
            L.stem_im2col_u8(dt, xs.data_ptr(), hwc, xcol.data_ptr(), B, H, W, Ho, Wo, st)
        else:
            L.stem_im2col(dt, xs.data_ptr(), xcol.data_ptr(), B, H, W, Ho, Wo, st)
        z, plan, saved = _dense_forward(xcol, call, 32, None, False)
    return z, (plan._replace(stem=True) if plan is not None else None), saved


def _dw_forward(xin, call):
    """depth-wise conv (one filter per channel): the eval form with folded BatchNorm + SiLU (+res) in its epilogue, or dwconv2d_fwd + the tail"""
    L, st, dtype, dev = lib(), stream(), xin.dtype, xin.device
    k, s, p, act, res, res_mode, training = call.k, call.s, call.p, call.act, call.res, call.res_mode, call.training
    dt = code(dtype)
    B, C, H, W = xin.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    sb, sh, sw = s3(xin)
    fused = not training and call.bn_apply and DW_EVAL_FUSED
    y = None if fused else nhwc_empty(B, C, Ho, Wo, dtype, dev)  # pre-BatchNorm tensor
    nblk = L.dw_blocks(B * Ho * Wo)
    part = ss_eval = None
    if training:
        part = _f32(nblk * C * 2, dev)
        wp = _dw_packed(call.w32, C, k, dtype, _wver(call))
    else:
        wp, ss_eval = _eval_consts(call, "dw", dtype, 1, 1, C)
        if fused:
            # eval: folded BatchNorm + SiLU (+ the RepVGGDW / shortcut residual) in the depth-wise kernel's epilogue - one launch, no
            # pre-BN tensor (12 depth-wise layers of S-3D: 12 bn_act_fwd launches and their read + write less per forward)
            ze = out_tensor(B, C, Ho, Wo, dtype, dev)
            rr = to_nhwc(res, dtype, dense=True) if res_mode else None
            if rr is not None:
                assert rr.shape == ze.shape, "residual shape mismatch"
            L.dwconv2d_fwd_affine(dt, xin.data_ptr(), sb, sh, sw, B, H, W, C, wp.data_ptr(), ss_eval[0].data_ptr(), ss_eval[1].data_ptr(), int(act),
                                  res_mode, rr.data_ptr() if rr is not None else None, rr.stride(3) if rr is not None else 0,
                                  ze.data_ptr(), ze.stride(3), Ho, Wo, k, k, s, p, st)
            return ze, None, None
    L.dwconv2d_fwd(dt, xin.data_ptr(), sb, sh, sw, B, H, W, C, wp.data_ptr(), y.data_ptr(), C, Ho, Wo, k, k, s, p,
                   part.data_ptr() if training else None, st)
    return _bn_act_tail(xin, y, part, nblk, ss_eval, call, C, _wver(call), None)


def _dense_forward(xin, call, Cin, qent, pack_cache):
    """dense / grouped conv over the NHWC input `xin` (Cin: its channels before padding); qent: the quantiser entry of call.w32 (fp8w
    mode) or None; pack_cache: training weight packs go through the registry"""
    L, st, dtype, dev = lib(), stream(), xin.dtype, xin.device
    w32, k, s, p, g, act, res, res_mode, training = call.w32, call.k, call.s, call.p, call.g, call.act, call.res, call.res_mode, call.training
    dt = code(dtype)
    B, Cin_k, H, W = xin.shape
    Cout = w32.shape[0]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    sb, sh, sw = s3(xin)
    wver = _wver(call)
    y = nhwc_empty(B, Cout, Ho, Wo, dtype, dev) if (training or res_mode) else None  # pre-BatchNorm tensor (the eval fast paths have none)
    # fp8 MFMA forward (set_fp8_conv): e4m3 codes of the weight x the MX-quantised activation; everything after the conv - BatchNorm
    # statistics from the partial rows, the apply pass, the bf16 backward over (xin, w_eff) - is the bf16 path's
    f8 = (FP8_CONV and qent is not None and dtype == torch.bfloat16 and k == 3 and s == 1 and p == 1 and Cin_k == Cin
          and bool(L.conv3x3_fp8_ok(B, H, W, Cin, Cout, g)))
    nblk = L.conv3x3_fp8_stat_rows(B, H, W) if f8 else L.conv2d_stat_rows(dt, B, H, W, Cin_k, Cout, g, k, k, s, p)
    part = _f32(nblk * Cout * 2, dev) if training else None
    Cg_pad = Cin_k // g
    wp = ss_eval = None
    if not training:
        wp, ss_eval = _eval_consts(call, "dense", dtype, Cin // g, Cg_pad, Cout)
    if f8:
        xq, xs = fp8_input(xin)
        wq, ws = fp8_weight(qent, Cin // g)
        if not training and not res_mode:
            ye = out_tensor(B, Cout, Ho, Wo, dtype, dev)
            _timed(("conv_eval_fp8", dt, B, H, W, Cin_k, Cout, k, s, g, p),
                   lambda: L.conv3x3_fp8_fwd(xq.data_ptr(), xs.data_ptr(), B, H, W, Cin, wq.data_ptr(), ws.data_ptr(), ye.data_ptr(), ye.stride(3), Cout, g, None,
                                             ss_eval[0].data_ptr(), ss_eval[1].data_ptr(), int(act), st))
            return ye, None, None
        _timed(("conv_fwd_fp8", dt, B, H, W, Cin_k, Cout, k, s, g),
               lambda: L.conv3x3_fp8_fwd(xq.data_ptr(), xs.data_ptr(), B, H, W, Cin, wq.data_ptr(), ws.data_ptr(), y.data_ptr(), y.stride(3), Cout, g,
                                         part.data_ptr() if training else None, None, None, 0, st))
    elif not training and not res_mode:
        # eval: BatchNorm (running statistics) + SiLU folded into the conv epilogue - one launch, no pre-BN tensor; the packed
        # weights and the scale/shift pair are cached until a parameter / buffer is modified in place or re-pointed
        ye = out_tensor(B, Cout, Ho, Wo, dtype, dev)  # a pending placement (C2f / SPPF / Concat slot) is honoured in eval too
        _timed(("conv_eval", dt, B, H, W, Cin_k, Cout, k, s, g, p),
               lambda: L.conv2d_fwd_affine(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin_k, wp.data_ptr(), ss_eval[0].data_ptr(), ss_eval[1].data_ptr(),
                                           int(act), ye.data_ptr(), ye.stride(3), Ho, Wo, Cout, g, k, k, s, p, st))
        return ye, None, None
    elif (not training and res_mode == 1 and dtype == torch.bfloat16
            and L.conv2d_fwd_affine_res_ok(dt, B, H, W, Cin_k, Cout, g, k, k, s, p)):
        # eval Bottleneck shortcut: conv + folded BatchNorm + SiLU + residual in ONE launch (the narrow resident-weight kernel)
        rr = to_nhwc(res, dtype, dense=True)
        ye = out_tensor(B, Cout, Ho, Wo, dtype, dev)
        L.conv2d_fwd_affine_res(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin_k, wp.data_ptr(), ss_eval[0].data_ptr(), ss_eval[1].data_ptr(), int(act),
                                rr.data_ptr(), rr.stride(3), ye.data_ptr(), ye.stride(3), Ho, Wo, Cout, g, k, k, s, p, st)
        return ye, None, None
    else:
        # training, or eval with a residual the epilogue kernel does not serve: conv (eval: the cached packed weights) + the tail's pass
        if training:
            wp = _fwd_packed(w32, Cout, Cin // g, Cg_pad, k, dtype, wver, registry=pack_cache)
        _timed(("conv_fwd", dt, B, H, W, Cin_k, Cout, k, s, g),
               lambda: L.conv2d_fwd(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin_k, wp.data_ptr(), None, y.data_ptr(), Cout, Ho, Wo, Cout, g,
                                    k, k, s, p, part.data_ptr() if training else None, st))
    return _bn_act_tail(xin, y, part, nblk, ss_eval, call, Cin, wver, qent if f8 else None)


def _bn_act_tail(xin, y, part, nblk, ss_eval, call, Cin, wver, fp8_entry):
    """BatchNorm + activation (+res) over the pre-BatchNorm tensor y of a conv that has run.  Training: statistics from the conv's `nblk`
    partial rows `part`; eval: the folded (scale, shift) pair `ss_eval`.  -> (z, plan, saved)"""
    L, st, dtype, dev = lib(), stream(), y.dtype, y.device
    dt = code(dtype)
    w32, g, act, res_mode, training, bn_apply = call.w32, call.g, call.act, call.res_mode, call.training, call.bn_apply
    B, Cin_k, H, W = xin.shape
    _, Cout, Ho, Wo = y.shape
    M = B * Ho * Wo
    plan = ConvPlan(B, Cin, Cin_k, H, W, Cout, Ho, Wo, call.k, call.s, call.p, g, g > 1 and g == Cin and g == Cout, res_mode, training, dtype,
                    int(act), wver, fp8_entry)
    if training:
        stats = _f32(6 * Cout, dev).view(6, Cout)  # mean, invstd, scale, shift, mean_g, mean_gx
        bump_param_epoch()  # bn_finalize updates the running statistics in place
        L.bn_finalize(part.data_ptr(), nblk, Cout, M, call.g32.data_ptr(), call.b32.data_ptr(), call.eps, call.momentum, call.rm.data_ptr(),
                      call.rv.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), stats[3].data_ptr(), st)
    elif not bn_apply:  # eval: the fused consumer reads the cached (scale, shift) pair as rows 2 / 3 of a statistics tensor
        stats = torch.zeros(6, Cout, dtype=torch.float32, device=dev)
        stats[2:4].copy_(ss_eval)
    else:
        stats = None
    if not bn_apply:  # the consumer applies BatchNorm + activation itself (FusedConvBNProjFn): hand back the pre-BN tensor
        return y, plan, (xin, w32, y, stats, None)
    z = out_tensor(B, Cout, Ho, Wo, dtype, dev)
    rr = None
    if res_mode:
        rr = to_nhwc(call.res, dtype, dense=True)
        assert rr.shape == z.shape, "residual shape mismatch"
    sc_t, sh_t = (stats[2], stats[3]) if training else (ss_eval[0], ss_eval[1])
    if _FP8_WANT and dtype == torch.bfloat16 and not res_mode and Cout % 64 == 0 and not plan.dw:
        # the consumer is an fp8 MFMA convolution: this pass also writes z's fp8 copy (e4m3 codes + E8M0 block scales)
        zq = torch.empty(B, Ho, Wo, Cout, dtype=torch.uint8, device=dev)
        zs = torch.empty(B, Ho, Wo, L.fp8_scale_pitch(Cout), dtype=torch.uint8, device=dev)
        L.bn_act_fwd_q(y.data_ptr(), Cout, sc_t.data_ptr(), sh_t.data_ptr(), int(act), z.data_ptr(), z.stride(3), zq.data_ptr(), zs.data_ptr(), M, Cout, st)
        _FP8_ACT[z.data_ptr()] = (zq, zs, (B, Cout, Ho, Wo), z)
    else:
        L.bn_act_fwd(dt, y.data_ptr(), Cout, sc_t.data_ptr(), sh_t.data_ptr(), int(act), res_mode,
                     rr.data_ptr() if rr is not None else None, rr.stride(3) if rr is not None else 0, z.data_ptr(), z.stride(3), M, Cout, st)
    return z, plan, (xin, w32, y, stats, rr if res_mode == 2 else None)


def _cba_backward(plan, saved, dz, need_dx, need_dres, dx_range=None, pre=None, dx_out=None, need_dw=True):
    """-> dx, dW (fp32 OIHW), dgamma, dbeta, dres.  dx_range=(lo, hi): only output channels lo..hi feed dx
    (the one-to-one head sees a detached input, reference head.py:820).  need_dw False (a frozen weight): no weight-gradient launch, no
    slab, no fold, no dW buffer - dW is None; the BatchNorm reduce / finalize still run (their sums feed the apply pass)."""
    L = lib()
    _, _, y, stats, rr = saved
    B, Cout, Ho, Wo, res_mode, dtype, act = plan.B, plan.Cout, plan.Ho, plan.Wo, plan.res_mode, plan.dtype, plan.act
    if not plan.training:
        raise Y3DError("backward through an eval-mode (running-statistics) Conv is not supported")
    if pre is not None:  # (dy, dgb): the BatchNorm part was done by the caller (FusedConvBNProjFn)
        return _conv_backward(plan, saved, pre[0], pre[1], None, need_dx, dx_range, dx_out, need_dw=need_dw)
    dt, st, dev = code(dtype), stream(), dz.device
    M = B * Ho * Wo
    dz = to_nhwc(dz, dtype, dense=True)
    nb = L.bn_bwd_blocks(M, Cout)
    part = _f32(nb * Cout * 2, dev)
    rptr = rr.data_ptr() if rr is not None else None
    rsw = rr.stride(3) if rr is not None else 0
    L.bn_act_bwd_reduce(dt, y.data_ptr(), Cout, dz.data_ptr(), dz.stride(3), rptr, rsw, stats[2].data_ptr(), stats[3].data_ptr(),
                        stats[0].data_ptr(), stats[1].data_ptr(), act, res_mode, part.data_ptr(), M, Cout, st)
    dgb = _f32(2 * Cout, dev).view(2, Cout)
    L.bn_bwd_finalize(part.data_ptr(), nb, Cout, M, dgb[0].data_ptr(), dgb[1].data_ptr(), 0, stats[4].data_ptr(), stats[5].data_ptr(), st)
    dy = nhwc_empty(B, Cout, Ho, Wo, dtype, dev)
    dres = None
    if res_mode == 2 and need_dres:
        dres = nhwc_empty(B, Cout, Ho, Wo, dtype, dev)
    L.bn_act_bwd_apply(dt, y.data_ptr(), Cout, dz.data_ptr(), dz.stride(3), rptr, rsw, stats[2].data_ptr(), stats[3].data_ptr(),
                       stats[0].data_ptr(), stats[1].data_ptr(), stats[4].data_ptr(), stats[5].data_ptr(), act, res_mode, 1,
                       dy.data_ptr(), Cout, dres.data_ptr() if dres is not None else None, Cout, M, Cout, st)
    if res_mode == 1:
        dres = dz
    return _conv_backward(plan, saved, dy, dgb, dres, need_dx, dx_range, dx_out, need_dw=need_dw)


def _fp8_dgrad_plan(plan, need_dx, dx_range):
    """(entry, lo, hi) when the data gradient of this layer runs on the fp8 kernel, else None (the bf16 call runs).  entry: the
    _QuantRegistry entry whose codes it multiplies - the switch is on, the layer's forward took the fp8 kernel and the entry still holds
    the weight version that forward packed"""
    ent = plan.fp8_entry
    if not (FP8_DGRAD and FP8_CONV and need_dx) or ent is None or plan.wver != ((WEIGHT_EPOCH, ent["count"]),):
        return None
    Cin, Cout, g = plan.Cin, plan.Cout, plan.g
    lo, hi = dx_range if dx_range is not None else (0, Cout)
    if plan.Cin_k != Cin or plan.dtype != torch.bfloat16 or (plan.k, plan.s, plan.p) != (3, 1, 1) or (g != 1 and (lo, hi) != (0, Cout)):
        return None
    # a window reads the slab's scale bytes as an aligned dword: lo and hi - lo in whole 128-channel units
    if (lo, hi) != (0, Cout) and (lo % 128 or (hi - lo) % 128):
        return None
    if not lib().conv3x3_fp8_dgrad_ok(plan.B, plan.H, plan.W, Cin, hi - lo, g):
        return None
    return ent, lo, hi


def _conv_backward(plan, saved, dy, dgb, dres, need_dx, dx_range, dx_out=None, registry=True, need_dw=True):
    """data and weight gradients of the conv given dy (gradient wrt its pre-BatchNorm output).  registry False: the data-gradient pack of
    the weight is made on the spot (a weight that is no parameter: the pack registry re-reads its entries' memory once per weight epoch,
    at the first lookup of ANY weight, which may come before the caller has refreshed such a buffer).  need_dw False: the weight-gradient
    half (launch, split-K slab, fold, dW buffer) is left out and dW is None; the data gradient - bf16 or fp8 - is the same call"""
    L = lib()
    xin, w32 = saved[:2]
    B, Cin, Cin_k, H, W, Cout, Ho, Wo = plan.B, plan.Cin, plan.Cin_k, plan.H, plan.W, plan.Cout, plan.Ho, plan.Wo
    k, s, p, g, dtype = plan.k, plan.s, plan.p, plan.g, plan.dtype
    dt, st = code(dtype), stream()
    dev = dy.device
    esz = 2 if dtype == torch.bfloat16 else 4
    M = B * Ho * Wo
    sb, sh, sw = s3(xin)
    dx = None
    dW = torch.empty_like(w32) if need_dw else None
    if plan.dw:
        wp = _dw_packed(w32, Cout, k, dtype, plan.wver)  # (the buffer the forward of this step used)
        if need_dx:
            dx = nhwc_empty(B, Cin, H, W, dtype, dev)
            dsb, dsh, dsw = s3(dy)
            L.dwconv2d_bwd_data(dt, dy.data_ptr(), dsb, dsh, dsw, B, Ho, Wo, Cout, wp.data_ptr(), dx.data_ptr(), Cin, H, W, k, k, s, p, st)
        if need_dw:
            slab = _f32(L.dw_wgrad_blocks(M) * k * k * Cout, dev)
            L.dwconv2d_bwd_weight(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin, dy.data_ptr(), Cout, Ho, Wo, k, k, s, p, slab.data_ptr(),
                                  dW.data_ptr(), 0, st)
    else:
        f8 = _fp8_dgrad_plan(plan, need_dx, dx_range)
        if f8 is not None and not (px_dense(dy) and dy.data_ptr() % 16 == 0 and dy.stride(3) % 8 == 0):
            f8 = None
        if f8 is not None:
            # fp8 data gradient (set_fp8_dgrad): the forward kernel on (dy * row scales -> MX, the forward's codes flipped and swapped)
            qent, lo, hi = f8
            wqd, wsd = fp8_weight_dgrad(qent, Cin, g, lo, hi)
            # dy's fp8 copy: the stand-alone quantiser over the window's channels (a copy written by the BatchNorm-backward apply pass itself
            # measured slower than apply + this pass on the head shapes and is not part of the path: DESIGN.md 3.9)
            co = hi - lo
            dq = torch.empty(B, Ho, Wo, co, dtype=torch.uint8, device=dev)
            ds = torch.empty(B, Ho, Wo, L.fp8_scale_pitch(co), dtype=torch.uint8, device=dev)
            L.fp8_quantize_grad(dy.data_ptr() + lo * esz, dy.stride(3), qent["scale"].data_ptr() + lo * 4, M, co, dq.data_ptr(), ds.data_ptr(), st)
            dx = dx_out if dx_out is not None else nhwc_empty(B, Cin, H, W, dtype, dev)
            if not (px_dense(dx) and dx.data_ptr() % 16 == 0 and dx.stride(3) % 8 == 0):
                raise Y3DError("fp8 data gradient: dx must be a pixel-dense NHWC tensor with 16-byte aligned rows")
            _timed(("conv_dgrad_fp8", dt, B, H, W, Cin, hi - lo, k, s, g),
                   lambda: L.conv3x3_fp8_dgrad(dq.data_ptr(), ds.data_ptr(), co, ds.shape[3], 0, co, B, H, W, wqd.data_ptr(), wsd.data_ptr(),
                                               dx.data_ptr(), dx.stride(3), Cin, g, st))
        elif need_dx and Cin_k == Cin:
            lo, hi = dx_range if dx_range is not None else (0, Cout)
            assert g == 1 or (lo, hi) == (0, Cout)
            co = hi - lo
            wpd = _dgrad_packed(w32, w32.data_ptr() + lo * (Cin // g) * k * k * 4, co, Cin // g, g, k, dtype, plan.wver, registry=registry and not plan.stem)
            dx = dx_out if dx_out is not None else nhwc_empty(B, Cin, H, W, dtype, dev)  # dx_out: a slice of a shared gradient buffer (grad_slot)
            dsb, dsh, dsw = s3(dy)
            _timed(("conv_dgrad", dt, B, H, W, Cin, co, k, s, g),
                   lambda: L.conv2d_bwd_data(dt, dy.data_ptr() + lo * esz, dsb, dsh, dsw, B, Ho, Wo, co, wpd.data_ptr(), dx.data_ptr(), dx.stride(3), H, W,
                                             Cin, g, k, k, s, p, st))
        if need_dw:
            ns = L.conv2d_wgrad_plan(dt, B, H, W, Cin_k, Cout, g, k, k, s, p)
            slab = _f32(ns * Cout * k * k * (Cin_k // g), dev)
            _timed(("conv_wgrad", dt, B, H, W, Cin_k, Cout, k, s, g),
                   lambda: L.conv2d_bwd_weight(dt, xin.data_ptr(), sb, sh, sw, B, H, W, Cin_k, Cin, dy.data_ptr(), Cout, Ho, Wo, Cout, g, k, k,
                                               s, p, slab.data_ptr(), ns, dW.data_ptr(), 0, st))
    if plan.stem:  # [Cout][(r*3+q)*3+ci | 5 zeros] -> OIHW (Cout, 3, 3, 3); the image itself gets no gradient
        if need_dw:
            dW = dW.reshape(Cout, 32)[:, :27].reshape(Cout, 3, 3, 3).permute(0, 3, 1, 2).contiguous()
        dx = None
    return dx, dW, dgb[0], dgb[1], dres


def _w32(weight):
    w = weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    return w


class ConvBNActFn(torch.autograd.Function):
    """act(bn(conv(x))) (+res)   — reference nn/modules/conv.py:120-122 plus the residual adds of
    block.py:342,711,758,816-817 fused into the BN-apply kernel.

    `m` is the owning Conv module (non-tensor): k, s, p, g, act, BN buffers/eps/momentum, training flag."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, res, res_mode, m):
        z, cfg, saved = _cba_forward(x, _module_call(m, w32=_w32(weight), g32=gamma.detach().float(), b32=beta.detach().float(), rm=m.bn.running_mean,
                                                     rv=m.bn.running_var, g=m.g, res=res, res_mode=res_mode,
                                                     cache=m.__dict__.setdefault("_eval_cache", {})))
        if m.training:
            m._nbt_pending += 1
        ctx.cfg = cfg
        if saved is not None:
            ctx.save_for_backward(*saved)
        return z

    @staticmethod
    def backward(ctx, dz):
        if ctx.cfg is None:
            raise Y3DError("backward through an eval-mode (running-statistics) Conv is not supported")
        need = ctx.needs_input_grad  # x, weight, gamma, beta, res: a frozen parameter gets None (and a frozen weight no launch)
        dx, dW, dg, db, dres = _cba_backward(ctx.cfg, ctx.saved_tensors, dz, need[0], need[4], need_dw=need[1])
        return dx, dW, dg if need[2] else None, db if need[3] else None, dres, None, None


class StackedConvs:
    """N sibling Conv modules (same input, kernel, stride) run as ONE convolution with their output channels stacked
    (the 8 branches x 2 head sets of v10Detect3d share their input).  The per-branch Parameters / BN buffers
    keep their identity and state_dict keys; their storage is re-pointed at slices of one flat tensor, so stacking costs
    nothing per step and optimizer / DDP / load_state_dict keep working on the per-branch tensors."""

    def __init__(self, convs, groups=1):
        self.convs = list(convs)
        self.groups = groups
        self.couts = [c.conv.out_channels for c in self.convs]
        self.flat = {}

    def _ensure(self, name, tensors, setter):
        flat = self.flat.get(name)
        ok = flat is not None and flat.device == tensors[0].device
        if ok:
            base, off = flat.data_ptr(), 0
            for t in tensors:
                if t.data_ptr() != base + off * 4:
                    ok = False
                    break
                off += t.numel()
        if not ok:
            flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
            off = 0
            for i, t in enumerate(tensors):
                n = t.numel()
                setter(i, flat[off:off + n].view(t.shape))
                off += n
            self.flat[name] = flat
        return flat

    def tensors(self):
        cs = self.convs
        w = self._ensure("w", [c.conv.weight for c in cs], lambda i, v: setattr(cs[i].conv.weight, "data", v))
        gm = self._ensure("g", [c.bn.weight for c in cs], lambda i, v: setattr(cs[i].bn.weight, "data", v))
        bt = self._ensure("b", [c.bn.bias for c in cs], lambda i, v: setattr(cs[i].bn.bias, "data", v))
        rm = self._ensure("rm", [c.bn.running_mean for c in cs], lambda i, v: cs[i].bn._buffers.__setitem__("running_mean", v))
        rv = self._ensure("rv", [c.bn.running_var for c in cs], lambda i, v: cs[i].bn._buffers.__setitem__("running_var", v))
        c0 = cs[0].conv
        # identity of what the flat tensors hold, as torch sees it: the per-branch tensors' own version counters (the flat views'
        # counters never move: `.data =` shares storage, not the counter)
        wv = tuple(c.conv.weight._version for c in cs)
        self.ver = (wv, wv + tuple(t._version for c in cs for t in (c.bn.weight, c.bn.bias, c.bn.running_mean, c.bn.running_var)))
        return w.view(sum(self.couts), c0.in_channels // c0.groups, *c0.kernel_size), gm, bt, rm, rv

    def params(self):
        return [c.conv.weight for c in self.convs] + [c.bn.weight for c in self.convs] + [c.bn.bias for c in self.convs]


def _stack_grads(dW, dg, db, couts):
    """the per-branch row slices of a stack's gradients in StackedConvs.params() order; dW None (frozen weights): None per branch"""
    return [*(dW.split(couts) if dW is not None else [None] * len(couts)), *dg.split(couts), *db.split(couts)]


def _masked(grads, need):
    """`grads` with None wherever autograd asked for no gradient (a frozen parameter)"""
    return [g if n else None for g, n in zip(grads, need)]


class FusedConvBNActFn(torch.autograd.Function):
    """One conv+BN+SiLU over the stacked output channels of `stack.convs`.  args: x, stack, groups, dx_range, *params
    (params only tie the per-branch Parameters into the autograd graph; the math runs on the stacked storage)."""

    @staticmethod
    def forward(ctx, x, stack, groups, dx_range, *params):
        w, gm, bt, rm, rv = stack.tensors()
        m = stack.convs[0]
        z, cfg, saved = _cba_forward(x, _module_call(m, w32=w, g32=gm, b32=bt, rm=rm, rv=rv, g=groups, ver=stack.ver))
        if m.training:
            for c in stack.convs:
                c._nbt_pending += 1
        ctx.cfg, ctx.couts, ctx.dx_range = cfg, stack.couts, dx_range
        ctx.gslot = grad_slot(x) if (m.training and torch.is_tensor(x) and x.is_cuda) else None
        if saved is not None:
            ctx.save_for_backward(*saved)
        return z

    @staticmethod
    def backward(ctx, dz):
        dx_out = grad_slot_tensor(ctx.gslot) if (ctx.gslot is not None and ctx.needs_input_grad[0]) else None
        need = ctx.needs_input_grad[4:]  # per branch: weights, gammas, betas
        n = len(ctx.couts)
        need_dw = any(need[:n])
        dx, dW, dg, db, _ = _cba_backward(ctx.cfg, ctx.saved_tensors, dz, ctx.needs_input_grad[0], False, ctx.dx_range, dx_out=dx_out, need_dw=need_dw)
        if all(need):
            return (dx, None, None, None, *dW.split(ctx.couts), *dg.split(ctx.couts), *db.split(ctx.couts))  # per-branch row slices of the stack
        return (dx, None, None, None, *_masked(_stack_grads(dW, dg, db, ctx.couts), need))


# ------------------------------------------------------------------------------------------------------
# channel slices of one map for several consumers
# ------------------------------------------------------------------------------------------------------
class SplitChannelsFn(torch.autograd.Function):
    """x[:, o_j : o_j + m_j] for every j as strided views (no copy); the backward writes the consumers' gradients side by side into
    ONE tensor.  Plain slicing makes autograd zero-fill a full-size tensor per slice and add them up pairwise: with the 16 branches
    of a non-uniform head (M-3D: 128-channel cls next to 64-channel regression branches) that was 15 full-map adds per level.
    Round 3: consumers that end their backward in a data-gradient kernel (FusedConvBNActFn / FusedConvBNProjFn) write it straight
    into their slice of one shared buffer (`grad_slot`), so a dense split returns that buffer without the concatenation either."""

    @staticmethod
    def forward(ctx, x, offs, widths):
        ctx.offs, ctx.widths, ctx.C = tuple(offs), tuple(widths), x.shape[1]
        covered = sorted(zip(offs, widths))
        ctx.dense = covered[0][0] == 0 and all(a + w == b for (a, w), (b, _) in zip(covered, covered[1:])) and covered[-1][0] + covered[-1][1] == x.shape[1]
        ctx.order = [j for _, j in sorted((o, j) for j, o in enumerate(offs))]
        outs = tuple(x[:, o:o + w] for o, w in zip(offs, widths))
        ctx.holder = None
        if ctx.dense and x.is_cuda and len(set(offs)) == len(offs) and all(o % ce(x.dtype) == 0 and w % ce(x.dtype) == 0 for o, w in zip(offs, widths)):
            ctx.holder = {"buf": None, "C": x.shape[1], "shape": (x.shape[0], x.shape[2], x.shape[3]), "dtype": x.dtype, "device": x.device}
            ctx.keys = []
            for v, o in zip(outs, offs):
                k = (v.data_ptr(), v.shape[1])
                _GRAD_SLOT[k] = (ctx.holder, o)
                ctx.keys.append(k)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        ref = next(g for g in grads if g is not None)
        B, _, H, W = ref.shape
        if ctx.holder is not None:
            for k in ctx.keys:
                _GRAD_SLOT.pop(k, None)
            buf = ctx.holder["buf"]
            esz = ref.element_size()
            if buf is not None and all(g is not None and g.dtype == buf.dtype and g.data_ptr() == buf.data_ptr() + o * esz and g.shape[1] == w
                                       and g.stride() == buf[:, o:o + w].stride() for g, o, w in zip(grads, ctx.offs, ctx.widths)):
                return buf, None, None  # every consumer wrote its slice in place
        if ctx.dense and all(g is not None for g in grads):
            parts = [to_nhwc(grads[j], ref.dtype, dense=True).permute(0, 2, 3, 1) for j in ctx.order]  # physical (B, H, W, c_j)
            return torch.cat(parts, 3).permute(0, 3, 1, 2), None, None
        dx = nhwc_empty(B, ctx.C, H, W, ref.dtype, ref.device)
        dx.zero_()
        for g, o, w in zip(grads, ctx.offs, ctx.widths):
            if g is not None:
                dx[:, o:o + w].add_(g)
        return dx, None, None


class InjectRowsFn(torch.autograd.Function):
    """Identity on the first head layer's output `z` ahead of the second layer, for feature distillation (loss.DistillFn): the
    distillation gradient is non-zero at the foreground anchors of two channel slices of `z` only.  Through autograd's slice backward
    it would be a zero-filled tensor of z's size plus a full-size add (S-3D, level 0, batch 32: 839 MB each way).  Instead the loss
    leaves its compact rows in `slot["entries"]`, its backward - which runs earlier in the same pass: the head maps it is tied to are
    made from this function's output - leaves the scale, and the backward here adds scale * rows into the gradient the second layer
    has just produced (csrc/distill.hip, y3d_distill_scatter: one wave per row) and hands that same tensor on.
    The add is IN PLACE on the gradient this backward is handed.  That assumes nobody else holds that tensor: z1's only consumer is
    layer 2 (or the channel split in front of it), whose backward makes a fresh tensor, and no `retain_grad` / tensor hook sits on
    this function's output.  A second consumer of the output would make autograd sum into a new tensor first, which is also fine."""

    @staticmethod
    def forward(ctx, z, slot):
        ctx.slot = slot
        return z.view_as(z)

    @staticmethod
    def backward(ctx, g):
        entries = ctx.slot.pop("entries", ())
        live = [e for e in entries if e["scale"] is not None]
        if g is None or not live:
            return g, None
        dt = live[0]["rows"].dtype
        g = to_nhwc(g, dt)
        sb, sh, sw = s3(g)
        B, _, H, W = g.shape
        for e in live:
            lib().distill_scatter(code(dt), e["rows"].data_ptr(), e["idx"].data_ptr(), e["nrows"].data_ptr(), e["scale"].data_ptr(), e["cap"],
                                  e["C"], g.data_ptr() + e["off"] * g.element_size(), sb, sh, sw, e["a0"], H, W, stream())
        return g, None


class C2fSplitFn(torch.autograd.Function):
    """`y = list(cv1(x).chunk(2, 1))` of C2f (reference block.py:233) with the second half handed out TWICE (it feeds the first block and
    the concat): -> (y0, y1 for the concat, y1 for the block), all views.  Plain chunk + reuse makes autograd (a) add the two
    gradients of y1 with a strided-operand elementwise kernel and (b) assemble the gradient of the chunked tensor from zero-filled
    full-size pieces.  Here the backward adds the block's gradient INTO the concat gradient's slice (`y3d_add2d`, in place: that slice
    of the concat gradient has no other reader) and returns the first two slices of that buffer as one strided view - no copy at all
    when the two concat gradients are neighbours in one buffer, one gather otherwise."""

    @staticmethod
    def forward(ctx, t):
        c = t.shape[1] // 2
        ctx.c = c
        return t[:, :c], t[:, c:], t[:, c:]

    @staticmethod
    def backward(ctx, d0, d1a, d1b):
        L, st, c = lib(), stream(), ctx.c
        ref = next(g for g in (d0, d1a, d1b) if g is not None)
        dtype, dev = ref.dtype, ref.device
        B, _, H, W = ref.shape
        dt = code(dtype)
        esz = ref.element_size()
        P = B * H * W
        ok = lambda g: g is not None and g.dtype == dtype and is_nhwc(g) and g.data_ptr() % 16 == 0 and g.stride(3) % ce(dtype) == 0 and px_dense(g)
        if (d0 is not None and d1a is not None and ok(d0) and ok(d1a) and d0.stride() == d1a.stride()
                and d1a.data_ptr() == d0.data_ptr() + c * esz and d0.stride(3) >= 2 * c):
            if d1b is not None:
                d1b = to_nhwc(d1b, dtype, dense=True)
                L.add2d(dt, d1a.data_ptr(), d1a.stride(3), d1b.data_ptr(), d1b.stride(3), d1a.data_ptr(), d1a.stride(3), P, c, st)
            return torch.as_strided(d0, (B, 2 * c, H, W), d0.stride(), d0.storage_offset())
        out = nhwc_empty(B, 2 * c, H, W, dtype, dev)
        if d0 is None:
            out[:, :c].zero_()
        else:
            d0 = to_nhwc(d0, dtype, dense=True)
            L.copy2d(dt, d0.data_ptr(), d0.stride(3), out.data_ptr(), 2 * c, P, c, st)
        parts = [to_nhwc(g, dtype, dense=True) for g in (d1a, d1b) if g is not None]
        if not parts:
            out[:, c:].zero_()
        elif len(parts) == 1:
            L.copy2d(dt, parts[0].data_ptr(), parts[0].stride(3), out.data_ptr() + c * esz, 2 * c, P, c, st)
        else:
            L.add2d(dt, parts[0].data_ptr(), parts[0].stride(3), parts[1].data_ptr(), parts[1].stride(3), out.data_ptr() + c * esz, 2 * c, P, c, st)
        return out


# ------------------------------------------------------------------------------------------------------
# plain nn.Conv2d(c, out, 1) with bias (head projections)
# ------------------------------------------------------------------------------------------------------
class HeadProjFn(torch.autograd.Function):
    """cat_j( conv1x1_j(x_j) + b_j ) written straight into one (B, sum(out_j), H, W) NHWC tensor
    (reference head.py:637 + the torch.cat of head.py:742).  args: n, x_0..x_{n-1}, w_0.., b_0.."""

    @staticmethod
    def forward(ctx, n, *args):
        L = lib()
        xs, ws, bs = args[:n], args[n:2 * n], args[2 * n:3 * n]
        dtype = _COMPUTE_DTYPE
        dt, st = code(dtype), stream()
        B, _, H, W = xs[0].shape
        P = B * H * W
        couts = [w.shape[0] for w in ws]
        tot = sum(couts)
        out = nhwc_empty(B, tot, H, W, dtype, xs[0].device)
        esz = out.element_size()
        xs = [to_nhwc(x, dtype, dense=True) for x in xs]
        w32 = [w.detach().float().contiguous() for w in ws]
        b32 = [b.detach().float().contiguous() for b in bs]
        off, wide = 0, []
        for x, w, b, co in zip(xs, w32, b32, couts):
            Cin = x.shape[1]
            # wide projections (the 2D head's 64 box-distribution and nc class outputs): a 1x1 conv with bias on the MFMA kernels,
            # written into its channel slice of `out`; the VALU kernel below is for the 3D head's 1..24 outputs per branch
            mf = co >= 32 and co % 8 == 0 and off % 8 == 0 and tot % 8 == 0 and Cin % 8 == 0
            wide.append(mf)
            if mf:
                wp = _fwd_packed(w, co, Cin, Cin, 1, dtype)  # (on the spot: these weights are no entries of the pack registry)
                sb, sh, sw = s3(x)
                L.conv2d_fwd(dt, x.data_ptr(), sb, sh, sw, B, H, W, Cin, wp.data_ptr(), b.data_ptr(), out.data_ptr() + off * esz, tot, H, W, co,
                             1, 1, 1, 1, 0, None, st)
            else:
                for o0 in range(0, co, 24):
                    oc = min(24, co - o0)
                    L.proj_fwd(dt, x.data_ptr(), x.stride(3), w.data_ptr() + o0 * w.shape[1] * 4, b.data_ptr() + o0 * 4,
                               out.data_ptr() + (off + o0) * esz, tot, P, x.shape[1], oc, st)
            off += co
        ctx.n, ctx.couts, ctx.dtype, ctx.wide = n, couts, dtype, wide
        ctx.save_for_backward(*xs, *w32)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = lib()
        n, couts, dtype = ctx.n, ctx.couts, ctx.dtype
        xs, ws = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        dt, st = code(dtype), stream()
        if not (dout.dtype == dtype and px_dense(dout)):
            dout = to_nhwc(dout, dtype, dense=True) if dout.shape[1] % ce(dtype) == 0 else _dense_any(dout, dtype)
        B, tot, H, W = dout.shape
        P = B * H * W
        dev = dout.device
        esz = dout.element_size()
        dsw = dout.stride(3)
        nb = L.proj_blocks(P)
        dxs, dws, dbs, off = [], [], [], 0
        need = ctx.needs_input_grad
        for j, (x, w, co) in enumerate(zip(xs, ws, couts)):
            Cin = x.shape[1]
            dx = dW = db = None
            need_w, need_b = need[1 + n + j], need[1 + 2 * n + j]  # a frozen branch: neither the weight-gradient launch nor the bias sums
            if ctx.wide[j]:
                dptr = dout.data_ptr() + off * esz
                dsb, dsh, _ = s3(dout)
                if ctx.needs_input_grad[1 + j]:
                    wpd = _dgrad_packed(w, w.data_ptr(), co, Cin, 1, 1, dtype)
                    dx = nhwc_empty(B, Cin, H, W, dtype, dev)
                    L.conv2d_bwd_data(dt, dptr, dsb, dsh, dsw, B, H, W, co, wpd.data_ptr(), dx.data_ptr(), Cin, H, W, Cin, 1, 1, 1, 1, 0, st)
                if need_w:
                    sb, sh, sw = s3(x)
                    ns = L.conv2d_wgrad_plan(dt, B, H, W, Cin, co, 1, 1, 1, 1, 0)
                    slab = _f32(ns * co * Cin, dev)
                    dW = torch.empty_like(w)
                    L.conv2d_bwd_weight(dt, x.data_ptr(), sb, sh, sw, B, H, W, Cin, Cin, dptr, dsw, H, W, co, 1, 1, 1, 1, 0, slab.data_ptr(), ns,
                                        dW.data_ptr(), 0, st)
                if need_b:
                    nbb = L.bn_bwd_blocks(P, co)  # bias gradient: column sums of the dout slice
                    part = _f32(nbb * co * 2, dev)
                    L.colsum_partials(dt, dptr, dsw, part.data_ptr(), P, co, st)
                    db, scratch = _f32(co, dev), _f32(2 * co, dev)
                    L.bn_bwd_finalize(part.data_ptr(), nbb, co, P, None, db.data_ptr(), 0, scratch.data_ptr(), scratch.data_ptr() + 4 * co, st)
            else:
                if ctx.needs_input_grad[1 + j]:
                    dx = nhwc_empty(B, Cin, H, W, dtype, dev)
                    for o0 in range(0, co, 24):  # 24 outputs per launch; the later chunks go through a temporary and are added
                        tgt = dx if o0 == 0 else nhwc_empty(B, Cin, H, W, dtype, dev)
                        L.proj_bwd_data(dt, dout.data_ptr() + (off + o0) * esz, dsw, w.data_ptr() + o0 * Cin * 4, tgt.data_ptr(), Cin, P, Cin,
                                        min(24, co - o0), st)
                        if o0:
                            L.add2d(dt, dx.data_ptr(), Cin, tgt.data_ptr(), Cin, dx.data_ptr(), Cin, P, Cin, st)
                if need_w or need_b:  # one launch makes both: with one of the two frozen the other half is computed and dropped
                    dW, db = torch.empty_like(w), _f32(co, dev)
                    slab, bslab = _f32(nb * co * Cin, dev), _f32(nb * co, dev)
                    L.proj_bwd_weight(dt, x.data_ptr(), x.stride(3), dout.data_ptr() + off * esz, dsw, slab.data_ptr(), bslab.data_ptr(),
                                      dW.data_ptr(), db.data_ptr(), 0, P, Cin, co, st)
                    dW, db = (dW if need_w else None), (db if need_b else None)
            dxs.append(dx)
            dws.append(dW)
            dbs.append(db)
            off += co
        return (None, *dxs, *dws, *dbs)


# What the grouped head projections (proj_group.hip, proj_bn_mfma.hip) take per launch: branch j projects channels [offsets[j],
# offsets[j] + cin) of one stacked tensor to couts[j] outputs (tot in all).  w32 / b32: the fp32 weights and biases; c_w / c_b / c_off /
# c_co: the ctypes arrays of their addresses, of the offsets and of the output counts.
ProjGroup = namedtuple("ProjGroup", "n cin couts tot w32 b32 c_w c_b c_off c_co")


def _proj_group(ws, bs, offsets, cin):
    """the ProjGroup of weights `ws` and biases `bs` (none: a backward, which launches nothing that reads them)"""
    n = len(ws)
    assert n <= 16, "grouped projections: at most 16 branches"
    couts = [w.shape[0] for w in ws]
    w32 = [w.detach().float().contiguous() for w in ws]
    b32 = [b.detach().float().contiguous() for b in bs]
    PV, IA = ctypes.c_void_p * n, ctypes.c_int * n
    return ProjGroup(n, cin, couts, sum(couts), w32, b32, PV(*[t.data_ptr() for t in w32]), PV(*[t.data_ptr() for t in b32]) if b32 else None,
                     IA(*offsets), IA(*couts))


def _proj_wgrad_buffers(pg, nb, dev):
    """the weight-gradient side of a ProjGroup for a launch of `nb` blocks: per-branch dW / db, the split slabs, and the ctypes arrays of
    the dW / db addresses -> (dws, dbs, slab, bslab, c_dw, c_db)"""
    dws = [torch.empty_like(w) for w in pg.w32]
    dbs = [_f32(co, dev) for co in pg.couts]
    PV = ctypes.c_void_p * pg.n
    return (dws, dbs, _f32(nb * pg.tot * pg.cin, dev), _f32(nb * pg.tot, dev), PV(*[t.data_ptr() for t in dws]), PV(*[t.data_ptr() for t in dbs]))


def _proj_mfma(dtype, cin):
    """the projections (and the BatchNorm backward through them) run on the matrix-core kernels of proj_bn_mfma.hip"""
    return dtype == torch.bfloat16 and cin in (64, 128) and PROJ_BN_MFMA


def proj_slices_eval(x, offsets, cin, ws, bs):
    """eval form of HeadProjSlicesFn (no graph): branch j projects channels [offsets[j], offsets[j] + cin) of the ACTIVATED features x with
    its 1x1 conv + bias (head.py:637), all branches in one launch.  bf16 with 64 / 128 channels per branch: the matrix-core kernel of
    the training head (proj_bn_mfma.hip) with an identity BatchNorm (scale 1, shift 0, no activation) - the VALU form
    (y3d_proj_group_fwd) took 42 us per level for the 1 600 candidate pixels of a batch of 32 (128-long serial dot products)."""
    n = len(ws)
    dtype = _COMPUTE_DTYPE
    if not (_proj_mfma(dtype, cin) and n <= 16):
        return HeadProjSlicesFn.apply(x, offsets, [cin] * n, n, *ws, *bs)
    x = to_nhwc(x, dtype, dense=True)
    B, Ct, H, W = x.shape
    pg = _proj_group(ws, bs, offsets, cin)
    out = nhwc_empty(B, pg.tot, H, W, dtype, x.device)
    ident = _identity_bn(Ct, x.device)
    lib().proj_group_fwd_bn_mfma(n, cin, x.data_ptr(), x.stride(3), pg.c_off, pg.c_w, pg.c_b, pg.c_co, ident[0].data_ptr(), ident[1].data_ptr(), 0,
                                 out.data_ptr(), pg.tot, B * H * W, stream())
    return out


class HeadProjSlicesFn(torch.autograd.Function):
    """Same projections as HeadProjFn, but every branch reads a channel slice [off_j, off_j+cin) of ONE stacked feature
    tensor, all branches of a level run as ONE launch per direction (proj_group.hip) and the backward writes each branch's
    input gradient straight into its slice of one gradient tensor.  args: x_full, offsets, cins, n, w_0.., b_0.."""

    @staticmethod
    def forward(ctx, x, offsets, cins, n, *args):
        L = lib()
        ws, bs = args[:n], args[n:2 * n]
        dtype = _COMPUTE_DTYPE
        x = to_nhwc(x, dtype, dense=True)
        B, Ct, H, W = x.shape
        cin = cins[0]
        assert all(c == cin for c in cins), "HeadProjSlicesFn: uniform branch width"
        pg = _proj_group(ws, bs, offsets, cin)
        out = nhwc_empty(B, pg.tot, H, W, dtype, x.device)
        L.proj_group_fwd(code(dtype), n, cin, x.data_ptr(), x.stride(3), pg.c_off, pg.c_w, pg.c_b, pg.c_co, out.data_ptr(), pg.tot, B * H * W, stream())
        ctx.meta = (list(offsets), cin, dtype)
        ctx.save_for_backward(x, *pg.w32)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = lib()
        offsets, cin, dtype = ctx.meta
        x, ws = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        dt, st = code(dtype), stream()
        if not (dout.dtype == dtype and px_dense(dout)):
            dout = _dense_any(dout, dtype)
        B, Ct, H, W = x.shape
        P = B * H * W
        dev = x.device
        pg = _proj_group(ws, (), offsets, cin)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = nhwc_empty(B, Ct, H, W, dtype, dev)
            if pg.n * cin != Ct:
                dx.zero_()
            L.proj_group_bwd_data(dt, pg.n, cin, dout.data_ptr(), dout.stride(3), pg.c_off, pg.c_w, pg.c_co, dx.data_ptr(), Ct, P, st)
        need = ctx.needs_input_grad[4:]  # the weights, then the biases
        if not any(need):  # a frozen head: no weight-gradient launch, no slabs
            return (dx, None, None, None, *([None] * len(need)))
        dws, dbs, slab, bslab, c_dw, c_db = _proj_wgrad_buffers(pg, L.proj_group_blocks(P), dev)
        L.proj_group_bwd_weight(dt, pg.n, cin, x.data_ptr(), x.stride(3), pg.c_off, dout.data_ptr(), dout.stride(3), pg.c_co, slab.data_ptr(),
                                bslab.data_ptr(), c_dw, c_db, P, st)
        if all(need):
            return (dx, None, None, None, *dws, *dbs)
        return (dx, None, None, None, *_masked(dws + dbs, need))


class FusedConvBNProjFn(torch.autograd.Function):
    """Second stacked head layer + the 16 projections of a level as ONE node: grouped conv -> BatchNorm statistics -> projections
    that apply BatchNorm + SiLU on the fly (proj_group.hip).  The activation tensor is never materialised: the forward reads the
    pre-BN tensor once instead of bn_act_fwd's read + write + the projections' read, and the projection weight gradient rebuilds
    the activation from the pre-BN tensor.  (A fully fused backward - BatchNorm reduce / apply recomputing W^T dout per pixel on the
    VALU - was measured slower than the three separate kernels and is not used.)  args: x, stack, groups, offsets, cins, n, *stack.params(), *proj_w, *proj_b"""

    @staticmethod
    def forward(ctx, x, stack, groups, offsets, cins, n, *params):
        L = lib()
        w, gm, bt, rm, rv = stack.tensors()
        m = stack.convs[0]
        npar = len(params) - 2 * n
        ws, bs = params[npar:npar + n], params[npar + n:]
        ctx.gslot = grad_slot(x) if (m.training and x.is_cuda) else None
        y, cfg, saved = _cba_forward(x, _module_call(m, w32=w, g32=gm, b32=bt, rm=rm, rv=rv, g=groups, bn_apply=False, ver=stack.ver))
        if m.training:
            for c in stack.convs:
                c._nbt_pending += 1
        dtype = _COMPUTE_DTYPE
        dt, st = code(dtype), stream()
        B, Ct, H, W = y.shape
        P = B * H * W
        cin = cins[0]
        assert all(c == cin for c in cins) and n * cin == Ct and cin % 64 == 0
        pg = _proj_group(ws, bs, offsets, cin)
        out = nhwc_empty(B, pg.tot, H, W, dtype, y.device)
        stats = saved[3]
        tail = (y.data_ptr(), y.stride(3), pg.c_off, pg.c_w, pg.c_b, pg.c_co, stats[2].data_ptr(), stats[3].data_ptr(), int(m.has_act), out.data_ptr(),
                pg.tot, P, st)
        if _proj_mfma(dtype, cin):
            L.proj_group_fwd_bn_mfma(n, cin, *tail)
        else:
            L.proj_group_fwd_bn(dt, n, cin, *tail)
        ctx.cfg, ctx.couts_stack, ctx.meta = cfg, stack.couts, (list(offsets), cin, dtype, int(m.has_act))
        ctx.save_for_backward(*[t for t in saved if t is not None], *pg.w32)
        ctx.none_mask = [t is None for t in saved]
        return out

    @staticmethod
    def backward(ctx, dout):
        L = lib()
        offsets, cin, dtype, act = ctx.meta
        it = iter(ctx.saved_tensors)
        saved = tuple(None if isnone else next(it) for isnone in ctx.none_mask)
        pg = _proj_group(list(it), (), offsets, cin)
        y, stats = saved[2], saved[3]
        dt, st = code(dtype), stream()
        if not (dout.dtype == dtype and px_dense(dout)):
            dout = _dense_any(dout, dtype)
        B, Ct, H, W = y.shape
        P = B * H * W
        dev = y.device
        n, c_w, c_off, c_co = pg.n, pg.c_w, pg.c_off, pg.c_co
        mfma = _proj_mfma(dtype, cin)
        dx_out = grad_slot_tensor(ctx.gslot) if (ctx.gslot is not None and ctx.needs_input_grad[0]) else None
        ns = len(ctx.couts_stack)
        need_stack, need_proj = ctx.needs_input_grad[6:6 + 3 * ns], ctx.needs_input_grad[6 + 3 * ns:]
        need_dw = any(need_stack[:ns])
        if any(need_proj):
            nb = L.proj_group_bwd_weight_bn_mfma_blocks(P) if mfma else L.proj_group_blocks(P)
            dws, dbs, slab, bslab, c_dw, c_db = _proj_wgrad_buffers(pg, nb, dev)
            tail = (y.data_ptr(), y.stride(3), c_off, dout.data_ptr(), dout.stride(3), c_co, stats[2].data_ptr(), stats[3].data_ptr(), act, slab.data_ptr(),
                    bslab.data_ptr(), c_dw, c_db, P, st)
            if mfma:
                L.proj_group_bwd_weight_bn_mfma(n, cin, *tail)
            else:
                L.proj_group_bwd_weight_bn(dt, n, cin, *tail)
        else:  # frozen projections: their weight-gradient launch, slabs and folds are left out
            dws, dbs = [None] * n, [None] * n
        if mfma and ctx.cfg.training:
            # BatchNorm backward straight from `dout`: dz = dout . W is recomputed on the matrix cores by the reduce and the apply pass
            # (proj_bn_mfma.hip) instead of being written once and read twice (839 MB at the stride-8 level)
            nblk = L.proj_group_bn_bwd_blocks(P)
            part = _f32(nblk * Ct * 2, dev)
            args = (n, cin, y.data_ptr(), y.stride(3), c_off, dout.data_ptr(), dout.stride(3), c_w, c_co, stats[2].data_ptr(), stats[3].data_ptr(),
                    stats[0].data_ptr(), stats[1].data_ptr())
            L.proj_group_bn_bwd(0, *args, None, None, act, part.data_ptr(), nblk, None, 0, P, Ct, st)
            dgb = _f32(2 * Ct, dev).view(2, Ct)
            L.bn_bwd_finalize(part.data_ptr(), nblk, Ct, P, dgb[0].data_ptr(), dgb[1].data_ptr(), 0, stats[4].data_ptr(), stats[5].data_ptr(), st)
            dy = nhwc_empty(B, Ct, H, W, dtype, dev)
            L.proj_group_bn_bwd(1, *args, stats[4].data_ptr(), stats[5].data_ptr(), act, None, 0, dy.data_ptr(), Ct, P, Ct, st)
            dx, dW, dg, db, _ = _cba_backward(ctx.cfg, saved, None, ctx.needs_input_grad[0], False, None, pre=(dy, dgb), dx_out=dx_out, need_dw=need_dw)
        else:
            dz = nhwc_empty(B, Ct, H, W, dtype, dev)
            L.proj_group_bwd_data(dt, n, cin, dout.data_ptr(), dout.stride(3), c_off, c_w, c_co, dz.data_ptr(), Ct, P, st)
            dx, dW, dg, db, _ = _cba_backward(ctx.cfg, saved, dz, ctx.needs_input_grad[0], False, None, dx_out=dx_out, need_dw=need_dw)
        cs = ctx.couts_stack
        if all(need_stack) and all(need_proj):
            return (dx, None, None, None, None, None, *dW.split(cs), *dg.split(cs), *db.split(cs), *dws, *dbs)
        return (dx, None, None, None, None, None, *_masked(_stack_grads(dW, dg, db, cs), need_stack), *_masked(dws + dbs, need_proj))


def _dense_any(x, dtype):
    """pixel-dense NHWC copy without the 16-byte channel constraint (head maps with 38 / 144 channels)"""
    B, C, H, W = x.shape
    out = nhwc_empty(B, C, H, W, dtype, x.device)
    out.copy_(x)
    return out


# ------------------------------------------------------------------------------------------------------
# graph glue
# ------------------------------------------------------------------------------------------------------
class ConcatFn(torch.autograd.Function):
    """torch.cat(xs, 1) on NHWC tensors (Concat conv.py:404; C2f/SPPF/PSA cats). Backward returns channel-slice views."""

    @staticmethod
    def forward(ctx, *xs):
        L = lib()
        dtype = _COMPUTE_DTYPE
        dt = code(dtype)
        st = stream()
        B, _, H, W = xs[0].shape
        cs = [x.shape[1] for x in xs]
        tot = sum(cs)
        ctx.cs = cs
        # inputs that already sit in their slice of one tot-channel NHWC buffer (ops.place) are not copied
        esz = 2 if dtype == torch.bfloat16 else 4
        out, inplace, off = None, [False] * len(xs), 0
        for i, (x, c) in enumerate(zip(xs, cs)):
            if (PLACEMENT and x.dtype == dtype and x.is_cuda and is_nhwc(x) and x.stride(3) == tot and x.stride(2) == W * tot
                    and x.stride(0) == H * W * tot):
                base = x.data_ptr() - off * esz
                if out is None and _CONCAT_BASE.get(base, (None, None))[0] == tot:
                    del _CONCAT_BASE[base]
                    out = torch.as_strided(x, (B, tot, H, W), x.stride(), x.storage_offset() - off)
                    assert out.data_ptr() == base
                    inplace[i] = True
                elif out is not None and out.data_ptr() == base:
                    inplace[i] = True
            off += c
        if out is None:
            out = nhwc_empty(B, tot, H, W, dtype, xs[0].device)
        off = 0
        for i, (x, c) in enumerate(zip(xs, cs)):
            if not inplace[i]:
                x = to_nhwc(x, dtype, dense=True)
                L.copy2d(dt, x.data_ptr(), x.stride(3), out.data_ptr() + off * esz, tot, B * H * W, c, st)
            off += c
        return out

    @staticmethod
    def backward(ctx, dout):
        outs, off = [], 0
        for c in ctx.cs:
            outs.append(dout[:, off:off + c])
            off += c
        return tuple(outs)


class MaxPoolFn(torch.autograd.Function):
    """nn.MaxPool2d(k, 1, k//2) (SPPF block.py:171)"""

    @staticmethod
    def forward(ctx, x, k):
        L = lib()
        dtype = _COMPUTE_DTYPE
        dt = code(dtype)
        x = to_nhwc(x, dtype)
        B, C, H, W = x.shape
        y = out_tensor(B, C, H, W, dtype, x.device)
        need = x.requires_grad
        arg = torch.empty(B * H * W * C, dtype=torch.uint8, device=x.device) if need else None
        sb, sh, sw = s3(x)
        L.maxpool_fwd(dt, x.data_ptr(), sb, sh, sw, y.data_ptr(), y.stride(3), arg.data_ptr() if need else None, B, H, W, C, k, stream())
        ctx.k = k
        ctx.dtype = dtype
        if need:
            ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = lib()
        (arg,) = ctx.saved_tensors
        dtype = ctx.dtype
        dy = to_nhwc(dy, dtype, dense=True)
        B, C, H, W = dy.shape
        dx = nhwc_empty(B, C, H, W, dtype, dy.device)
        L.maxpool_bwd(code(dtype), dy.data_ptr(), dy.stride(3), arg.data_ptr(), dx.data_ptr(), C, B, H, W, C, ctx.k, stream())
        return dx, None


class Upsample2xFn(torch.autograd.Function):
    """nn.Upsample(None, 2, 'nearest')"""

    @staticmethod
    def forward(ctx, x):
        L = lib()
        dtype = _COMPUTE_DTYPE
        x = to_nhwc(x, dtype)
        B, C, H, W = x.shape
        y = out_tensor(B, C, 2 * H, 2 * W, dtype, x.device)
        sb, sh, sw = s3(x)
        L.upsample2x_fwd(code(dtype), x.data_ptr(), sb, sh, sw, y.data_ptr(), y.stride(3), B, H, W, C, stream())
        ctx.dtype = dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        L = lib()
        dtype = ctx.dtype
        dy = to_nhwc(dy, dtype)
        B, C, H2, W2 = dy.shape
        dx = nhwc_empty(B, C, H2 // 2, W2 // 2, dtype, dy.device)
        sb, sh, sw = s3(dy)
        L.upsample2x_bwd(code(dtype), dy.data_ptr(), sb, sh, sw, dx.data_ptr(), C, B, H2 // 2, W2 // 2, C, stream())
        return dx


class AttentionFn(torch.autograd.Function):
    """softmax(q^T k * scale) applied to v, per head, on the NHWC qkv tensor; also returns v re-laid-out as
    (B, nh*hd, H, W) for the `pe` branch (reference block.py:785-797)."""

    @staticmethod
    def forward(ctx, qkv, nh, kd, hd, scale):
        L = lib()
        dtype = _COMPUTE_DTYPE
        dt = code(dtype)
        st = stream()
        qkv = to_nhwc(qkv, dtype, dense=True)
        B, Ct, H, W = qkv.shape
        N = H * W
        C = nh * hd
        dev = qkv.device
        out = nhwc_empty(B, C, H, W, dtype, dev)
        v = nhwc_empty(B, C, H, W, dtype, dev)
        lse = _f32(B * nh * N, dev)
        L.attn_fwd(dt, qkv.data_ptr(), qkv.stride(3), out.data_ptr(), C, lse.data_ptr(), B, N, nh, kd, hd, scale, st)
        esz = qkv.element_size()
        for h in range(nh):
            L.copy2d(dt, qkv.data_ptr() + (h * (2 * kd + hd) + 2 * kd) * esz, qkv.stride(3), v.data_ptr() + h * hd * esz, C, B * N, hd, st)
        ctx.cfg = (nh, kd, hd, scale, dtype)
        ctx.save_for_backward(qkv, out, lse)
        return out, v

    @staticmethod
    def backward(ctx, dout, dv):
        L = lib()
        qkv, out, lse = ctx.saved_tensors
        nh, kd, hd, scale, dtype = ctx.cfg
        dt = code(dtype)
        B, Ct, H, W = qkv.shape
        N = H * W
        C = nh * hd
        dev = qkv.device
        if dout is None:
            dout = torch.zeros_like(out)
        dout = to_nhwc(dout, dtype, dense=True)
        dvp, dvs = None, 0
        if dv is not None:
            dv = to_nhwc(dv, dtype, dense=True)
            dvp, dvs = dv.data_ptr(), dv.stride(3)
        dqkv = nhwc_empty(B, Ct, H, W, dtype, dev)
        delta = _f32(B * nh * N, dev)
        L.attn_bwd(dt, qkv.data_ptr(), qkv.stride(3), out.data_ptr(), C, dout.data_ptr(), dout.stride(3), dvp, dvs, lse.data_ptr(),
                   delta.data_ptr(), dqkv.data_ptr(), Ct, B, N, nh, kd, hd, scale, stream())
        return dqkv, None, None, None, None


# ---- depth predictor of the 3D head (modules.DepthPredictor, reference head.py:978-1042) -----------------------------------------------
# Conv2d (with bias) + GroupNorm(32, 128) pairs.  The conv writes its raw output without the bias (conv2d_fwd with bias None keeps the
# fast 3x3 / streaming 1x1 routes); the GroupNorm kernels of csrc/group_norm.hip add it.  Conv data / weight gradients are _conv_backward's.
GN_C, GN_G = 128, 32


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _gn_maps(who, ts):
    """the (B, C, H, W) maps of one GroupNorm call: same shape and dtype, pixel-dense NHWC on a HIP device"""
    t0 = ts[0]
    for t in ts:
        _require_gpu(t)
        if t.shape != t0.shape or t.dtype != t0.dtype or t.dim() != 4:
            raise Y3DError(f"{who}: the maps must share one (B, C, H, W) shape and dtype")
        if not (is_nhwc(t) and px_dense(t)):
            raise Y3DError(f"{who}: the maps must be pixel-dense NHWC tensors")
    return t0.shape, t0.dtype, t0.device


def _gn_vecs(who, vs, C):
    out = []
    for v in vs:
        _require_gpu(v)
        v = v.detach()
        if v.dtype != torch.float32 or not v.is_contiguous():
            v = v.float().contiguous()
        if v.numel() != C:
            raise Y3DError(f"{who}: per-channel vectors must hold {C} values (got {v.numel()})")
        out.append(v)
    return out


def gn_forward(ys, bconvs, gammas, betas, eps=1e-5, scale=1.0, relu=False, groups=GN_G, out=None):
    """out = act(scale * sum_i GroupNorm_i(ys[i] + bconvs[i])) over 1 or 3 raw conv outputs -> (out, stats); stats [nsrc][B][G][2] =
    (mean, rstd) for gn_backward.  Two launches: chunk statistics, then the apply pass that folds them in its prologue."""
    (B, C, H, W), dtype, dev = _gn_maps("gn_forward", ys)
    n = len(ys)
    bconvs, gammas, betas = _gn_vecs("gn_forward", bconvs, C), _gn_vecs("gn_forward", gammas, C), _gn_vecs("gn_forward", betas, C)
    L, st, dt = lib(), stream(), code(dtype)
    if out is None:
        out = nhwc_empty(B, C, H, W, dtype, dev)
    else:
        _gn_maps("gn_forward", [out, ys[0]])
    sw = (ctypes.c_int64 * n)(*[y.stride(3) for y in ys])
    part = _f32(n * B * max(L.gn_chunks(H * W), 1) * groups * 2, dev)
    stats = _f32(n * B * groups * 2, dev)
    L.gn_stats(dt, n, _ptrs(ys), sw, _ptrs(bconvs), B, H * W, C, groups, part.data_ptr(), st)
    L.gn_apply(dt, n, _ptrs(ys), sw, _ptrs(bconvs), _ptrs(gammas), _ptrs(betas), part.data_ptr(), float(eps), float(scale), int(relu),
               out.data_ptr(), out.stride(3), stats.data_ptr(), B, H * W, C, groups, st)
    return out, stats


def gn_backward(ys, bconvs, gammas, betas, stats, dz, scale=1.0, relu=False, groups=GN_G, dys=None):
    """-> (dys, dgamma, dbeta, dbconv): the gradient wrt every raw conv output (compute dtype, pixel-dense) and the (nsrc, C) fp32 parameter
    gradients, given dz = gradient wrt gn_forward's out.  Two launches: reduce, apply."""
    (B, C, H, W), dtype, dev = _gn_maps("gn_backward", list(ys) + [dz])
    n = len(ys)
    bconvs, gammas, betas = _gn_vecs("gn_backward", bconvs, C), _gn_vecs("gn_backward", gammas, C), _gn_vecs("gn_backward", betas, C)
    L, st, dt = lib(), stream(), code(dtype)
    if dys is None:
        dys = [nhwc_empty(B, C, H, W, dtype, dev) for _ in range(n)]
    else:
        _gn_maps("gn_backward", list(dys) + [ys[0]])
    sw = (ctypes.c_int64 * n)(*[y.stride(3) for y in ys])
    dsw = (ctypes.c_int64 * n)(*[d.stride(3) for d in dys])
    part = _f32(B * max(L.gn_chunks(H * W), 1) * (2 * n + 1) * C, dev)
    dpar = _f32(3 * n * C, dev).view(3, n, C)
    args = (dt, n, _ptrs(ys), sw, _ptrs(bconvs), _ptrs(gammas), _ptrs(betas), stats.data_ptr(), float(scale), int(relu), dz.data_ptr(), dz.stride(3),
            part.data_ptr())
    L.gn_bwd_reduce(*args, B, H * W, C, groups, st)
    L.gn_bwd_apply(*args, _ptrs(dys), dsw, dpar[0].data_ptr(), dpar[1].data_ptr(), dpar[2].data_ptr(), B, H * W, C, groups, st)
    return dys, dpar[0], dpar[1], dpar[2]


def resize_bilinear(x, size):
    """F.interpolate(x, size=size, mode="bilinear", align_corners=False) of an NHWC map (C % 8 == 0) on the HIP kernel of csrc/resize.hip"""
    _require_gpu(x)
    x = to_nhwc(x, x.dtype if x.dtype in (torch.float32, torch.bfloat16) else None)
    B, C, H, W = x.shape
    y = nhwc_empty(B, C, size[0], size[1], x.dtype, x.device)
    lib().resize_bilinear_fwd(code(x.dtype), x.data_ptr(), *s3(x), y.data_ptr(), y.stride(3), B, H, W, size[0], size[1], C, stream())
    return y


def resize_bilinear_adjoint(dy, size):
    """the adjoint of resize_bilinear from (H, W) = `size`: dx (B, C, H, W) given dy (B, C, Ho, Wo)"""
    _require_gpu(dy)
    dy = to_nhwc(dy, dy.dtype if dy.dtype in (torch.float32, torch.bfloat16) else None, dense=True)
    B, C, Ho, Wo = dy.shape
    dx = nhwc_empty(B, C, size[0], size[1], dy.dtype, dy.device)
    lib().resize_bilinear_bwd(code(dy.dtype), dy.data_ptr(), dy.stride(3), dx.data_ptr(), dx.stride(3), B, size[0], size[1], Ho, Wo, C, stream())
    return dx


class ResizeBilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        ctx.size = tuple(x.shape[2:])
        return resize_bilinear(x, size)

    @staticmethod
    def backward(ctx, dy):
        return resize_bilinear_adjoint(dy, ctx.size), None


def _raw_conv(x, w32, k, s, p):
    """y = conv(x, w) without bias, dense, groups 1 -> (xin, y, plan): the operands _conv_backward takes"""
    _require_gpu(x)
    dtype = _COMPUTE_DTYPE
    xin = to_nhwc(x.detach(), dtype)
    B, Cin, H, W = xin.shape
    Cout = w32.shape[0]
    if Cin % ce(dtype) or w32.shape[1] != Cin:
        raise Y3DError(f"conv over {Cin} input channels: a multiple of {ce(dtype)} that matches the weight's {w32.shape[1]} is needed")
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = nhwc_empty(B, Cout, Ho, Wo, dtype, xin.device)
    wp = _fwd_packed(w32, Cout, Cin, Cin, k, dtype, None, registry=True)
    lib().conv2d_fwd(code(dtype), xin.data_ptr(), *s3(xin), B, H, W, Cin, wp.data_ptr(), None, y.data_ptr(), Cout, Ho, Wo, Cout, 1, k, k, s, p,
                     None, stream())
    return xin, y, ConvPlan(B, Cin, Cin, H, W, Cout, Ho, Wo, k, s, p, 1, False, 0, True, dtype, 0, None, None)


class ConvGroupNormFn(torch.autograd.Function):
    """out = act(scale * sum_i GroupNorm(conv_i(x_i) + b_i)) for 1 or 3 branches of Conv2d(c_i, 128, k_i, s_i, p_i) + GroupNorm(32, 128).
    apply(spec, x_0, w_0, b_0, gamma_0, beta_0, x_1, ...); spec = (((k, s, p), ...), eps, scale, relu, (H, W)).  A branch whose conv output
    is not (H, W) is resized to it bilinearly AFTER the conv: conv and resize are linear and the
    bilinear weights sum to 1, so conv(resize(x)) + b = resize(conv(x)) + b, at a quarter of the conv's work for a 2x map."""

    @staticmethod
    def forward(ctx, spec, *args):
        geo, eps, scale, relu, size = spec
        srcs, saved, plans = [], [], []
        for i, (k, s, p) in enumerate(geo):
            x, w, b, gamma, beta = args[5 * i:5 * i + 5]
            w32 = _w32(w)
            xin, y, plan = _raw_conv(x, w32, k, s, p)
            if w32.shape[0] != GN_C:
                raise Y3DError(f"ConvGroupNormFn: the GroupNorm kernels are built for {GN_C} channels in {GN_G} groups (got {w32.shape[0]})")
            if (plan.Ho, plan.Wo) != tuple(size):
                y = resize_bilinear(y, size)
            srcs.append(y)
            plans.append(plan)
            saved += [xin, w32, y, b.detach(), gamma.detach(), beta.detach()]
        out, stats = gn_forward(srcs, saved[3::6], saved[4::6], saved[5::6], eps, scale, relu)
        ctx.plans, ctx.spec = plans, spec
        ctx.save_for_backward(stats, *saved)
        return out

    @staticmethod
    def backward(ctx, dz):
        geo, eps, scale, relu, size = ctx.spec
        stats, *saved = ctx.saved_tensors
        dtype = ctx.plans[0].dtype
        dz = to_nhwc(dz, dtype, dense=True)
        dys, dgamma, dbeta, dbconv = gn_backward(saved[2::6], saved[3::6], saved[4::6], saved[5::6], stats, dz, scale, relu)
        grads = [None]
        for i, plan in enumerate(ctx.plans):
            xin, w32 = saved[6 * i], saved[6 * i + 1]
            dy = dys[i]
            if (plan.Ho, plan.Wo) != tuple(size):
                dy = resize_bilinear_adjoint(dy, (plan.Ho, plan.Wo))
            need = ctx.needs_input_grad[1 + 5 * i:6 + 5 * i]  # x, w, b, gamma, beta of branch i
            dx, dW = _conv_backward(plan, (xin, w32), dy, (None, None), None, need[0], None, need_dw=need[1])[:2]
            # (the GroupNorm apply pass folds dgamma / dbeta / db_conv beside dy: frozen ones are computed and dropped here)
            grads += _masked([dx, dW, dbconv[i], dgamma[i], dbeta[i]], need)
        return tuple(grads)


CLS_PAD = 8  # the depth classifier's 81 output channels run as 88: the data / weight gradient kernels take whole 16-byte chunks of Cout


class DepthClassifierFn(torch.autograd.Function):
    """logits = Conv2d(128, 81, 1)(x) (head.py:1014, 1034) on a weight zero-padded to 88 rows: the logits live in an 88-channel NHWC
    buffer whose pad columns are 0 (zero weight rows, zero bias), the result is its [:, :81] view; the backward pads the logits'
    gradient with +0 columns, runs _conv_backward at 88 channels and slices dW back.  apply(x, weight, bias, wpad, bpad): wpad / bpad are
    the caller's persistent padded fp32 buffers, refreshed here."""

    @staticmethod
    def forward(ctx, x, weight, bias, wpad, bpad):
        co = weight.shape[0]
        wpad[:co].copy_(weight.detach())
        bpad[:co].copy_(bias.detach())
        _require_gpu(x)
        dtype = _COMPUTE_DTYPE
        xin = to_nhwc(x.detach(), dtype)
        B, Cin, H, W = xin.shape
        cp = wpad.shape[0]
        z = nhwc_empty(B, cp, H, W, dtype, xin.device)
        # packed on the spot, here and in the backward: a registry entry of wpad would be repacked at the first lookup of any weight after
        # an optimizer step - possibly before the refresh above - and then count as current: last step's classifier
        wp = _fwd_packed(wpad, cp, Cin, Cin, 1, dtype, None, registry=False)
        lib().conv2d_fwd(code(dtype), xin.data_ptr(), *s3(xin), B, H, W, Cin, wp.data_ptr(), bpad.data_ptr(), z.data_ptr(), cp, H, W, cp, 1, 1, 1, 1, 0,
                         None, stream())
        ctx.plan = ConvPlan(B, Cin, Cin, H, W, cp, H, W, 1, 1, 0, 1, False, 0, True, dtype, 0, None, None)
        ctx.co = co
        # (wpad rides outside save_for_backward: the next forward refreshes it in place - with the same values until an optimizer step)
        ctx.wpad = wpad
        ctx.save_for_backward(xin)
        return z[:, :co]

    @staticmethod
    def backward(ctx, dz):
        (xin,), wpad = ctx.saved_tensors, ctx.wpad
        plan, co = ctx.plan, ctx.co
        B, cp, H, W = plan.B, plan.Cout, plan.H, plan.W
        dy = torch.zeros((B, H, W, cp), dtype=plan.dtype, device=dz.device).permute(0, 3, 1, 2)  # the pad columns: +0
        dy[:, :co].copy_(dz)
        L = lib()
        M = B * H * W
        need = ctx.needs_input_grad
        db = None
        if need[2]:
            part = _f32(L.colsum_blocks(M) * cp, dz.device)
            db = _f32(cp, dz.device)
            L.colsum(code(plan.dtype), dy.data_ptr(), cp, M, cp, part.data_ptr(), db.data_ptr(), stream())
            db = db[:co]
        dx, dW = _conv_backward(plan, (xin, wpad), dy, (None, None), None, need[0], None, registry=False, need_dw=need[1])[:2]
        return dx, dW[:co] if need[1] else None, db, None, None


def depth_expect(logits, bins):
    """weighted_depth = sum_c softmax(logits)_c * bins[c] (head.py:1036-1037) -> (B, h, w) fp32, one launch.  No gradient: nothing in the
    reference consumes it (the fgdm loss reads the logits); call it under no_grad."""
    _require_gpu(logits)
    z = logits.detach()
    B, C, h, w = z.shape
    c = ce(z.dtype)
    if not (z.dtype in (torch.float32, torch.bfloat16) and is_nhwc(z) and px_dense(z) and z.stride(3) % c == 0 and z.stride(3) >= -(-C // c) * c
            and z.data_ptr() % 16 == 0):
        pad = nhwc_empty(B, -(-C // c) * c, h, w, z.dtype if z.dtype in (torch.float32, torch.bfloat16) else _COMPUTE_DTYPE, z.device)
        pad[:, :C].copy_(z)
        z = pad[:, :C]
    out = torch.empty(B, h, w, dtype=torch.float32, device=z.device)
    bins = bins.detach().float().contiguous()
    lib().depth_expect(code(z.dtype), z.data_ptr(), z.stride(3), B * h * w, C, bins.data_ptr(), out.data_ptr(), stream())
    return out
