"""Losses + task-aligned assignment for the YOLOv10 (2D) and YOLOv10-3D heads — device side.

Mirrors the reference interfaces (utils/loss.py: v8DetectionLoss :157, v10DetectLoss :727, DetectLoss3d :740,
DDDetectionLoss :774; utils/tal.py: TaskAlignedAssigner :19, TaskAlignedAssigner3d :355;
utils/keypoint_utils.py; utils/metrics.py:78 bbox_iou).  All arithmetic is fp32 (the reference runs these
under autocast's fp32 policy), on the tensors' own device.

Both training losses (3D: DetectLoss3d / DDDetectionLoss, 2D: v10DetectLoss / v8DetectionLoss — target padding, assignment, the loss
terms and the gradient wrt the head maps) run on the fused HIP kernels of csrc/tal_loss3d.hip / tal_loss2d.hip (`Loss3dFn`,
`DualLoss3dFn`, `Loss2dFn`).  Tie rule of the top-k is pinned to lowest-index-first.  Torch formulations of the
assigners used as test comparators live in tests/torch_assigners.py, not here.

The glue between the criteria and the kernels passes named records: `LossCfg3d` / `LossCfg2d` (what a head set's
kernels are told), `Levels` (the per-level ctypes arrays of a launch) and `SetResult` (a head set's outputs, the assignment's `scal`
words among them: the distillation item is handed its own set's).

Feature distillation (`distillation: True`; SupervisionLoss.forward_head :1156-1188): the seventh item of each 3D head set runs on
csrc/distill.hip (`DistillFn`) over a teacher feature map the caller supplies (batch["teacher_emb"] or `set_teacher`); the DINOv2
teacher network itself is not part of the package.

Hierarchical task learning (`htl: True`, engine/trainer.py:398-400): `DetectLoss3d.set_item_weights(table)` makes both 3D routes read 12
device weights (train.HtlWeights) in the kernel `y3d_loss3d_weighted`: gradient rows times the weight of their item, loss = sum(w * items).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import ctypes
from typing import NamedTuple, Optional

from . import ops
from ._lib import Y3DError, lib
from .modules import make_anchors


_OVERFLOW_PENDING = []  # (event, pinned int32[1], cap) of pad_targets launches whose per-image box count has not been looked at yet
TARGET_CAP = 64  # rows per image the assigner kernels take (tal_loss3d.hip / tal_loss2d.hip)
CROWDED_CAPS = tuple(range(128, 513, 64))  # `max_boxes` of the 2D losses: rows per image on the crowded route of tal_loss2d.hip


def check_max_boxes(max_boxes):
    """the opt-in per-image capacity of the 2D losses: None (64 rows, the dense assigner) or a multiple of 64 in 128..512"""
    if max_boxes is None:
        return None
    if isinstance(max_boxes, bool) or not isinstance(max_boxes, int) or max_boxes not in CROWDED_CAPS:
        raise ValueError(f"max_boxes must be None or a multiple of 64 in 128..512 (got {max_boxes!r})")
    return max_boxes


def check_target_overflow(wait=False):
    """Raise Y3DError if a `pad_targets` launch met an image with more boxes than its capacity (its surplus boxes were dropped).
    The count comes back through a pinned host word behind an event: `pad_targets` polls the finished ones at its next call (the
    training step keeps running without a host synchronisation and the error surfaces a step or two late); wait=True synchronises
    on all of them (validators, tests)."""
    keep = []
    for ev, host, cap in _OVERFLOW_PENDING:
        if wait:
            ev.synchronize()
        if not ev.query():
            keep.append((ev, host, cap))
            continue
        n = int(host[0])
        if n > cap:
            _OVERFLOW_PENDING[:] = keep
            if cap == TARGET_CAP:
                raise Y3DError(f"pad_targets: an image of a recent batch has {n} ground-truth boxes, the assigner kernels take at most {cap} per "
                               f"image (KITTI's max_objs is 50); its last {n - cap} boxes were not trained on")
            raise Y3DError(f"pad_targets: an image of a recent batch has {n} ground-truth boxes, the capacity in use is {cap} per image "
                           f"(the 2D losses' max_boxes); its last {n - cap} boxes were not trained on")
    _OVERFLOW_PENDING[:] = keep


def pad_targets(rows, B, width, scale_xy, cap=TARGET_CAP):
    """utils/loss.py:795-810 on the HIP kernel `y3d_pad_targets`: ragged rows (nbox, 1+width) -> (B, cap, width) + the device-side
    largest per-image box count.  The reference sizes the padded tensor with a host-side `counts.max()`; here the capacity is fixed
    (`cap`: the assigner kernels' limit of 64 rows, KITTI's max_objs is 50, data/datasets/kitti.py:23; or the 2D losses' `max_boxes`) and the count stays on the
    device, so the step has no host synchronisation.  An image with more than `cap` boxes (crowded 2D data, mosaics) is NOT trained
    on silently truncated targets: the true count travels to a pinned host word asynchronously and `check_target_overflow` raises
    (ADVICE round 2).  -> (gt (B, cap, width) fp32, n_used (1,) int32: min(largest count, cap))"""
    if not rows.is_cuda:
        raise Y3DError("pad_targets runs on the HIP kernel of tal_loss3d.hip: the batch must live on a HIP device (no CPU fallback)")
    capturing = torch.cuda.is_current_stream_capturing()
    if not capturing:
        check_target_overflow()
    rows = rows.float().contiguous()
    out = torch.empty(B, cap, width, dtype=torch.float32, device=rows.device)
    n_used = torch.empty(2, dtype=torch.int32, device=rows.device)  # [min(count, cap), true count]
    lib().pad_targets(rows.data_ptr(), rows.shape[0], width, B, cap, float(scale_xy[0]), float(scale_xy[1]), out.data_ptr(), n_used.data_ptr(),
                      ops.stream())
    if capturing:  # no read-back inside a hipGraph capture: graph.GraphedTrainStep reads this (static) word back after every replay
        _CAPTURED_COUNTS.append((n_used, cap))
    else:
        watch_target_count(n_used, cap)
    return out, n_used[:1]


_CAPTURED_COUNTS = []  # (n_used, cap) of the pad_targets launches recorded into the hipGraph being captured


def watch_target_count(n_used, cap):
    """queue an asynchronous read-back of n_used[1] (the true largest per-image box count) for check_target_overflow"""
    host = torch.empty(1, dtype=torch.int32).pin_memory()
    host.copy_(n_used[1:2], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _OVERFLOW_PENDING.append((ev, host, cap))
    if len(_OVERFLOW_PENDING) > 64:  # a caller that never lets the stream drain: look now
        check_target_overflow(wait=True)


def _flatten_maps(feats):
    """list of (B, no, H, W) NHWC maps -> (B, A, no) fp32 (a free view per level + one cat)"""
    B, no = feats[0].shape[:2]
    return torch.cat([f.permute(0, 2, 3, 1).reshape(B, -1, no) for f in feats], 1).float()


class LossCfg3d(NamedTuple):
    """what one 3D head set's kernels are told (`DDDetectionLoss.cfg`)"""
    strides: list
    nc: int
    topk: int
    alpha: float
    beta: float
    gamma: float
    weights: tuple  # the six gains (loss2d, cls, depth, offset3d, size3d, heading)
    mode: int = 11  # assigner mode bits (include/y3d.h: y3d_tal3d_assign); default tal_2d | tal_3d | constrain_anchors, l1
    item_w: Optional[torch.Tensor] = None  # 6 device floats (`set_item_weights`): the y3d_loss3d_weighted entry
    store_grads: bool = True  # False (a weighted call under no_grad): no gradient rows are stored


class LossCfg2d(NamedTuple):
    """what one 2D head set's kernels are told (`v8DetectionLoss.cfg`)"""
    strides: list
    nc: int
    topk: int
    alpha: float
    beta: float
    weights: tuple  # the three gains (box, cls, dfl)


class SetResult(NamedTuple):
    """one head set's outputs.  scal: the assignment's two device words [max(sum(target_scores), 1), n_fg] (the distillation item
    divides by the first, loss.py:898; they never visit the host).  total: 1 float = sum(item_w * items) of the weighted entry, else None"""
    items: torch.Tensor
    fg: torch.Tensor  # (B, A) uint8
    gt_idx: torch.Tensor  # (B, A) int32
    target_scores: torch.Tensor  # (B, A, nc)
    scal: torch.Tensor
    total: Optional[torch.Tensor] = None

    def outputs(self):
        """the six outputs of Loss3dFn / Loss2dFn (and each half of DualLoss3dFn's twelve): the differentiable total first"""
        total = self.total.reshape(()) if self.total is not None else self.items.sum()
        return (total, *self[:5])

    @classmethod
    def of(cls, six):
        return cls(*six[1:], six[0])


class Levels:
    """the per-level arguments of a launch, built once per call from raw pointers (DualLoss3dFn offsets them by a channel count):
    nl, A = sum(H * W), and the ctypes arrays maps, psw (pixel strides), H, W, st (strides; None where the kernel takes none)"""
    __slots__ = ("nl", "A", "maps", "psw", "H", "W", "st")

    def __init__(self, ptrs, psw, Hs, Ws, strides=None):
        nl = self.nl = len(ptrs)
        self.A = sum(h * w for h, w in zip(Hs, Ws))
        self.maps, self.psw = (ctypes.c_void_p * nl)(*ptrs), (ctypes.c_int64 * nl)(*psw)
        self.H, self.W = (ctypes.c_int * nl)(*Hs), (ctypes.c_int * nl)(*Ws)
        self.st = (ctypes.c_float * nl)(*strides) if strides is not None else None

    @classmethod
    def of(cls, maps, strides=None, offset=0):
        """of (B, C, H, W) NHWC maps, read `offset` bytes behind their first element"""
        return cls([m.data_ptr() + offset for m in maps], [m.stride(3) for m in maps], [m.shape[2] for m in maps], [m.shape[3] for m in maps], strides)

    def rows(self, ptrs, psw):
        """the gradient-row arguments: (pointer array or None: nothing is stored, pixel strides)"""
        return (ctypes.c_void_p * self.nl)(*ptrs) if ptrs is not None else None, (ctypes.c_int64 * self.nl)(*psw)


def _check_maps(maps, who, what="head maps"):
    """every map of a call lives on a HIP device with its channels dense per pixel"""
    if not all(m.is_cuda and ops.px_dense(m) for m in maps):
        raise Y3DError(f"{who}: {what} must be pixel-dense NHWC tensors on a HIP device")


def _assignment_buffers(nfloats, who, B, A, nc, dev):
    """what an assigner writes: (scratch of `nfloats`, fg (B, A) uint8, gt_idx (B, A) int32, target_scores (B, A, nc), scal (2,))"""
    if nfloats < 0:
        raise Y3DError(f"{who}: assignment scratch exceeds 2^31 floats")
    return (torch.empty(nfloats, dtype=torch.float32, device=dev), torch.empty(B, A, dtype=torch.uint8, device=dev),
            torch.empty(B, A, dtype=torch.int32, device=dev), torch.empty(B, A, nc, dtype=torch.float32, device=dev),
            torch.empty(2, dtype=torch.float32, device=dev))


def _item_buffers(B, A, k, dev):
    """(per-block partial sums, the k loss items) of a loss launch: one block per 256 anchors"""
    return torch.empty((B * A + 255) // 256 * k, dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.float32, device=dev)


def _head_inputs(crit, dim, preds, batch, targets):
    """the opening of both criteria: preds -> (feats, device, B, image (w, h), targets or None: the batch has no box, maps in the compute dtype)"""
    feats = preds[1] if isinstance(preds, tuple) else preds
    dev = feats[0].device
    if not feats[0].is_cuda:
        raise Y3DError(f"the {dim} loss runs on the HIP kernels of tal_loss{dim.lower()}.hip: head maps must live on a HIP device (no CPU fallback)")
    B, (H, W) = feats[0].shape[0], feats[0].shape[2:]
    if targets is None:
        targets = crit.targets(batch, B, H, W, dev)
    dt = ops.compute_dtype()
    maps = None if targets is None else [f if f.dtype == dt else f.to(dt) for f in feats]
    return feats, dev, B, (W * crit.stride[0], H * crit.stride[0]), targets, maps


def _close_forward(ctx, grads, nmaps, *sets):
    """the close of the three forwards: the gradient rows kept for the backward -> the six outputs of every set, all but the totals
    non-differentiable"""
    ctx.save_for_backward(*grads)
    ctx.nmaps = nmaps
    ctx.set_materialize_grads(False)  # no zero-filled gradients for the assignment outputs
    out = tuple(t for r in sets for t in r.outputs())
    ctx.mark_non_differentiable(*[t for i, t in enumerate(out) if i % 6])
    return out


def _scaled_rows(ctx, d_total, lead):
    """the backward of Loss3dFn / Loss2dFn: the rows the forward stored times the incoming scalar, one multiply per level"""
    grads = ctx.saved_tensors
    if d_total is None or not grads:
        return (None,) * (lead + ctx.nmaps)
    return (None,) * lead + tuple(g * d_total.to(g.dtype) for g in grads)


_TEACHER = None


def set_teacher(fn):
    """Register the distillation teacher: a callable with `DinoDepther.forward`'s contract, `(depth_maps, embeddings) = fn(img)` with
    embeddings (B, C, h, w) on the HIP device, C = width of the depth branch.  It is called once per step under torch.no_grad() when
    the batch carries no "teacher_emb" entry, and both head sets share its result.  None unregisters.  -> the previous callable"""
    global _TEACHER
    prev, _TEACHER = _TEACHER, fn
    return prev


def get_teacher():
    return _TEACHER


def teacher_map(batch, C=None, fn=None, like=None):
    """the teacher feature map of a step: batch["teacher_emb"], else `fn` / the registered callable on batch["img"]
    (utils/loss.py:1159-1160).  C: expected channel count; like: a tensor whose batch size and device the map must share"""
    t = batch.get("teacher_emb")
    fn = fn if fn is not None else _TEACHER
    if t is None:
        if fn is None:
            raise Y3DError('distillation needs a teacher feature map: pass it as batch["teacher_emb"] (B, C, h, w) or register a callable '
                           "with loss.set_teacher(fn), (depth_maps, embeddings) = fn(img); the DINOv2 teacher itself is not part of this package")
        with torch.no_grad():
            t = fn(batch["img"])[1]
    if not (torch.is_tensor(t) and t.dim() == 4):
        raise ValueError("distillation: the teacher map must be a (B, C, h, w) tensor")
    if not t.is_cuda:
        raise Y3DError("distillation runs on the HIP kernels of distill.hip: the teacher map must live on a HIP device (no CPU fallback)")
    if C is not None and t.shape[1] != C:
        raise ValueError(f"distillation: the teacher map has {t.shape[1]} channels, the depth branch of the head is {C} wide")
    if like is not None:
        check_teacher(t, like)
    t = t.detach()
    return t if t.dtype in (torch.float32, ops.compute_dtype()) else t.float()


def check_teacher(t, emb):
    """the kernel reads teacher image b for every image b of the embeddings, on the embeddings' device"""
    if t.shape[0] != emb.shape[0]:
        raise ValueError(f"distillation: the teacher map holds {t.shape[0]} images, the batch {emb.shape[0]}")
    if t.device != emb.device:
        raise ValueError(f"distillation: the teacher map lives on {t.device}, the head's embeddings on {emb.device}")
    if t.shape[1] != emb.shape[1]:
        raise ValueError(f"distillation: the teacher map has {t.shape[1]} channels, the depth branch of the head is {emb.shape[1]} wide")


CRITERIA = {"soft": 0, "mse": 1, "cos": 2}


class DistillFn(torch.autograd.Function):
    """utils/loss.py:893-898 + 1156-1188 for one head set on the HIP kernels of csrc/distill.hip: the distillation item (weighted,
    divided by the target-score sum) and its gradient wrt the depth branch's first-layer embeddings, as compact rows.
    apply(spec, *tensors) -> item (0-dim fp32).  spec: dict(embs, teacher, gt, fg, gi, scal, mixed, img_wh, T, weight, crit, no_mixup,
    cap, slots, which).  Two ways back into the head:
      * slots is None: `tensors` are the embeddings (one (B, C, H, W) NHWC map per level) and the backward returns their dense
        gradients (zeros + scattered rows) - the per-branch head.
      * slots (one per level, made by v10Detect3d.forward_train_fused): the embeddings are channel slices of z1 and take NO gradient
        through autograd; `tensors` are the head maps, given only so that this backward runs before the head's.  The rows are left in
        the slots, this backward adds the scale, and ops.InjectRowsFn adds scale * rows into z1's gradient.
    The valid rows of every image of `gt` must be a prefix of its rows (pad_targets lays them out so): target_gt_idx indexes padded
    rows here, valid rows in the reference.  An image with boxes but no foreground anchor contributes 0 (the reference: NaN)."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        L = lib()
        embs, teacher, gt, fg = spec["embs"], spec["teacher"], spec["gt"], spec["fg"]
        dtype, dev = embs[0].dtype, embs[0].device
        _check_maps(embs, "DistillFn", "embeddings")
        if dtype != ops.compute_dtype() or not all(ops.is_nhwc(e) for e in embs):
            raise Y3DError("DistillFn: embeddings must be NHWC tensors of the compute dtype")
        B, C = embs[0].shape[:2]
        lv = Levels.of(embs)
        A, n, cap = lv.A, gt.shape[1], int(spec["cap"])
        if fg.shape != (B, A):
            raise ValueError(f"DistillFn: fg_mask {tuple(fg.shape)} does not match the {B} x {A} anchors of the embeddings")
        check_teacher(teacher, embs[0])
        if spec["mixed"] is not None and spec["mixed"].numel() != B:
            raise ValueError(f"DistillFn: {spec['mixed'].numel()} `mixed` flags for {B} images")
        if gt.shape[0] != B or spec["gi"].shape != (B, A):
            raise ValueError(f"DistillFn: targets {tuple(gt.shape)} / target_gt_idx {tuple(spec['gi'].shape)} do not match {B} images x {A} anchors")
        counts = torch.empty(B + 2, dtype=torch.int32, device=dev)
        idx = torch.empty(cap, 2, dtype=torch.int32, device=dev)
        rows = torch.empty(cap, C, dtype=dtype, device=dev)
        part = torch.empty((cap + 3) // 4, dtype=torch.float32, device=dev)
        item = torch.empty(1, dtype=torch.float32, device=dev)
        mixed = spec["mixed"]
        L.distill_loss(ops.code(dtype), lv.nl, lv.maps, lv.psw, lv.H, lv.W, B, C, teacher.data_ptr(), ops.code(teacher.dtype), teacher.shape[2],
                       teacher.shape[3], *teacher.stride(), gt.data_ptr(), n, fg.data_ptr(), spec["gi"].data_ptr(), spec["scal"].data_ptr(),
                       mixed.data_ptr() if mixed is not None else None, int(spec["img_wh"][0]), int(spec["img_wh"][1]), float(spec["T"]),
                       float(spec["weight"]), int(spec["crit"]), int(bool(spec["no_mixup"])), cap, counts.data_ptr(), idx.data_ptr(), rows.data_ptr(),
                       part.data_ptr(), item.data_ptr(), ops.stream())
        ctx.entries, a0 = [], 0
        for h, w in zip(lv.H, lv.W):
            ctx.entries.append({"rows": rows, "idx": idx, "nrows": counts[B:], "cap": cap, "C": C, "a0": a0, "scale": None, "shape": (B, C, h, w)})
            a0 += h * w
        ctx.sparse = spec["slots"] is not None
        if ctx.sparse:
            for e, slot in zip(ctx.entries, spec["slots"]):
                e["off"] = slot["offs"][spec["which"]]
                slot.setdefault("entries", []).append(e)
        ctx.nt, ctx.dtype, ctx.dev = len(tensors), dtype, dev
        spec["compact"] = (rows, idx, counts)  # (rows, (image, anchor) index, [n_fg per image..., rows written, total]) for tests / tools
        return item.reshape(())

    @staticmethod
    def backward(ctx, d):
        if d is None:
            return (None,) * (1 + ctx.nt)
        scale = d.detach().float().reshape(1).contiguous()
        if ctx.sparse:
            for e in ctx.entries:
                e["scale"] = scale
            return (None,) * (1 + ctx.nt)
        grads = []
        for e in ctx.entries:
            B, C, H, W = e["shape"]
            g = ops.nhwc_empty(B, C, H, W, ctx.dtype, ctx.dev).zero_()
            lib().distill_scatter(ops.code(ctx.dtype), e["rows"].data_ptr(), e["idx"].data_ptr(), e["nrows"].data_ptr(), scale.data_ptr(), e["cap"], C,
                                  g.data_ptr(), *ops.s3(g), e["a0"], H, W, ops.stream())
            grads.append(g)
        return (None, *grads)


class FgdmLossFn(torch.autograd.Function):
    """utils/loss.py:1299-1324 on the HIP kernel of csrc/fgdm_loss.hip.  apply(logits, depth_maps, cfg) -> loss (0-dim fp32);
    cfg = (num_bins, dmin, dmax, alpha, gamma, fg_weight, bg_weight).  The forward launch also writes d loss / d logits in the logits'
    dtype and layout (no softmax tensor is kept); the backward multiplies it by the incoming scalar on the device.  After a forward
    `FgdmLossFn.last_targets` holds the (B, h, w) int32 class of every cell (for tests and tools)."""

    last_targets = None

    @staticmethod
    def forward(ctx, logits, depth_maps, cfg):
        num_bins, dmin, dmax, alpha, gamma, fgw, bgw = cfg
        if not (torch.is_tensor(logits) and logits.dim() == 4 and torch.is_tensor(depth_maps) and depth_maps.dim() == 3):
            raise ValueError("ForegroundDepthMapLoss: depth_logits must be (B, num_bins + 1, h, w) and depth_maps (B, H, W)")
        if not logits.is_cuda:
            raise Y3DError("ForegroundDepthMapLoss runs on the HIP kernel of fgdm_loss.hip: the logits must live on a HIP device (no CPU fallback)")
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise Y3DError(f"ForegroundDepthMapLoss: logits must be float32 or bfloat16 (got {logits.dtype})")
        if not depth_maps.is_floating_point():
            raise ValueError(f"ForegroundDepthMapLoss: depth_maps must be a floating-point tensor (got {depth_maps.dtype})")
        B, C, h, w = logits.shape
        if C != num_bins + 1:
            raise ValueError(f"ForegroundDepthMapLoss: the logits have {C} channels, num_bins + 1 = {num_bins + 1} are needed")
        H, W = depth_maps.shape[1:]
        if depth_maps.shape[0] != B or (h, w) != (H // 16, W // 16) or h < 1 or w < 1:
            raise ValueError(f"ForegroundDepthMapLoss: logits of {B} x {h} x {w} cells do not match depth maps {tuple(depth_maps.shape)}: "
                             "the grid must be (H // 16, W // 16)")
        if depth_maps.device != logits.device:
            raise ValueError(f"ForegroundDepthMapLoss: the depth maps live on {depth_maps.device}, the logits on {logits.device}")
        z = logits.detach()
        dense = z.is_contiguous() or z.is_contiguous(memory_format=torch.channels_last)
        # a channel slice of a wider pixel-dense NHWC buffer (the depth classifier's 81 of 88 columns) is read where it lies
        sliced = not dense and ops.is_nhwc(z) and ops.px_dense(z) and z.data_ptr() % 16 == 0
        if not (dense or sliced):
            z, dense = z.contiguous(), True
        dm = depth_maps.detach()
        if dm.dtype not in (torch.float32, torch.float64):
            dm = dm.float()  # half and bfloat16 values are float32 values
        dm = dm.contiguous()
        dev = z.device
        L = lib()
        # the logits' strides (the kernel writes the gradient where it read the logit); a slice's gaps are never read
        grad = torch.empty_like(z) if dense else torch.empty_strided(z.shape, z.stride(), dtype=z.dtype, device=dev)
        part = torch.empty(L.fgdm_loss_blocks(B, h, w), dtype=torch.float32, device=dev)
        item = torch.empty(1, dtype=torch.float32, device=dev)
        tgt = torch.empty(B, h, w, dtype=torch.int32, device=dev)
        L.fgdm_loss(ops.code(z.dtype), z.data_ptr(), *z.stride(), int(dm.dtype == torch.float64), dm.data_ptr(), B, H, W, h, w, num_bins,
                    float(dmin), float(dmax), float(alpha), float(gamma), float(fgw), float(bgw), grad.data_ptr(), part.data_ptr(),
                    item.data_ptr(), tgt.data_ptr(), ops.stream())
        FgdmLossFn.last_targets = tgt
        ctx.grad = grad
        return item.reshape(())

    @staticmethod
    def backward(ctx, d):
        if d is None:
            return None, None, None
        g = ctx.grad
        scale = d.detach().float().reshape(1).contiguous()
        if g.is_contiguous() or g.is_contiguous(memory_format=torch.channels_last):
            out, n = torch.empty_like(g), g.numel()
        else:  # a slice's layout: every element from the first to the last, the gaps with them
            out = torch.empty_strided(g.shape, g.stride(), dtype=g.dtype, device=g.device)
            n = sum((s - 1) * st for s, st in zip(g.shape, g.stride())) + 1
        lib().fgdm_scale(ops.code(g.dtype), g.data_ptr(), scale.data_ptr(), out.data_ptr(), n, ops.stream())
        return out, None, None


class ForegroundDepthMapLoss:
    """utils/loss.py:1225-1324: focal classification of depth logits (B, num_bins + 1, H // 16, W // 16) against the LID bins of the
    foreground depth maps (B, H, W) (`batch["depth_map"]` of the KITTI builders under `load_depth_maps`), foreground cells weighted
    `fg_weight`, background cells `bg_weight`, mean over cells.  `model_or_args`: a model (its `.args`) or the args themselves;
    `min_depth_threshold` / `max_depth_threshold` are the bin range.  The logits are supplied by the caller: the DepthPredictor that
    makes them is modules.DepthPredictor (`v10Detect3d(fgdm_predictor=True)`), and DetectLoss3d adds this loss times `fgdm_loss_weight`
    as its 13th item under `fgdm_loss`."""

    def __init__(self, model_or_args, alpha=0.25, gamma=2.0, fg_weight=13, bg_weight=1, num_bins=80):
        args = getattr(model_or_args, "args", model_or_args)
        self.args = args
        self.num_bins = int(num_bins)
        if not 1 <= self.num_bins <= 255:
            raise ValueError(f"ForegroundDepthMapLoss: num_bins must be in 1..255 (got {num_bins})")
        self.alpha, self.gamma, self.fg_weight, self.bg_weight = float(alpha), float(gamma), float(fg_weight), float(bg_weight)
        if not (self.gamma == 0.0 or self.gamma >= 1.0):
            raise ValueError(f"ForegroundDepthMapLoss: gamma must be 0 or >= 1 (got {gamma})")
        self.dmin, self.dmax = float(args.min_depth_threshold), float(args.max_depth_threshold)
        if not self.dmax > self.dmin:
            raise ValueError("ForegroundDepthMapLoss: max_depth_threshold must exceed min_depth_threshold")

    def __call__(self, depth_logits, depth_maps):
        cfg = (self.num_bins, self.dmin, self.dmax, self.alpha, self.gamma, self.fg_weight, self.bg_weight)
        return FgdmLossFn.apply(depth_logits, depth_maps, cfg)

    forward = __call__


def loss_names(args):
    """models/yolov10_3D/train.py:33-39: names of the loss items DetectLoss3d returns, one-to-many set first"""
    om = ["box_om", "cls_om", "dep_om", "o3d_om", "s3d_om", "hd_om"]
    oo = ["box_oo", "cls_oo", "dep_oo", "o3d_oo", "s3d_oo", "hd_oo"]
    if getattr(args, "distillation", False):
        om, oo = om + ["dis_om"], oo + ["dis_oo"]
    names = om + oo
    if getattr(args, "fgdm_loss", False):
        names = names + ["fgdm"]  # models/yolov10_3D/train.py:41-42
    return names


def _loss3d_set(cfg, gt, n_used, calib, mean_sizes, lv, grad_ptrs, gsw, B, dtype, dev):
    """one head set (cfg: LossCfg3d) on the HIP kernels over the levels `lv`: assignment + six loss items + gradient rows written at
    grad_ptrs (pixel strides gsw) -> SetResult.  With cfg.item_w the launch is y3d_loss3d_weighted: the rows come out times the weight
    of their item, the items as ever, and `total` = sum(item_w * items); grad_ptrs None (a pass under no_grad): no rows are stored."""
    L = lib()
    nc, w = cfg.nc, cfg.weights
    dt, st = ops.code(dtype), ops.stream()
    n = gt.shape[1]
    c_grads, c_gsw = lv.rows(grad_ptrs, gsw)
    scratch, fg, gi, ts, scal = _assignment_buffers(L.tal3d_scratch_floats(B, n, lv.A, cfg.topk), "Loss3dFn", B, lv.A, nc, dev)
    L.tal3d_assign(dt, lv.nl, lv.maps, lv.psw, lv.H, lv.W, lv.st, B, nc, gt.data_ptr(), n, calib.data_ptr(), mean_sizes.data_ptr(), cfg.topk,
                   cfg.alpha, cfg.beta, cfg.gamma, int(cfg.mode), scratch.data_ptr(), fg.data_ptr(), gi.data_ptr(), ts.data_ptr(), scal.data_ptr(),
                   n_used.data_ptr() if n_used is not None else None, st)
    part, items = _item_buffers(B, lv.A, 6, dev)
    if cfg.item_w is None:
        L.loss3d(dt, lv.nl, lv.maps, lv.psw, c_grads, c_gsw, lv.H, lv.W, lv.st, B, nc, gt.data_ptr(), n, fg.data_ptr(), gi.data_ptr(), ts.data_ptr(),
                 scal.data_ptr(), w[0], w[1], w[2], w[3], w[4], w[5], 1.0, part.data_ptr(), items.data_ptr(), st)
        return SetResult(items, fg, gi, ts, scal)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    L.loss3d_weighted(dt, lv.nl, lv.maps, lv.psw, c_grads, c_gsw, lv.H, lv.W, lv.st, B, nc, gt.data_ptr(), n, fg.data_ptr(), gi.data_ptr(),
                      ts.data_ptr(), scal.data_ptr(), w[0], w[1], w[2], w[3], w[4], w[5], 1.0, part.data_ptr(), items.data_ptr(),
                      cfg.item_w.data_ptr(), total.data_ptr(), st)
    return SetResult(items, fg, gi, ts, scal, total)


class Loss3dFn(torch.autograd.Function):
    """One head set: task-aligned assignment (no grad) + the six 3D loss terms + d(sum of terms)/d(head maps), on the fused HIP
    kernels.  apply(cfg, gt(B,n,17), n_used, calib, mean_sizes, *maps) -> (sum_of_items, items[6], fg_mask, target_gt_idx, target_scores,
    scal), `SetResult.outputs`; cfg: LossCfg3d; n_used: device int32 from pad_targets (or None: walk all n rows).  With cfg.item_w
    (`set_item_weights`): the weighted entry, sum_of_items = sum(table * items), and no gradient rows when cfg.store_grads is off."""

    @staticmethod
    def forward(ctx, cfg, gt, n_used, calib, mean_sizes, *maps):
        dtype, dev = maps[0].dtype, maps[0].device
        _check_maps(maps, "Loss3dFn")
        B, no = maps[0].shape[:2]
        lv = Levels.of(maps, cfg.strides)
        grads = [ops.nhwc_empty(B, no, h, w, dtype, dev) for h, w in zip(lv.H, lv.W)] if cfg.store_grads else []
        r = _loss3d_set(cfg, gt.float().contiguous(), n_used, calib.float().contiguous(), mean_sizes.float().contiguous(), lv,
                        [g.data_ptr() for g in grads] if cfg.store_grads else None, [no] * lv.nl, B, dtype, dev)
        return _close_forward(ctx, grads, len(maps), r)

    @staticmethod
    def backward(ctx, d_total, *unused):
        return _scaled_rows(ctx, d_total, 5)


class DualLoss3dFn(torch.autograd.Function):
    """Both head sets of a step on the head's own (B, 2*no, H, W) maps ([one-to-one | one-to-many] channels, as
    v10Detect3d.forward_train_fused writes them): the gradient rows of both sets go into ONE NHWC tensor per level and the backward
    is one broadcast multiply per level.  With the two sets as separate autograd inputs (channel slices of that map) autograd
    zero-fills a full map per slice, copies, adds and re-lays the sum out: 7 elementwise launches per level instead of 1.
    apply(cfg_o2o, cfg_o2m, gt, n_used, calib, mean_sizes, *maps) -> the six outputs of Loss3dFn for the one-to-one set, then the six
    for the one-to-many set.  Each set takes its own cfg's item weights (`set_item_weights` gives both a table or neither); whether
    gradient rows are stored is cfg_o2o.store_grads for both"""

    @staticmethod
    def forward(ctx, cfg1, cfgm, gt, n_used, calib, mean_sizes, *maps):
        dtype, dev = maps[0].dtype, maps[0].device
        _check_maps(maps, "DualLoss3dFn")
        B, no2 = maps[0].shape[:2]
        no, esz, store = no2 // 2, maps[0].element_size(), cfg1.store_grads
        grads = [ops.nhwc_empty(B, no2, m.shape[2], m.shape[3], dtype, dev) for m in maps] if store else []
        gt, calib, mean_sizes = gt.float().contiguous(), calib.float().contiguous(), mean_sizes.float().contiguous()
        r1, rm = [_loss3d_set(cfg, gt, n_used, calib, mean_sizes, Levels.of(maps, cfg.strides, off), [g.data_ptr() + off for g in grads] if store else None,
                              [no2] * len(maps), B, dtype, dev) for cfg, off in ((cfg1, 0), (cfgm, no * esz))]
        ctx.no = no
        return _close_forward(ctx, grads, len(maps), r1, rm)

    @staticmethod
    def backward(ctx, d1, _i1, _fg1, _gi1, _ts1, _scal1, dm, *unused):
        grads = ctx.saved_tensors
        if (d1 is None and dm is None) or not grads:
            return (None,) * (6 + ctx.nmaps)
        no = ctx.no
        z = torch.zeros((), dtype=torch.float32, device=grads[0].device)
        scale = torch.cat(((d1 if d1 is not None else z).float().reshape(1).expand(no), (dm if dm is not None else z).float().reshape(1).expand(no)))
        scale = scale.to(grads[0].dtype).view(1, 2 * no, 1, 1)
        return (None, None, None, None, None, None, *[g * scale for g in grads])


class DDDetectionLoss:
    """utils/loss.py:774-963"""

    def __init__(self, model, tal_topk=10):
        h = model.args
        m = model.model[-1]
        self.hyp = h
        self.stride = [float(s) for s in m.stride]
        self.nc, self.no = m.nc, m.no
        # assigner modes of cfg/default.yaml:116-119 (utils/tal.py:465-497), as the mode bits of y3d_tal3d_assign
        if not (h.tal_2d or h.tal_3d):
            raise RuntimeError("Either 2D or 3D assignment or both has to be selected!")  # the reference's message, tal.py:484
        if h.kps_dist_metric not in ("l1", "l2"):
            raise ValueError(f"kps_dist_metric {h.kps_dist_metric!r}: 'l1' or 'l2' (utils/tal.py:465-470)")
        self.mode = (1 if h.tal_2d else 0) | (2 if h.tal_3d else 0) | (4 if h.kps_dist_metric == "l2" else 0) | (8 if h.constrain_anchors else 0)
        self.topk = tal_topk
        # feature distillation (loss.py:792-793, 1146-1150): the loss runs here, the teacher map is supplied (batch["teacher_emb"] / set_teacher)
        self.distillation = bool(getattr(h, "distillation", False))
        m.distill = self.distillation  # on: the fused head opens its sparse gradient path (modules.v10Detect3d.forward_train_fused)
        if self.distillation:
            if h.distillation_loss not in CRITERIA:
                raise RuntimeError(f"Unknown criterion function: {h.distillation_loss}")  # the reference's message, loss.py:1185
            self.dis = (float(h.distillation_temp), float(h.distillation_weight), CRITERIA[h.distillation_loss], bool(h.distillation_no_mixup))
        self.item_w = None

    def set_item_weights(self, table):
        """`table`: 6 device floats (in the order of the loss items: box, cls, dep, o3d, s3d, hd) that weight this head set's items,
        read by the loss kernel at every call - whoever owns the tensor may change its contents between calls (train.HtlWeights) - or
        None: the calls of before.  With a table the loss is sum(table * items), NOT times the batch size (engine/trainer.py:398-400)."""
        if table is not None:
            if self.distillation:
                raise NotImplementedError("item weights (htl) with distillation: the reference multiplies 12 weights into 14 items")
            if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.numel() == 6 and table.is_contiguous()):
                raise Y3DError("set_item_weights: 6 contiguous fp32 values on a HIP device (no host path)")
        self.item_w = table
    GT_KEYS = ("batch_idx", "cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res")

    def targets(self, batch, B, H, W, dev):
        """padded ground truth of one step (loss.py:848-856): (gt (B, cap, 17), n_used) or None when the batch has no box at all"""
        if batch["batch_idx"].shape[0] == 0:  # (checked first: a `view(0, -1)` of an empty tensor is ambiguous and raises)
            return None
        rows = torch.cat([batch[k].to(dev).float().view(batch[k].shape[0], -1) for k in self.GT_KEYS], 1)
        return pad_targets(rows, B, 17, (W * self.stride[0], H * self.stride[0]))

    def __call__(self, preds, batch, embeddings=None, targets=None, teacher=None):
        """`targets`: the result of `self.targets(...)` when the caller shares it between the two head sets of a step"""
        feats, dev, B, img_wh, targets, maps = _head_inputs(self, "3D", preds, batch, targets)
        if targets is None:
            loss = torch.zeros(7 if self.distillation else 6, device=dev)
            return loss.sum() * B, loss  # reference: graph-less zeros (loss.py:873-877); callers skip the step
        g, n_used = targets
        r = SetResult.of(Loss3dFn.apply(self.cfg(len(feats)), g, n_used, batch["calib"].to(dev), batch["mean_sizes"].to(dev), *maps))
        self._assignment = r[1:4]
        if self.item_w is not None:
            return r.total, r.items
        if not self.distillation:
            return r.total * B, r.items
        if embeddings is None:
            raise Y3DError("distillation: the head's embeddings (preds['o2o_embs'] / preds['o2m_embs']) must be passed as `embeddings`")
        dis = self.distill(batch, g, embeddings, r.fg, r.gt_idx, r.scal, img_wh, teacher=teacher)
        return (r.total + dis) * B, torch.cat((r.items, dis.detach().reshape(1)))

    def distill(self, batch, gt, embeddings, fg, gt_idx, scal, img_wh, teacher=None, slots=None, which=0, ties=()):
        """the distillation item of this head set (loss.py:893-898) -> 0-dim tensor tied into the autograd graph (DistillFn)"""
        embs = list(embeddings)
        dev = embs[0].device
        if teacher is None:
            teacher = teacher_map(batch, like=embs[0])
        else:
            check_teacher(teacher, embs[0])
        T, weight, crit, no_mixup = self.dis
        mixed = None
        if no_mixup:
            if "mixed" not in batch:
                raise Y3DError('distillation_no_mixup: the batch needs its per-image "mixed" flags')
            mixed = batch["mixed"].to(dev).to(torch.uint8).contiguous()
        if "img" in batch and torch.is_tensor(batch["img"]):
            img_wh = (batch["img"].shape[3], batch["img"].shape[2])  # loss.py:1165
        B, n = gt.shape[:2]
        A = sum(e.shape[2] * e.shape[3] for e in embs)
        spec = dict(teacher=teacher, gt=gt.float().contiguous(), fg=fg, gi=gt_idx, scal=scal, mixed=mixed, img_wh=img_wh, T=T, weight=weight, crit=crit,
                    no_mixup=no_mixup, cap=B * min(A, n * self.topk), slots=slots, which=which)
        if slots is not None:
            spec["embs"] = [e.detach() for e in embs]
            return DistillFn.apply(spec, *ties)
        dt = ops.compute_dtype()
        embs = [e if (e.dtype == dt and ops.is_nhwc(e) and ops.px_dense(e)) else ops.to_nhwc(e, dt, dense=True) for e in embs]
        spec["embs"] = [e.detach() for e in embs]
        return DistillFn.apply(spec, *embs)

    def cfg(self, nl):
        h = self.hyp
        # with a table, whether gradient rows are wanted is read HERE: inside an autograd Function's forward grad mode is always off
        return LossCfg3d(self.stride[:nl], self.nc, self.topk, float(h.tal_alpha), float(h.tal_beta), float(h.tal_gamma),
                         (float(h.loss2d), float(h.cls), float(h.depth), float(h.offset3d), float(h.size3d), float(h.heading)), self.mode,
                         self.item_w, self.item_w is None or torch.is_grad_enabled())

    @property
    def last_assignment(self):
        """(fg_mask bool, target_gt_idx int64, target_scores) of the last call, in the reference's dtypes (converted on access)"""
        fg, gi, ts = self._assignment
        return fg.bool(), gi.long(), ts


class DetectLoss3d:
    """utils/loss.py:740-771"""

    def __init__(self, model):
        self.one2many = DDDetectionLoss(model, tal_topk=model.args.tal_topk)
        self.one2one = DDDetectionLoss(model, tal_topk=1)
        # auxiliary depth supervision (loss.py:745-748, 757-767): ForegroundDepthMapLoss over the head's DepthPredictor logits
        args = model.args
        if getattr(args, "fgdm_supervision", False):
            raise NotImplementedError("fgdm_supervision: SupervisionLoss.forward_fgdm needs the DINOv2 teacher, which is not part of this "
                                      "package; set fgdm_supervision: False (fgdm_loss alone trains the depth predictor)")
        self.fgdm = None
        if getattr(args, "fgdm_loss", False):
            if not getattr(model.model[-1], "fgdm_pred", False):
                raise Y3DError("fgdm_loss: the head has no depth predictor; build the model with `fgdm_predictor: True` in the head's yaml "
                               "arguments (v10Detect3d(fgdm_predictor=True)) or set fgdm_loss: False")
            if not hasattr(args, "min_depth_threshold"):
                args.min_depth_threshold, args.max_depth_threshold = 1, 120  # cfg/default.yaml:123-124
            self.fgdm = ForegroundDepthMapLoss(model)
            self.fgdm_weight = float(getattr(args, "fgdm_loss_weight", 2))

    def _depth_pair(self, preds, batch):
        """(depth logits, depth maps) of a step under fgdm_loss, checked before any launch"""
        if "depth_map" not in batch:
            raise Y3DError('fgdm_loss: the batch has no "depth_map"; build it with load_depth_maps=True in the data args (kitti.data_args) '
                           "and, for a resident split, DeviceSplit(..., load_depth_maps=True)")
        dm = preds.get("depth_maps")
        if not isinstance(dm, (tuple, list)):
            raise Y3DError("fgdm_loss: the head returned no depth logits; build it with fgdm_predictor=True")
        return dm[0], batch["depth_map"].to(dm[0].device)

    def __call__(self, preds, batch):
        """loss.py:750-771: the two head sets, and under fgdm_loss the depth predictor's loss times fgdm_loss_weight - NOT times the batch
        size, unlike the two head-set totals - appended as the last item"""
        if self.fgdm is None:
            return self._head_sets(preds, batch)
        pair = self._depth_pair(preds, batch) if preds.get("one2many", None) else None
        total, items = self._head_sets(preds, batch)
        if pair is None:
            return total, items
        f = self.fgdm(*pair) * self.fgdm_weight
        return total + f, torch.cat((items, f.detach().reshape(1)))

    def set_item_weights(self, table):
        """`table`: 12 device floats, the one-to-many set's six first (`loss_names`), or None; see DDDetectionLoss.set_item_weights"""
        if table is not None and self.fgdm is not None:
            raise NotImplementedError("item weights (htl) with fgdm_loss: 12 weights for 13 items")
        if table is not None and not (torch.is_tensor(table) and table.numel() == 12 and table.dim() == 1):
            raise Y3DError("set_item_weights: a 1-D tensor of 12 values")
        self.one2many.set_item_weights(None if table is None else table[0:6])
        self.one2one.set_item_weights(None if table is None else table[6:12])
    @staticmethod
    def _shared_maps(maps, o2o, o2m, no):
        """`maps`: the head's own (B, 2*no, H, W) tensors (preds["_y3d_maps"], written by v10Detect3d.forward_train_fused), accepted
        only when the two head sets really are their channel halves [one-to-one | one-to-many]; else None"""
        if not maps or len(maps) != len(o2o) or len(o2o) != len(o2m):
            return None
        for base, a, b in zip(maps, o2o, o2m):
            if (base.dim() != 4 or base.shape[1] != 2 * no or a.shape[1] != no or b.shape[1] != no or base.dtype != ops.compute_dtype()
                    or not ops.px_dense(base) or a.stride() != base.stride() or b.stride() != base.stride()
                    or a.data_ptr() != base.data_ptr() or b.data_ptr() != base.data_ptr() + no * base.element_size()):
                return None
        return list(maps)

    @staticmethod
    def _z1_slots(slots, e1, em):
        """`slots`: preds["_y3d_distill"] of the fused head, accepted only when the embeddings really are the channel slices of z1 the
        slots describe (then their gradient goes in as compact rows, ops.InjectRowsFn); else None: plain autograd"""
        if not slots or len(slots) != len(e1) or len(e1) != len(em):
            return None
        for s, a, b in zip(slots, e1, em):
            esz = a.element_size()
            if (a.dtype != ops.compute_dtype() or a.data_ptr() != s["ptr"] + s["offs"][0] * esz or b.data_ptr() != s["ptr"] + s["offs"][1] * esz
                    or a.shape[1] != s["C"][0] or b.shape[1] != s["C"][1] or not (ops.is_nhwc(a) and ops.px_dense(a) and ops.px_dense(b))):
                return None
        return slots

    def _head_sets(self, preds, batch):
        o2o = preds["one2one"][1] if isinstance(preds["one2one"], tuple) else preds["one2one"]
        dev = o2o[0].device
        B, (H, W) = o2o[0].shape[0], o2o[0].shape[2:]
        tg = self.one2one.targets(batch, B, H, W, dev) if o2o[0].is_cuda else None  # padded once per step
        kw = {"targets": tg} if tg is not None else {}
        o2m = preds.get("one2many", None)
        if self.one2one.distillation and tg is not None:  # one teacher map per step, shared by both head sets (the reference runs its teacher once per set, loss.py:1159-1160)
            kw["teacher"] = teacher_map(batch, like=preds["o2o_embs"][0])
        out = self._dual(preds, batch, o2o, o2m[1] if isinstance(o2m, tuple) else o2m, tg, kw.get("teacher")) if o2m and tg is not None else None
        return out if out is not None else self._two_calls(preds, batch, kw)

    def _dual(self, preds, batch, o2o, o2m, tg, teacher):
        """both head sets in one DualLoss3dFn call on the head's own (B, 2*no, H, W) maps (teacher: the step's teacher map under
        distillation, else None) -> (loss, items), or None when `_shared_maps` refuses"""
        c1, cm = self.one2one, self.one2many
        bases = self._shared_maps(preds.get("_y3d_maps"), o2o, o2m, c1.no)
        if bases is None:
            return None
        dev, B, (H, W) = o2o[0].device, o2o[0].shape[0], o2o[0].shape[2:]
        g, n_used = tg
        nl = len(bases)
        out = DualLoss3dFn.apply(c1.cfg(nl), cm.cfg(nl), g, n_used, batch["calib"].to(dev), batch["mean_sizes"].to(dev), *bases)
        r1, rm = SetResult.of(out[:6]), SetResult.of(out[6:])
        c1._assignment, cm._assignment = r1[1:4], rm[1:4]
        items = (rm.items, r1.items)
        if c1.item_w is not None:
            loss = rm.total + r1.total
        elif teacher is None:
            loss = rm.total * B + r1.total * B
        else:
            e1, em = preds["o2o_embs"], preds["o2m_embs"]
            slots = self._z1_slots(preds.get("_y3d_distill"), e1, em)
            ties = tuple(bases) if slots is not None else ()
            wh = (W * c1.stride[0], H * c1.stride[0])
            d1 = c1.distill(batch, g, e1, r1.fg, r1.gt_idx, r1.scal, wh, teacher=teacher, slots=slots, which=0, ties=ties)
            dm = cm.distill(batch, g, em, rm.fg, rm.gt_idx, rm.scal, wh, teacher=teacher, slots=slots, which=1, ties=ties)
            loss = (rm.total + dm) * B + (r1.total + d1) * B
            items = (rm.items, dm.detach().reshape(1), r1.items, d1.detach().reshape(1))
        return loss, torch.cat(items)

    def _two_calls(self, preds, batch, kw):
        """the head sets through their own criteria, one Loss3dFn call each (separate maps, or a batch without boxes)"""
        l1, i1 = self.one2one(preds["one2one"], batch, embeddings=preds.get("o2o_embs"), **kw)
        if not preds.get("one2many", None):
            return torch.zeros(1), i1
        lm, im = self.one2many(preds["one2many"], batch, embeddings=preds.get("o2m_embs"), **kw)
        return lm + l1, torch.cat((im, i1))


class Loss2dFn(torch.autograd.Function):
    """2D head set: assignment + (box, cls, dfl) + gradient wrt the head maps on the fused HIP kernels of tal_loss2d.hip.
    apply(cfg, gt(B,n,5), n_used, *maps) -> (sum_of_items, items[3], fg_mask, target_gt_idx, target_scores, scal), `SetResult.outputs`;
    cfg: LossCfg2d"""

    @staticmethod
    def forward(ctx, cfg, gt, n_used, *maps):
        L = lib()
        nc, topk, w = cfg.nc, cfg.topk, cfg.weights
        dtype, dev = maps[0].dtype, maps[0].device
        dt, st = ops.code(dtype), ops.stream()
        _check_maps(maps, "Loss2dFn")
        B, no = maps[0].shape[:2]
        lv = Levels.of(maps, cfg.strides)
        n = gt.shape[1]
        gt = gt.float().contiguous()
        grads = [ops.nhwc_empty(B, no, h, w_, dtype, dev) for h, w_ in zip(lv.H, lv.W)]
        c_grads, c_gsw = lv.rows([g.data_ptr() for g in grads], [no] * lv.nl)
        crowded = n > TARGET_CAP  # more rows than the dense assigner takes (`max_boxes`): the route without (B, n, A) planes
        nsc = L.tal2d_scratch_floats(B, n, lv.A, topk) if crowded else L.tal3d_scratch_floats(B, n, lv.A, topk)
        scratch, fg, gi, ts, scal = _assignment_buffers(nsc, "Loss2dFn", B, lv.A, nc, dev)
        assign = L.tal2d_assign_crowded if crowded else L.tal2d_assign
        assign(dt, lv.nl, lv.maps, lv.psw, lv.H, lv.W, lv.st, B, nc, gt.data_ptr(), n, topk, cfg.alpha, cfg.beta, scratch.data_ptr(), fg.data_ptr(),
               gi.data_ptr(), ts.data_ptr(), scal.data_ptr(), n_used.data_ptr() if n_used is not None else None, st)
        part, items = _item_buffers(B, lv.A, 3, dev)
        L.loss2d(dt, lv.nl, lv.maps, lv.psw, c_grads, c_gsw, lv.H, lv.W, lv.st, B, nc, gt.data_ptr(), n, fg.data_ptr(), gi.data_ptr(), ts.data_ptr(),
                 scal.data_ptr(), w[0], w[1], w[2], 1.0, part.data_ptr(), items.data_ptr(), st)
        return _close_forward(ctx, grads, len(maps), SetResult(items, fg, gi, ts, scal))

    @staticmethod
    def backward(ctx, d_total, *unused):
        return _scaled_rows(ctx, d_total, 3)


class v8DetectionLoss:
    """utils/loss.py:157-257 (+BboxLoss :73-113) on the HIP kernels of tal_loss2d.hip.
    max_boxes (or `model.args.max_boxes`): ground-truth rows per image.  None: 64 and the dense assigner; a multiple of 64 in 128..512
    (crowded 2D data, mosaics): the targets are padded to that many rows and the assignment takes the crowded route."""

    def __init__(self, model, tal_topk=10, max_boxes=None):
        m = model.model[-1]
        self.hyp = model.args
        self.max_boxes = check_max_boxes(max_boxes if max_boxes is not None else getattr(model.args, "max_boxes", None))
        self.stride = [float(s) for s in m.stride]
        self.nc, self.no, self.reg_max = m.nc, m.no, m.reg_max
        if self.reg_max != 16:
            raise NotImplementedError("the DFL kernels are built for reg_max = 16")
        self.topk = tal_topk

    def targets(self, batch, B, H, W, dev):
        """padded ground truth (loss.py:223-226): (gt (B, cap, 5), n_used) or None when the batch has no box at all"""
        rows = torch.cat((batch["batch_idx"].view(-1, 1), batch["cls"].view(-1, 1), batch["bboxes"]), 1).to(dev).float()
        if rows.shape[0] == 0:
            return None
        return pad_targets(rows, B, 5, (W * self.stride[0], H * self.stride[0]), cap=self.max_boxes or TARGET_CAP)

    def __call__(self, preds, batch, targets=None):
        feats, dev, B, _, targets, maps = _head_inputs(self, "2D", preds, batch, targets)
        if targets is None:
            # no boxes at all: background-only classification loss (loss.py:244), dense BCE against zero targets
            sc = _flatten_maps(feats)[..., self.reg_max * 4:]
            l_cls = F.binary_cross_entropy_with_logits(sc, torch.zeros_like(sc), reduction="none").sum() * self.hyp.cls
            loss = torch.stack((torch.zeros((), device=dev), l_cls, torch.zeros((), device=dev)))
            return loss.sum() * B, loss.detach()
        g, n_used = targets
        r = SetResult.of(Loss2dFn.apply(self.cfg(len(feats)), g, n_used, *maps))
        self.last_assignment = (r.fg.bool(), r.gt_idx.long(), r.target_scores)
        return r.total * B, r.items

    def cfg(self, nl):
        h = self.hyp
        return LossCfg2d(self.stride[:nl], self.nc, self.topk, 0.5, 6.0, (float(h.box), float(h.cls), float(h.dfl)))


class v10DetectLoss:
    """utils/loss.py:727-737"""

    def __init__(self, model, max_boxes=None):
        self.one2many = v8DetectionLoss(model, tal_topk=10, max_boxes=max_boxes)
        self.one2one = v8DetectionLoss(model, tal_topk=1, max_boxes=max_boxes)
        self.max_boxes = self.one2many.max_boxes

    def __call__(self, preds, batch):
        f0 = preds["one2many"][1] if isinstance(preds["one2many"], tuple) else preds["one2many"]
        tg = self.one2many.targets(batch, f0[0].shape[0], f0[0].shape[2], f0[0].shape[3], f0[0].device)  # padded once per step
        kw = {"targets": tg} if tg is not None else {}
        lm, im = self.one2many(preds["one2many"], batch, **kw)
        l1, i1 = self.one2one(preds["one2one"], batch, **kw)
        return lm + l1, torch.cat((im, i1))


def _postprocess(preds, max_det, nc, boxes_first):
    """preds (B, A, C) as the reference passes it (a permuted view of the head's (B, C, A) output): one HIP launch"""
    if not preds.is_cuda:
        raise Y3DError("v10 postprocess runs on the HIP kernel of post.hip: predictions must live on a HIP device")
    B, A, C = preds.shape
    y = preds.permute(0, 2, 1)
    if not (y.is_contiguous() and y.dtype == torch.float32):
        y = y.float().contiguous()
    nr = C - nc
    reg = torch.empty(B, max_det, nr, dtype=torch.float32, device=preds.device)
    scores = torch.empty(B, max_det, dtype=torch.float32, device=preds.device)
    labels = torch.empty(B, max_det, dtype=torch.int64, device=preds.device)
    ns = lib().v10_postprocess_scratch_floats(B, A, nc, max_det)  # hi-res maps: the per-image score row lives in HBM instead of LDS
    scratch = torch.empty(ns, dtype=torch.float32, device=preds.device) if ns else None
    lib().v10_postprocess(y.data_ptr(), B, C, A, nc, max_det, int(boxes_first), reg.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                          scratch.data_ptr() if ns else None, ops.stream())
    return reg, scores, labels


def v10_3Dpostprocess(preds, max_det, nc=3):
    """utils/ops.py:867-880: top-k over anchors of the max-class score, then over the k*nc scores -> (reg, scores, labels)"""
    assert preds.shape[-1] == nc + 35
    return _postprocess(preds, max_det, nc, False)


def v10postprocess(preds, max_det, nc=80):
    """utils/ops.py:852-865"""
    assert 4 + nc == preds.shape[-1]
    return _postprocess(preds, max_det, nc, True)
