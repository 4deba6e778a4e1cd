"""Mints tests/golden/ops_call_trace.json.gz: every call the Python glue makes into the library (name + arguments) over a set of small
cases, so that a change to `ops.py` that is meant to keep the launch sequence and every launch argument can be checked call for call.

    python tools/make_golden_ops_trace.py             # needs the built library and a HIP device; writes the fixture
    python tools/make_golden_ops_trace.py --check     # replays the cases and compares them with the fixture instead

The `yolov10_3d_amd._lib._lib` singleton (what every `lib()` of the package returns) is replaced by a proxy that records a call and forwards
it to the real library.  Recorded per argument: ints and floats as they are; a pointer (`c_void_p` in the parsed header) as 0 / 1 for
null / non-null; a ctypes int or float array as its values; a ctypes pointer array as its length.  The pack and quantiser registries are
replaced by empty ones for the duration of a case (their multi-tensor launches cover every weight the process has registered), and a case
runs once unrecorded first, so that nothing in the trace depends on what the process did before.  Regenerate the fixture ONLY with a
change that is meant to move a launch, and say so there.

Cases (`CASES`): the tiny 3D model of `__graft_entry__.smoke()` (training forward + backward at 64x64, eval forward at 256x256: the
smallest image whose stride-32 map holds the head's 50 candidates) in bf16 and f32, bf16 with each of PACK_CACHE / STEM_FUSED /
PROJ_BN_MFMA / DW_EVAL_FUSED / PLACEMENT off, two steps around a `bump_weight_epoch()`, the eval forward of the model folded the
reference's way; the stem on uint8 images; the 128-wide head of tests/test_hip_fp8.py under the three fp8 switches and with
PROJ_BN_MFMA off; the 2D `v10Detect` head with a wide and a narrow projection; eval Bottlenecks with a shortcut on both residual arms;
the stacking layouts of `modules.v10Detect3d` that the models above do not have (`head3d_layout`: cls wider than the regression
branches with every / some / no part on the fused BatchNorm projections, the uniform layout unfused at 64 channels, no second-layer
stack, the distillation node), each in training and in eval; the loss glue (`loss/...`) through the public criterion classes on the
smallest cases of the loss tests: DDDetectionLoss on separate maps, DetectLoss3d on shared maps (nc = 2: an odd element offset), the
same with an item-weight table (with grad, under no_grad, the table taken away again), with distillation through both ways back into
the head, v10DetectLoss on the dense and on the crowded assigner, ForegroundDepthMapLoss.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, "tests", "golden", "ops_call_trace.json.gz")
DEV = "cuda"


# ---- the recording proxy -----------------------------------------------------------------------------------------------------------
def _encode(v, t):
    if t is ctypes.c_void_p:
        if isinstance(v, ctypes.Array):
            return ["ptrs", len(v)] if v._type_ is ctypes.c_void_p else ["vals", list(v)]
        return 1 if v else 0
    return float(v) if t in (ctypes.c_float, ctypes.c_double) else int(v)


class Recorder:
    """stands in for the `_Lib` singleton: `sink` receives [name, [encoded arguments]] per call of a function declared in y3d.h"""

    def __init__(self, real, sink):
        self.__dict__.update(_real=real, _sink=sink)

    def __getattr__(self, name):
        real, sink = self.__dict__["_real"], self.__dict__["_sink"]
        fn = getattr(real, name)
        proto = real.protos.get("y3d_" + name)
        if proto is None:
            return fn

        def call(*a):
            sink.append([name, [_encode(v, t) for v, t in zip(a, proto[1])]])
            return fn(*a)

        return call


@contextlib.contextmanager
def recording(sink):
    from yolov10_3d_amd import _lib
    _lib.lib()
    prev = _lib._lib
    _lib._lib = Recorder(prev, sink)
    try:
        yield
    finally:
        _lib._lib = prev


@contextlib.contextmanager
def fresh_registries():
    from yolov10_3d_amd import ops
    prev = ops.PACK_FWD, ops.PACK_DGRAD, ops.QUANT
    ops.PACK_FWD, ops.PACK_DGRAD, ops.QUANT = ops._PackRegistry(0), ops._PackRegistry(1), ops._QuantRegistry()
    try:
        yield
    finally:
        ops.PACK_FWD, ops.PACK_DGRAD, ops.QUANT = prev


@contextlib.contextmanager
def flag_off(name):
    from yolov10_3d_amd import ops
    prev = getattr(ops, name) if name else None
    if name:
        setattr(ops, name, False)
    try:
        yield
    finally:
        if name:
            setattr(ops, name, prev)


@contextlib.contextmanager
def compute_dtype(dt):
    import torch
    import yolov10_3d_amd as y3d
    y3d.set_compute_dtype(dt)
    try:
        yield
    finally:
        y3d.set_compute_dtype(torch.bfloat16)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def _tiny_model():
    import torch
    import yolov10_3d_amd as y3d
    cfg = y3d.yaml_model_load("yolov10s_3D.yaml")
    cfg.update(scales={"n": [0.33, 0.125, 1024]}, scale="n",
               channels={k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")})
    torch.manual_seed(0)
    return y3d.YOLOv10_3DDetectionModel(cfg).to(DEV)


def _tiny_batch():
    import torch
    g = torch.Generator().manual_seed(1)
    b = {
        "img": torch.rand(2, 3, 64, 64, generator=g),
        "batch_idx": torch.tensor([0.0, 0.0, 1.0]), "cls": torch.tensor([[0.0], [2.0], [1.0]]),
        "bboxes": torch.tensor([[0.4, 0.5, 0.3, 0.25], [0.6, 0.4, 0.2, 0.3], [0.5, 0.5, 0.35, 0.3]]),
        "size_3d": torch.zeros(3, 3), "depth": torch.tensor([12.0, 30.0, 20.0]), "heading_bin": torch.tensor([1.0, 5.0, 9.0]),
        "heading_res": torch.tensor([0.1, -0.1, 0.0]), "calib": torch.tensor([[32.0, 32.0, 700.0, 700.0, 0.06, -0.002]]).repeat(2, 1),
        "mean_sizes": torch.tensor([[1.76, 0.66, 0.84], [1.53, 1.63, 3.88], [1.74, 0.60, 1.76]]),
    }
    b["center_2d"] = b["bboxes"][:, :2] * 64
    b["size_2d"] = b["bboxes"][:, 2:] * 64
    b["center_3d"] = b["center_2d"] + 1.0
    return {k: v.to(DEV) for k, v in b.items()}


def _eval_image():
    import torch
    return torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(2)).to(DEV)


def _reference_fuse(model):
    """what the reference's BaseModel.fuse() does to every Conv: a new nn.Conv2d with folded weight + bias, no `.bn`, `forward_fuse`"""
    import torch
    import yolov10_3d_amd as y3d
    from yolov10_3d_amd import modules as M
    for m in model.modules():
        if isinstance(m, M.Conv) and hasattr(m, "bn"):
            w, b = y3d.tasks.fuse_conv_and_bn(m.conv.weight.detach(), m.bn.weight.detach(), m.bn.bias.detach(), m.bn.running_mean, m.bn.running_var, m.bn.eps)
            c = m.conv
            f = torch.nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, groups=c.groups, bias=True).requires_grad_(False).to(w.device)
            f.weight.copy_(w)
            f.bias.copy_(b)
            m.conv = f
            delattr(m, "bn")
            m.forward = m.forward_fuse
    return model


def tiny(dtype="bf16", off=None, steps=1, fuse=False):
    import torch
    from yolov10_3d_amd import ops
    with compute_dtype(torch.bfloat16 if dtype == "bf16" else torch.float32), flag_off(off):
        model, batch = _tiny_model().train(), _tiny_batch()
        for i in range(steps):
            if i:
                ops.bump_weight_epoch()  # what the fused optimizer does after writing the weights: the registries refresh every pack
                model.zero_grad(set_to_none=True)
            loss, _ = model(batch)
            loss.backward()
        model.eval()
        with torch.no_grad():
            if fuse:
                model = _reference_fuse(copy.deepcopy(model))
            model(_eval_image())
    torch.cuda.synchronize()


def stem_u8(off=None):
    """the stem Conv on the dataset's bytes (NCHW and channels-last), training forward + backward and eval"""
    import torch
    from yolov10_3d_amd import modules as M
    torch.manual_seed(1)
    with flag_off(off):
        m = M.Conv(3, 16, 3, 2).to(DEV)
        img = torch.randint(0, 256, (2, 3, 32, 48), dtype=torch.uint8, device=DEV)
        for x in (img, img.contiguous(memory_format=torch.channels_last)):
            m.train()(x).float().sum().backward()
            with torch.no_grad():
                m.eval()(x)
    torch.cuda.synchronize()


def head3d(quant=None, conv=False, dgrad=False, off=None, eval_too=False):
    """the 128-wide two-level head of tests/test_hip_fp8.py: training forward + backward (and the eval forward) under the fp8 switches"""
    import torch
    import yolov10_3d_amd as y3d
    from test_hip_fp8 import _head_case
    hd, xs = _head_case(DEV)
    y3d.set_weight_quant(quant)
    try:
        with flag_off(off):
            y3d.set_fp8_conv(conv)
            y3d.set_fp8_dgrad(dgrad)
            m = hd.to(DEV).train()
            xin = [x.to(DEV).requires_grad_(True) for x in xs]
            out = m(xin)
            sum(t.float().sum() for t in out["one2many"] + out["one2one"]).backward()
            if eval_too:
                with torch.no_grad():
                    m.eval()([x.detach() for x in xin])
    finally:
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)
    torch.cuda.synchronize()


HEAD_BRANCHES = ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")


def head3d_layout(cls_c, reg_c, fuse=True, distill=False, eval_too=True, **other):
    """one stacking layout of `modules.v10Detect3d`: the two-level head of tests/test_hip_distill.py (`_head`) with `cls` `cls_c` wide and
    the seven regression branches `reg_c` wide (`other`: single branches at another width), B = 2 on a 12x12 and an 8x8 map (64 cells:
    the smallest map that holds the eval head's 50 candidates); training forward + backward, then the eval forward.  `distill`: the
    InjectRowsFn node sits behind z1, and its backward is handed one EMPTY compact-row entry per head set and level (no row is written),
    so that the trace holds the `distill_scatter` launches with the widths and level sizes the slots name."""
    import torch
    from yolov10_3d_amd import modules as M
    torch.manual_seed(7)
    chan = {k + "_c": other.get(k, cls_c if k == "cls" else reg_c) for k in HEAD_BRANCHES}
    hd = M.v10Detect3d(3, (32, 64), False, chan, False, False, False, False, 2, False, False, 3, 3)
    hd.stride = torch.tensor([8.0, 16.0])
    hd.bias_init()
    hd = hd.to(DEV).train()
    with torch.no_grad():
        for p in hd.parameters():
            p.add_(0.02 * torch.randn_like(p))
    hd.fuse_bn_proj, hd.distill = fuse, distill
    g = torch.Generator().manual_seed(8)
    xs = [torch.randn(2, 32, 12, 12, generator=g).to(DEV), torch.randn(2, 64, 8, 8, generator=g).to(DEV)]
    out = hd([x.requires_grad_(True) for x in xs])
    a0 = 0
    for slot, z in zip(out.get("_y3d_distill", ()), out["o2o_embs"]):
        for which in (0, 1):
            C = slot["C"][which]
            slot.setdefault("entries", []).append({
                "rows": torch.zeros(4, C, dtype=z.dtype, device=DEV), "idx": torch.zeros(4, 2, dtype=torch.int32, device=DEV),
                "nrows": torch.zeros(1, dtype=torch.int32, device=DEV), "scale": torch.ones(1, device=DEV), "cap": 4, "C": C,
                "off": slot["offs"][which], "a0": a0})
        a0 += z.shape[2] * z.shape[3]
    sum(t.float().sum() for t in out["one2many"] + out["one2one"]).backward()
    if eval_too:
        with torch.no_grad():
            hd.eval()([x.detach() for x in xs])
    torch.cuda.synchronize()


def head3d_wide_cls_fused():
    """(128, 64): the parts arm with every part (cls | 14 regression branches | cls) on FusedConvBNProjFn; the 16 projected slices are
    lined up by one `cat`.  Eval: the per-branch patch path (only the uniform layout has the stacked one)."""
    head3d_layout(128, 64)


def head3d_wide_cls_mixed():
    """(128, 32): the parts arm with the two cls parts on FusedConvBNProjFn and the regression part unfused (32 is no multiple of 64): its
    14 features are projected one by one and the 16 outputs lined up - the mixed tail."""
    head3d_layout(128, 32)


def head3d_wide_cls_unfused():
    """the parts arm with no part fused: (32, 16), no width a multiple of 64, and (128, 64) with `fuse_bn_proj` off; one HeadProjFn over
    the 16 features in canonical order."""
    head3d_layout(32, 16)
    head3d_layout(128, 64, fuse=False)


def head3d_uniform_unfused():
    """(64, 64) with `fuse_bn_proj` off: the uniform arm on FusedConvBNActFn + HeadProjSlicesFn at a width where FusedConvBNProjFn would be
    taken otherwise.  Eval: the stacked patch path."""
    head3d_layout(64, 64, fuse=False)


def head3d_no_stack():
    """regression widths not all equal (hd 32, the others 16): no second-layer stack, the per-branch second layer over one channel split of
    z1 and one HeadProjFn.  Eval: the per-branch patch path with its temporary padding edit."""
    head3d_layout(16, 16, hd=32)


def head3d_distill():
    """(128, 64) with `distill` on: InjectRowsFn between z1 and the channel split of the parts arm (training part only)."""
    head3d_layout(128, 64, distill=True, eval_too=False)


def head2d():
    """one level at 8x8, nc = 8: the 64 box-distribution outputs take HeadProjFn's wide (MFMA) arm, the 8 class outputs its narrow one"""
    import torch
    from yolov10_3d_amd import modules as M
    torch.manual_seed(2)
    hd = M.v10Detect(8, (64,))
    hd.stride = torch.tensor([8.0])
    hd.bias_init()
    hd = hd.to(DEV).train()
    x = torch.randn(2, 64, 8, 8, device=DEV).requires_grad_(True)
    out = hd([x])
    sum(t.float().sum() for t in out["one2many"] + out["one2one"]).backward()
    torch.cuda.synchronize()


def bottleneck_eval():
    """eval Bottleneck with shortcut: 32 channels (`y3d_conv2d_fwd_affine_res_ok` says yes) and 128 (no: conv + bn_act_fwd with the residual)"""
    import torch
    from yolov10_3d_amd import modules as M
    torch.manual_seed(3)
    for c in (32, 128):
        mod = M.Bottleneck(c, c, True, 1, (3, 3), 1.0).to(DEV).eval()
        with torch.no_grad():
            mod(torch.randn(2, c, 20, 20, device=DEV))
    torch.cuda.synchronize()


# ---- the loss glue: the public criterion classes of loss.py on the smallest cases of the loss tests ------------------------------------
def _on_device(maps, dtype, grad=True):
    from yolov10_3d_amd import ops
    return [ops._dense_any(m.to(DEV), dtype).requires_grad_(grad) for m in maps]


def loss3d_single():
    """DDDetectionLoss on separate maps (the Loss3dFn route): tests/test_hip_htl.py's B = 4, nc = 3 case, 64 + 16 + 4 anchors per image"""
    import torch
    import loss_ref as LR
    from test_hip_htl import CASES as HTL_CASES
    from yolov10_3d_amd import loss as PL
    case = HTL_CASES["b4_nc3_nl3"]
    with compute_dtype(torch.float32):
        batch, B = LR.make_batch(case)
        crit = PL.DDDetectionLoss(LR.model_of(case), tal_topk=case["topk"])
        loss, _ = crit(_on_device(LR.make_maps(case), torch.float32), {k: v.to(DEV) for k, v in batch.items()})
        loss.backward()
    torch.cuda.synchronize()


def _dual_odd(dtype):
    """DetectLoss3d + the head's own (B, 2 * no, H, W) maps of loss_ref's l3_dual_o2o / l3_dual_o2m pair (nc = 2, no = 37) + the batch"""
    import torch
    import loss_ref as LR
    from yolov10_3d_amd import loss as PL
    c1, cm = LR.BY_NAME["l3_dual_o2o"], LR.BY_NAME["l3_dual_o2m"]
    batch, B = LR.make_batch(c1)
    no = c1["nc"] + 35
    crit = PL.DetectLoss3d(LR.model_of(cm))

    def preds():
        bases = _on_device([torch.cat((x, y), 1) for x, y in zip(LR.make_maps(c1, dtype), LR.make_maps(cm, dtype))], dtype)
        return {"one2one": [b[:, :no] for b in bases], "one2many": [b[:, no:] for b in bases], "_y3d_maps": bases}

    return crit, preds, {k: v.to(DEV) for k, v in batch.items()}


def loss3d_dual_odd():
    """DetectLoss3d on shared maps, bf16: the DualLoss3dFn route with the one-to-many half at an odd element offset"""
    import torch
    with compute_dtype(torch.bfloat16):
        crit, preds, batch = _dual_odd(torch.bfloat16)
        loss, _ = crit(preds(), batch)
        loss.backward()
    torch.cuda.synchronize()


def loss3d_weighted():
    """the same criterion with an item-weight table: with grad, under no_grad (a null gradient-pointer array), and after
    set_item_weights(None)"""
    import torch
    with compute_dtype(torch.float32):
        crit, preds, batch = _dual_odd(torch.float32)
        crit.set_item_weights(torch.linspace(0.5, 1.6, 12, device=DEV))
        loss, _ = crit(preds(), batch)
        loss.backward()
        with torch.no_grad():
            crit(preds(), batch)
        crit.set_item_weights(None)
        loss, _ = crit(preds(), batch)
        loss.backward()
    torch.cuda.synchronize()


def loss3d_distill(fused):
    """DetectLoss3d with `distillation: True` behind the two-level 12x12 + 8x8 head of tests/test_hip_distill.py, the teacher map in the
    batch.  fused: the head's shared maps and z1 slots (compact rows, ops.InjectRowsFn); else the per-branch head: two calls and dense
    embedding gradients (DistillFn.backward)."""
    import torch
    from types import SimpleNamespace
    import yolov10_3d_amd as y3d
    from bench import synth_batch
    from test_hip_distill import _head
    from yolov10_3d_amd import loss as PL
    with compute_dtype(torch.float32):
        hd = _head((64, 64), DEV)
        hd.fused = fused
        hyp = dict(y3d.tasks.DEFAULT_HYP, distillation=True, distillation_temp=2.0, distillation_weight=1.0, distillation_loss="soft",
                   distillation_no_mixup=True)
        crit = PL.DetectLoss3d(SimpleNamespace(model=[hd], args=SimpleNamespace(**hyp)))
        g = torch.Generator().manual_seed(8)
        xs = [torch.randn(2, 32, 12, 12, generator=g).to(DEV).requires_grad_(True), torch.randn(2, 64, 8, 8, generator=g).to(DEV).requires_grad_(True)]
        batch = synth_batch(2, 96, 96, 5, DEV)
        batch["mixed"] = torch.tensor([0, 0], dtype=torch.uint8, device=DEV)
        batch["teacher_emb"] = torch.randn(2, 64, 5, 7, generator=g).to(DEV)
        out = hd(xs)
        assert ("_y3d_distill" in out) == fused
        loss, items = crit(out, batch)
        assert items.numel() == 14
        loss.backward()
    torch.cuda.synchronize()


def loss2d(max_boxes):
    """v10DetectLoss: max_boxes=None on loss_ref's one-level 2D case (the dense assigner), max_boxes=128 on the 65-box crowd"""
    import torch
    import crowded_cases as CC
    import loss_ref as LR
    from yolov10_3d_amd import loss as PL
    case = LR.BY_NAME["l2_nl1"] if max_boxes is None else CC.BY_NAME["c65_nc1_k10"]
    with compute_dtype(torch.float32), CC.registered():
        batch, B = LR.make_batch(case)
        maps = LR.make_maps(case, seed=case["seeds"]["fp32"] if max_boxes else None)
        crit = PL.v10DetectLoss(LR.model_of(case), max_boxes=max_boxes)
        loss, _ = crit({"one2many": _on_device(maps, torch.float32), "one2one": _on_device(maps, torch.float32)}, {k: v.to(DEV) for k, v in batch.items()})
        loss.backward()
        PL.check_target_overflow(wait=True)
    torch.cuda.synchronize()


def loss_fgdm():
    """ForegroundDepthMapLoss on logits (2, 81, 2, 3) and float32 depth maps (2, 32, 48), forward + backward"""
    import torch
    from types import SimpleNamespace
    from yolov10_3d_amd import loss as PL
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 81, 2, 3, generator=g).to(DEV).requires_grad_(True)
    dm = (torch.rand(2, 32, 48, generator=g) * 60.0 * (torch.rand(2, 32, 48, generator=g) > 0.5)).to(DEV)
    PL.ForegroundDepthMapLoss(SimpleNamespace(min_depth_threshold=1, max_depth_threshold=120))(z, dm).backward()
    torch.cuda.synchronize()


CASES = {
    "tiny/bf16": lambda: tiny("bf16"),
    "tiny/f32": lambda: tiny("f32"),
    "tiny/bf16/PACK_CACHE_off": lambda: tiny(off="PACK_CACHE"),
    "tiny/bf16/STEM_FUSED_off": lambda: tiny(off="STEM_FUSED"),
    "tiny/bf16/PROJ_BN_MFMA_off": lambda: tiny(off="PROJ_BN_MFMA"),
    "tiny/bf16/DW_EVAL_FUSED_off": lambda: tiny(off="DW_EVAL_FUSED"),
    "tiny/bf16/PLACEMENT_off": lambda: tiny(off="PLACEMENT"),
    "tiny/bf16/two_steps": lambda: tiny(steps=2),
    "tiny/bf16/fused_eval": lambda: tiny(steps=0, fuse=True),
    "stem/u8": stem_u8,
    "stem/u8/STEM_FUSED_off": lambda: stem_u8("STEM_FUSED"),
    "fp8/weights": lambda: head3d("fp8"),
    "fp8/conv": lambda: head3d("fp8", conv=True, eval_too=True),  # eval: the fp8 kernel's affine epilogue, the matrix-core proj_slices_eval
    "fp8/dgrad": lambda: head3d("fp8", conv=True, dgrad=True),
    "head3d/PROJ_BN_MFMA_off": lambda: head3d(off="PROJ_BN_MFMA", eval_too=True),  # (the tiny model's 16-wide head never takes the matrix-core forms)
    "head2d": head2d,
    "bottleneck_eval": bottleneck_eval,
    "head3d/wide_cls/fused": head3d_wide_cls_fused,
    "head3d/wide_cls/mixed": head3d_wide_cls_mixed,
    "head3d/wide_cls/unfused": head3d_wide_cls_unfused,
    "head3d/uniform/unfused": head3d_uniform_unfused,
    "head3d/no_stack": head3d_no_stack,
    "head3d/distill": head3d_distill,
    "loss/3d/single": loss3d_single,
    "loss/3d/dual_odd": loss3d_dual_odd,
    "loss/3d/weighted": loss3d_weighted,
    "loss/3d/distill/two_call": lambda: loss3d_distill(False),
    "loss/3d/distill/slots": lambda: loss3d_distill(True),
    "loss/2d/dense": lambda: loss2d(None),
    "loss/2d/crowded": lambda: loss2d(128),
    "loss/fgdm": loss_fgdm,
}

# the head layout cases: (launches a case must hold, launches it must not), looked at when the fixture is minted
HEAD_LAYOUT_CALLS = {
    "head3d/wide_cls/fused": (("proj_group_bn_bwd",), ("proj_bwd_weight", "proj_group_bwd_weight")),
    "head3d/wide_cls/mixed": (("proj_group_bn_bwd", "proj_bwd_weight"), ("proj_group_bwd_weight",)),
    "head3d/wide_cls/unfused": (("proj_bwd_weight",), ("proj_group_bn_bwd", "proj_group_bwd_weight")),
    "head3d/uniform/unfused": (("proj_group_bwd_weight", "proj_group_fwd_bn_mfma"), ("proj_group_bn_bwd", "proj_bwd_weight")),
    "head3d/no_stack": (("proj_bwd_weight",), ("proj_group_bn_bwd", "proj_group_bwd_weight", "proj_group_fwd_bn_mfma")),
    "head3d/distill": (("proj_group_bn_bwd", "distill_scatter"), ("proj_bwd_weight",)),
}


def off_layout(traces):
    """the head layout cases whose trace does not show the arm they are for"""
    bad = []
    for case, (must, must_not) in HEAD_LAYOUT_CALLS.items():
        names = {c[0] for c in traces[case]}
        if not set(must) <= names or names & set(must_not):
            bad.append(case)
    return bad


def run_case(name):
    """-> the calls of one case, [[name, [arguments]], ...]"""
    import torch
    from yolov10_3d_amd import ops
    torch.cuda.synchronize()
    try:
        with fresh_registries():
            CASES[name]()  # unrecorded: whatever the process does once (module loads, tables, caches) happens here
        calls = []
        with fresh_registries(), recording(calls):
            CASES[name]()
    finally:
        ops.reset_placement()
    return json.loads(json.dumps(calls))


# ---- which arms of the conv + BatchNorm + activation glue and of the loss glue a trace reaches -------------------------------------
def _has(name, cond=lambda a: True):
    return lambda calls: any(c[0] == name and cond(c[1]) for c in calls)


ARMS = {
    "_stem_forward: fused eval (stem_conv_eval)": _has("stem_conv_eval"),
    "_stem_forward: fused training (stem_conv_train)": _has("stem_conv_train"),
    "_stem_forward: im2col of a float image + dense conv": _has("stem_im2col"),
    "_stem_forward: im2col of a uint8 image + dense conv": _has("stem_im2col_u8"),
    "_dw_forward: eval, BatchNorm + SiLU in the epilogue": _has("dwconv2d_fwd_affine", lambda a: a[13] == 0),
    "_dw_forward: eval, epilogue with a residual": _has("dwconv2d_fwd_affine", lambda a: a[13] != 0),
    "_dw_forward: eval, conv + tail (DW_EVAL_FUSED off)": _has("dwconv2d_fwd", lambda a: a[-2] == 0),
    "_dw_forward: training": _has("dwconv2d_fwd", lambda a: a[-2] == 1),
    "_dw_packed: packed on the spot": _has("dw_pack_weight"),
    "_dense_forward: fp8 eval (affine epilogue)": _has("conv3x3_fp8_fwd", lambda a: a[12] == 0 and a[13] == 1),
    "_dense_forward: fp8 training": _has("conv3x3_fp8_fwd", lambda a: a[12] == 1),
    "_dense_forward: eval, affine epilogue": _has("conv2d_fwd_affine"),
    "_dense_forward: eval, affine epilogue with the residual": _has("conv2d_fwd_affine_res"),
    "_dense_forward: eval, conv + tail with the residual": _has("conv2d_fwd", lambda a: a[-2] == 0 and a[10] == 0),
    "_dense_forward: training": _has("conv2d_fwd", lambda a: a[-2] == 1),
    "forward pack on the spot": _has("pack_weight_fwd"),
    "registry refresh-all": _has("mt_pack_weights"),
    "_bn_act_tail: training statistics": _has("bn_finalize"),
    "_bn_act_tail: apply + fp8 copy": _has("bn_act_fwd_q"),
    "_bn_act_tail: apply": _has("bn_act_fwd", lambda a: a[6] == 0),
    "_bn_act_tail: apply, res_mode 1": _has("bn_act_fwd", lambda a: a[6] == 1),
    "_bn_act_tail: apply, res_mode 2": _has("bn_act_fwd", lambda a: a[6] == 2),
    "_conv_backward: depth-wise data gradient": _has("dwconv2d_bwd_data"),
    "_conv_backward: depth-wise weight gradient": _has("dwconv2d_bwd_weight"),
    "_conv_backward: fp8 data gradient": _has("conv3x3_fp8_dgrad"),
    "_conv_backward: data-gradient pack on the spot": _has("pack_weight_dgrad"),
    "_conv_backward: data gradient": _has("conv2d_bwd_data"),
    "_conv_backward: weight gradient": _has("conv2d_bwd_weight"),
    "HeadProjFn: narrow arm": _has("proj_fwd"),
    "HeadProjFn: narrow arm, backward": _has("proj_bwd_weight"),
    "HeadProjFn: wide arm, backward (bias column sums)": _has("colsum_partials"),
    "HeadProjSlicesFn / FusedConvBNProjFn: VALU forms": _has("proj_group_fwd_bn"),
    "FusedConvBNProjFn: matrix-core forms": _has("proj_group_bn_bwd"),
    "proj_slices_eval: matrix-core form": _has("proj_group_fwd_bn_mfma", lambda a: a[10] == 0),
    "conv_bias_act_eval (folded model)": _has("bn_eval_scale", lambda a: a[5] == 0.0),
    "Loss2dFn: dense assigner": _has("tal2d_assign"),
    "Loss2dFn: crowded assigner": _has("tal2d_assign_crowded"),
    "Loss2dFn: loss + gradient rows": _has("loss2d"),
    "_loss3d_set: weighted entry with a gradient-pointer array": _has("loss3d_weighted", lambda a: a[4] != 0),
    "_loss3d_set: weighted entry under no_grad (null gradient-pointer array)": _has("loss3d_weighted", lambda a: a[4] == 0),
    "DistillFn: forward": _has("distill_loss"),
    "DistillFn: backward, dense embedding gradient (pixel stride = width)": _has("distill_scatter", lambda a: a[10] == a[6]),
    "FgdmLossFn: forward": _has("fgdm_loss"),
    "FgdmLossFn: backward": _has("fgdm_scale"),
}


def unreached(traces):
    calls = [c for t in traces.values() for c in t]
    return [arm for arm, hit in ARMS.items() if not hit(calls)]


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def pack(traces):
    """{case: calls} -> the stored form: every distinct call once, the cases as index lists"""
    table, index = [], {}
    cases = []
    for name, calls in traces.items():
        seq = []
        for c in calls:
            k = json.dumps(c)
            if k not in index:
                index[k] = len(table)
                table.append(c)
            seq.append(index[k])
        cases.append([name, seq])
    return {"calls": table, "cases": cases}


def unpack(stored):
    return {name: [stored["calls"][i] for i in seq] for name, seq in stored["cases"]}


def load(path=OUT):
    with gzip.open(path, "rt") as f:
        return unpack(json.load(f))


def first_difference(got, want, context=10):
    """None when the two call lists are equal, else a report: the first differing call with `context` calls around it"""
    if got == want:
        return None
    i = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    lines = [f"{len(got)} calls, {len(want)} recorded; first difference at call {i}"]
    for j in range(max(0, i - context), min(max(len(got), len(want)), i + context + 1)):
        a = got[j] if j < len(got) else None
        b = want[j] if j < len(want) else None
        lines.append(f"{'>>' if j == i else '  '} {j}: {a}" + ("" if a == b else f"\n      recorded: {b}"))
    return "\n".join(lines)


def main():
    traces = {name: run_case(name) for name in CASES}
    miss = unreached(traces)
    if "--check" in sys.argv:
        want = load()
        bad = [name for name in CASES if traces[name] != want.get(name)]
        for name in bad:
            print(f"{name}:\n{first_difference(traces[name], want.get(name, []))}")
        print(f"{len(CASES) - len(bad)} of {len(CASES)} cases equal the fixture")
        sys.exit(1 if bad else 0)
    if miss and "--allow-unreached" not in sys.argv:
        sys.exit(f"arms not reached by any case: {miss}")
    print(f"arms not reached: {miss}")
    if off_layout(traces):
        sys.exit(f"head layout cases that did not reach their arm: {off_layout(traces)}")
    out =sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps(pack(traces), separators=(",", ":")).encode())
    names = sorted({c[0] for t in traces.values() for c in t})
    print(f"{out}: {len(CASES)} cases, {sum(len(t) for t in traces.values())} calls of {len(names)} functions, {os.path.getsize(out)} bytes")
    for name, t in traces.items():
        print(f"  {name}: {len(t)} calls")


if __name__ == "__main__":
    main()
