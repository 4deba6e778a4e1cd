"""GPU: frozen layers (`train.apply_freeze`) against the unfrozen model built from the same seed on the same batch, on yolov10n_3D /
yolov10n at 256 x 256, B = 2.

Every kernel on this path is deterministic (tests/test_hip_train.py relies on that bit for bit) and a frozen layer runs the same forward
and hands the same data gradient on, so every comparison is torch.equal: loss, loss items, and the gradient of every trainable
parameter; a frozen parameter has no gradient.  The one number with a bound is the optimizer's gradient norm over the trainable
parameters against a float64 sum: the any-order bound of tests/test_hip_optim.py, (chunk + 1) u + 2^-23 relative.

Call traces (the recording proxy of tools/make_golden_ops_trace.py): a forward pre-hook on every yaml layer writes a marker into the
trace, so every forward conv / BatchNorm-apply call belongs to a layer; a body layer makes exactly one weight-gradient call per forward
conv call of the same geometry and one BatchNorm backward reduce + apply per forward apply of the same (pixels, channels).  What a
freeze must leave of the unfrozen backward is therefore computed from the unfrozen trace by layer - nothing is hard-coded."""
import collections
import importlib.util
import os

import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import mt, ops, optim, train
from yolov10_3d_amd.modules import Conv

import stem_optim_ref as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_ops_trace", os.path.join(ROOT, "tools", "make_golden_ops_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tool()


@pytest.fixture(scope="module")
def batches():
    from bench import synth_batch
    return [synth_batch(2, 256, 256, 40 + j, DEV) for j in range(4)]


@pytest.fixture(autouse=True)
def _bf16_after():
    yield
    y3d.set_compute_dtype(BF16)


def make(freeze, dtype=BF16, name="yolov10n_3D.yaml", seed=3):
    y3d.set_compute_dtype(dtype)
    torch.manual_seed(seed)
    model = (y3d.YOLOv10_3DDetectionModel if "_3D" in name else y3d.YOLOv10DetectionModel)(name).to(DEV).train()
    head = model.model[-1]
    if hasattr(head, "restack"):
        head.restack()
    frozen = train.apply_freeze(model, freeze)
    return model, frozen


def step(model, batch):
    """forward + loss + backward -> (loss, items, {name: gradient or None})"""
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    out = loss.detach().clone(), items.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    del loss
    return out


def same_step(got, want, frozen, what):
    assert torch.equal(got[0], want[0]), f"{what}: loss"
    assert torch.equal(got[1], want[1]), f"{what}: loss items"
    frozen = set(frozen)
    n = 0
    for k, g in got[2].items():
        if k in frozen:
            assert g is None, f"{what}: frozen {k} has a gradient"
        else:
            w = want[2][k]
            assert (g is None) == (w is None), f"{what}: {k}"
            if g is not None:
                n += 1
                assert torch.equal(g, w), f"{what}: gradient of {k} differs"
    assert n > 0


@pytest.fixture(scope="module")
def unfrozen(batches):
    """one unfrozen step per (model, dtype), made once and left unchanged"""
    out = {}
    for name, dtype in (("yolov10n_3D.yaml", BF16), ("yolov10n_3D.yaml", F32), ("yolov10n.yaml", BF16)):
        model, frozen = make(None, dtype, name)
        assert frozen == ([] if "_3D" in name else ["model.23.dfl.conv.weight"])
        out[(name, dtype)] = step(model, batches[0])
        del model
    y3d.set_compute_dtype(BF16)
    return out


FREEZES = [11, [4, 13], [23]]


@pytest.mark.parametrize("freeze", FREEZES, ids=str)
def test_frozen_step_equals_the_unfrozen_one_and_the_optimizer_leaves_frozen_alone(batches, unfrozen, freeze):
    want = unfrozen[("yolov10n_3D.yaml", BF16)]
    model, frozen = make(freeze)
    assert frozen
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = optim.build_optimizer(model, lr=0.01)
    got = step(model, batches[0])
    same_step(got, want, frozen, f"freeze={freeze}")
    opt.step(max_norm=10.0)
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    for k in frozen:
        assert torch.equal(named[k].detach(), before[k]), f"the step moved frozen {k}"
    assert any(not torch.equal(p.detach(), before[k]) for k, p in named.items() if k not in set(frozen)), "nothing was trained"
    # BatchNorm of a frozen module stays in training mode: its running statistics move
    stems = {k[:-len(".weight")] for k in frozen if k.endswith(".bn.weight")}
    now = model.state_dict()
    moved = [s for s in stems if not torch.equal(now[s + ".running_mean"], before[s + ".running_mean"])]
    assert stems and moved, "no frozen BatchNorm moved its running mean"
    # the norm the step clipped by: over the trainable gradients only
    sq = sum(float(g.double().pow(2).sum()) for k, g in want[2].items() if g is not None and k not in set(frozen))
    norm = sq ** 0.5
    total = sum(float(g.double().pow(2).sum()) for g in want[2].values() if g is not None) ** 0.5
    got_norm = float(opt.last_norm[0])
    print(f"freeze={freeze}: norm {got_norm:.9g}, float64 over the trainable gradients {norm:.9g}, over all {total:.9g}")
    assert abs(got_norm - norm) <= ((mt.CHUNK + 1) * S.U + 2.0 ** -23) * norm
    assert total > norm


def test_frozen_prefix_fp32(batches, unfrozen):
    model, frozen = make(11, F32)
    same_step(step(model, batches[0]), unfrozen[("yolov10n_3D.yaml", F32)], frozen, "fp32 freeze=11")


@pytest.mark.parametrize("freeze", [11, [23]], ids=str)
def test_frozen_2d_model(batches, unfrozen, freeze):
    """yolov10n.yaml: the 2D head's projections (HeadProjFn, narrow and wide arm); `.dfl` is frozen under every setting"""
    model, frozen = make(freeze, BF16, "yolov10n.yaml")
    assert "model.23.dfl.conv.weight" in frozen
    same_step(step(model, batches[0]), unfrozen[("yolov10n.yaml", BF16)], frozen, f"2D freeze={freeze}")


def test_frozen_layers_on_the_fp8_routes(batches):
    """set_weight_quant("fp8") + set_fp8_conv(True) + set_fp8_dgrad(True), freeze=[4, 13].  At 256 x 256 the n model reaches the fp8
    kernels in layer 8 (C2f, 128 -> 128 3x3 convs on the 8 x 8 map: the kernel takes Cin / groups >= 128) - asserted below from the
    trace; layers 4 and 13 themselves are narrower and run bf16, with the fp8 layers' gradients flowing through them."""
    try:
        ops.set_weight_quant("fp8")
        ops.set_fp8_conv(True)
        ops.set_fp8_dgrad(True)
        with T.fresh_registries():
            model, _ = make(None)
            sink = []
            with T.recording(sink):
                want = step(model, batches[0])
            names = {c[0] for c in sink}
            assert "conv3x3_fp8_fwd" in names and "conv3x3_fp8_dgrad" in names, "the fp8 routes were not reached: the case checks nothing"
            del model
        with T.fresh_registries():
            model, frozen = make([4, 13])
            same_step(step(model, batches[0]), want, frozen, "fp8 freeze=[4, 13]")
    finally:
        ops.set_weight_quant(None)
        ops.set_fp8_conv(False)


def test_depth_predictor_with_frozen_parameters_or_inputs():
    """ConvGroupNormFn / DepthClassifierFn (the head's `fgdm_predictor`): all parameters frozen over inputs that need a gradient, and
    trainable parameters over inputs that need none, each against the run where everything needs one: the gradients that remain are
    bit-equal, the others are None."""
    from yolov10_3d_amd.modules import DepthPredictor
    y3d.set_compute_dtype(BF16)
    torch.manual_seed(5)
    dp = DepthPredictor((64, 128, 256)).to(DEV).train()
    g = torch.Generator().manual_seed(6)
    shapes = [(2, 64, 32, 32), (2, 128, 16, 16), (2, 256, 8, 8)]
    feats0 = [torch.randn(s, generator=g).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last) for s in shapes]
    cot = torch.randn(2, 81, 16, 16, generator=g).to(DEV)
    trainable = [k for k, p in dp.named_parameters() if p.requires_grad]
    assert "depth_bin_values" not in trainable and len(trainable) == 22

    def run(params, inputs):
        for k, p in dp.named_parameters():
            p.grad = None
            if k in trainable:
                p.requires_grad = params
        feats = [f.clone().requires_grad_(inputs) for f in feats0]
        logits, _ = dp(feats)
        (logits.float() * cot).sum().backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), [f.grad for f in feats], {k: p.grad for k, p in dp.named_parameters()}

    full = run(True, True)
    assert all(t is not None for t in full[1]) and all(full[2][k] is not None for k in trainable)
    frozen = run(False, True)
    assert torch.equal(frozen[0], full[0])
    assert all(torch.equal(a, b) for a, b in zip(frozen[1], full[1])) and all(v is None for v in frozen[2].values())
    blind = run(True, False)
    assert torch.equal(blind[0], full[0]) and all(t is None for t in blind[1])
    assert all(torch.equal(blind[2][k], full[2][k]) for k in trainable)
    for k, p in dp.named_parameters():
        if k in trainable:
            p.requires_grad = True


# ---- call traces ------------------------------------------------------------------------------------------------------------------------------
WGRAD = ("conv2d_bwd_weight", "dwconv2d_bwd_weight")
DGRAD = ("conv2d_bwd_data", "dwconv2d_bwd_data")
BN_BWD = ("bn_act_bwd_reduce", "bn_act_bwd_apply")
# what an all-frozen head leaves out besides its convs' weight gradients: the projection weight / bias gradient launches
HEAD_WGRAD = ("proj_group_bwd_weight_bn_mfma", "proj_group_bwd_weight_bn", "proj_group_bwd_weight", "proj_bwd_weight", "colsum_partials", "colsum")


def conv_key(name, a):
    """the geometry (kind, B, H, W, Cin, Cout, groups, k, stride, pad) a conv call works on, the same for forward, data and weight gradient"""
    if name == "conv2d_fwd":
        return ("dense", a[5], a[6], a[7], a[8], a[15], a[16], a[17], a[19], a[20])
    if name == "conv2d_bwd_weight":
        return ("dense", a[5], a[6], a[7], a[8], a[14], a[15], a[16], a[18], a[19])
    if name == "conv2d_bwd_data":
        return ("dense", a[5], a[12], a[13], a[14], a[8], a[15], a[16], a[18], a[19])
    if name == "dwconv2d_fwd":
        return ("dw", a[5], a[6], a[7], a[8], a[8], a[8], a[14], a[16], a[17])
    if name == "dwconv2d_bwd_weight":
        return ("dw", a[5], a[6], a[7], a[8], a[8], a[8], a[13], a[15], a[16])
    if name == "dwconv2d_bwd_data":
        return ("dw", a[5], a[12], a[13], a[8], a[8], a[8], a[14], a[16], a[17])
    if name == "stem_conv_train":  # the stem runs as a 1x1 conv over 32 im2col channels of its output map; its weight gradient too
        return ("dense", a[7], (a[8] - 1) // 2 + 1, (a[9] - 1) // 2 + 1, 32, a[10], 1, 1, 1, 0)
    return None


def bn_key(a):
    return (a[-3], a[-2])  # (pixels, channels)


def traced_step(model, batch):
    """-> the trace of one forward + backward with ["@layer", i] markers, and the number of Conv modules in trainable layers whose input
    carried no gradient (their data gradient does not exist)"""
    sink, blind, hooks = [], [], []
    for i, m in enumerate(model.model):
        hooks.append(m.register_forward_pre_hook(lambda mod, inp, i=i: sink.append(["@layer", i])))
    trainable = {id(m) for m in model.modules() if isinstance(m, Conv) and any(p.requires_grad for p in m.parameters())}
    for m in model.modules():
        if id(m) in trainable:
            hooks.append(m.register_forward_pre_hook(lambda mod, inp: blind.append(1) if not inp[0].requires_grad else None))
    try:
        with T.fresh_registries(), T.recording(sink):
            loss, _ = model(batch)
            sink.append(["@backward", 0])
            loss.backward()
            torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    return sink, len(blind)


def by_layer(trace):
    """forward conv keys and BatchNorm-apply keys per yaml layer; the backward's weight-gradient, data-gradient and BatchNorm keys"""
    fwd, bn = collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter)
    wg, dg, bb, names = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    layer, backward = None, False
    for name, a in trace:
        if name == "@layer":
            layer = a
        elif name == "@backward":
            backward = True
        elif not backward:
            if name in ("conv2d_fwd", "dwconv2d_fwd", "stem_conv_train"):
                fwd[layer][conv_key(name, a)] += 1
            elif name in ("bn_act_fwd", "bn_act_fwd_q"):
                bn[layer][bn_key(a)] += 1
        else:
            names[name] += 1
            if name in WGRAD:
                wg[conv_key(name, a)] += 1
            elif name in DGRAD:
                dg[conv_key(name, a)] += 1
            elif name in BN_BWD:
                bb[(name, bn_key(a))] += 1
    return fwd, bn, wg, dg, bb, names


def total(counters, layers):
    out = collections.Counter()
    for i in layers:
        out.update(counters.get(i, {}))
    return out


@pytest.fixture(scope="module")
def unfrozen_trace(batches):
    model, _ = make(None)
    trace, blind = traced_step(model, batches[0])
    fwd, bn, wg, dg, bb, names = by_layer(trace)
    body = range(23)
    # what the derivations below stand on, checked on the unfrozen trace itself: one weight-gradient call per forward conv of every
    # layer (head included), one BatchNorm reduce + apply per forward apply of a body layer, a data gradient for every conv but the stem
    assert wg == total(fwd, range(24)), "weight-gradient calls do not pair up with the forward convs"
    assert sum(wg.values()) > 50
    body_bn = total(bn, body)
    for name in BN_BWD:
        assert all(bb[(name, k)] >= n for k, n in body_bn.items())
    assert blind == 1, "only the stem's input carries no gradient in the unfrozen model"
    assert sum(dg.values()) >= sum(total(fwd, body).values()) - 1
    return fwd, bn, wg, dg, bb, names


def test_trace_frozen_prefix_has_no_backward(batches, unfrozen_trace):
    fwd, bn, wg, dg, bb, names = unfrozen_trace
    model, _ = make(11)
    trace, blind = traced_step(model, batches[0])
    f_fwd, f_bn, f_wg, f_dg, f_bb, f_names = by_layer(trace)
    assert f_fwd == fwd and f_bn == bn, "the forward of a frozen model makes other conv / BatchNorm calls"
    low, high = range(11), range(11, 24)
    low_convs, low_bn = total(fwd, low), total(bn, low)
    high_convs, high_bn = total(fwd, high), total(bn, high)
    # exactly the weight-gradient calls of layers 11-23, which also says: none of a geometry that only layers 0-10 have
    assert f_wg == wg - low_convs == high_convs
    assert sum(f_wg.values()) == sum(high_convs.values()) < sum(wg.values())
    only_low = [k for k in low_convs if k not in high_convs]
    assert only_low and all(f_wg[k] == 0 and f_dg[k] == 0 for k in only_low)
    # BatchNorm backward: the unfrozen calls minus one reduce + apply per forward apply of layers 0-10
    for name in BN_BWD:
        want = collections.Counter({k[1]: n for k, n in bb.items() if k[0] == name}) - low_bn
        got = collections.Counter({k[1]: n for k, n in f_bb.items() if k[0] == name})
        assert got == want, name
        assert all(got[k] == 0 for k in low_bn if k not in high_bn)
    # data gradients: none below layer 11, and none for the trainable convs whose input comes from frozen layers alone
    assert blind >= 1
    assert sum(f_dg.values()) == sum(dg.values()) - (sum(low_convs.values()) - 1) - blind
    assert not (f_dg - dg)


def test_trace_frozen_inner_layers_keep_their_data_gradients(batches, unfrozen_trace):
    fwd, bn, wg, dg, bb, names = unfrozen_trace
    model, _ = make([4, 13])
    trace, blind = traced_step(model, batches[0])
    f_fwd, f_bn, f_wg, f_dg, f_bb, f_names = by_layer(trace)
    assert f_fwd == fwd and f_bn == bn
    gone = total(fwd, [4, 13])
    assert sum(gone.values()) >= 8
    assert f_wg == wg - gone and sum(f_wg.values()) == sum(wg.values()) - sum(gone.values())
    assert f_dg == dg, "dx still passes through the frozen layers"
    assert f_bb == bb, "the BatchNorm backward of a frozen layer still runs: its sums feed the apply pass"


def test_trace_frozen_head_makes_no_weight_gradient(batches, unfrozen_trace):
    fwd, bn, wg, dg, bb, names = unfrozen_trace
    assert any(names[n] for n in HEAD_WGRAD), "the unfrozen head launches none of the calls this test looks for"
    model, _ = make([23])
    trace, blind = traced_step(model, batches[0])
    f_fwd, f_bn, f_wg, f_dg, f_bb, f_names = by_layer(trace)
    assert f_fwd == fwd and f_bn == bn
    assert all(f_names[n] == 0 for n in HEAD_WGRAD), {n: f_names[n] for n in HEAD_WGRAD if f_names[n]}
    head = total(fwd, [23])
    assert sum(head.values()) >= 6
    assert f_wg == wg - head == total(fwd, range(23))
    assert f_dg == dg and f_bb == bb
    for n in ("proj_group_bn_bwd", "bn_bwd_finalize"):  # the BatchNorm backward through the projections stays: dx needs it
        assert f_names[n] == names[n]


# ---- GradAccumulator over a frozen model --------------------------------------------------------------------------------------------------------
def snapshot(model, opt):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone()


def test_accumulator_over_a_frozen_model(batches):
    def new():
        model, frozen = make(11)
        return model, optim.build_optimizer(model, lr=0.01), frozen

    model, opt, frozen = new()
    acc = optim.GradAccumulator(model.parameters())
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert [id(p) for p in acc.params] == [id(p) for p in trainable] and len(trainable) + len(frozen) == len(list(model.parameters()))
    assert acc.sizes == [p.numel() for p in trainable]
    assert acc.total == sum((n + 3) // 4 * 4 for n in acc.sizes), "the arena holds the trainable sizes only"
    after = []
    for w in range(2):
        for b in batches[2 * w:2 * w + 2]:
            loss, _ = model(b)
            loss.backward()
            del loss
            acc.add()
            assert all(p.grad is None for p in model.parameters())
        acc.bind()
        opt.step(max_norm=10.0)
        acc.reset()
        after.append(snapshot(model, opt))
    assert acc.arena.numel() == acc.total
    model, opt, _ = new()
    for w in range(2):
        for b in batches[2 * w:2 * w + 2]:
            loss, _ = model(b)
            loss.backward()  # autograd adds into the persistent p.grad
            del loss
        opt.step(max_norm=10.0)
        opt.zero_grad()
        got = snapshot(model, opt)
        for k, v in got[0].items():
            assert torch.equal(v, after[w][0][k]), f"window {w}: {k}"
        assert torch.equal(got[1], after[w][1]), f"window {w}: optimizer state"


def test_graphed_step_refuses_frozen_layers(batches):
    from yolov10_3d_amd import graph
    from yolov10_3d_amd._lib import Y3DError
    model, _ = make(11)
    opt = optim.build_optimizer(model, lr=0.01)
    with pytest.raises(Y3DError, match="frozen layers"):
        graph.GraphedTrainStep(model, opt, batches[0])
