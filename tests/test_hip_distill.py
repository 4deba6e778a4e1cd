"""GPU: feature distillation (csrc/distill.hip, loss.DistillFn, ops.InjectRowsFn) against the float64 restatement of the reference
(tests/distill_ref.py) and the reference's own fixtures (tests/golden/distill.npz, loss3d_distill.npz)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, has_gpu, load_golden

import distill_ref as DR
import yolov10_3d_amd as y3d
from yolov10_3d_amd import loss as PL, modules as M, ops

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV = "cuda"
Z = np.load(os.path.join(GOLDEN, "distill.npz"))
CASES = sorted(k[:-4] for k in Z.files if k.endswith("/cfg"))
TSS = 1.75  # the target-score sum the item is divided by (any value > 1)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def levels_of(emb, dtype):
    """(B, C, A) -> one NHWC (B, C, H, W) map per fixture level"""
    out, a0 = [], 0
    for h, w in Z["levels"]:
        out.append(ops._dense_any(emb[:, :, a0:a0 + h * w].reshape(emb.shape[0], emb.shape[1], h, w).to(DEV), dtype))
        a0 += h * w
    return out


def padded_gt(gt_center, mask_gt):
    """(B, n, 17) padded targets carrying only what the kernel reads: a box with a positive coordinate sum on valid rows, center_3d"""
    g = torch.zeros(*mask_gt.shape, 17)
    g[..., 1:5] = torch.as_tensor(mask_gt).float().unsqueeze(-1) * torch.tensor([1.0, 2.0, 30.0, 40.0])
    g[..., 9:11] = torch.as_tensor(gt_center)
    return g.to(DEV)


def run_kernel(i, cfg, dtype, nhwc_teacher, teacher_dtype, fg=None, mixed=None):
    C, crit, T, nomix = cfg
    emb = torch.from_numpy(i["emb"])
    embs = [e.requires_grad_(True) for e in levels_of(emb, dtype)]
    t = torch.from_numpy(i["teacher"]).to(DEV).to(teacher_dtype)
    if nhwc_teacher:
        t = t.contiguous(memory_format=torch.channels_last)
    fg = torch.from_numpy(i["fg"] if fg is None else fg)
    B, A = fg.shape
    spec = dict(embs=[e.detach() for e in embs], teacher=t, gt=padded_gt(i["gt_center"], i["mask_gt"]), fg=fg.to(DEV).to(torch.uint8),
                gi=torch.from_numpy(i["gt_idx"]).to(DEV).int(), scal=torch.tensor([TSS, 0.0], device=DEV),
                mixed=torch.from_numpy(i["mixed"] if mixed is None else mixed).to(DEV).to(torch.uint8), img_wh=tuple(int(v) for v in Z["img_wh"]), T=T,
                weight=float(Z["weight"]), crit=int(crit), no_mixup=bool(nomix), cap=B * A, slots=None, which=0)
    item = PL.DistillFn.apply(spec, *embs)
    item.backward()
    torch.cuda.synchronize()
    grad = torch.cat([e.grad.float().reshape(B, int(C), -1) for e in embs], 2).cpu().numpy()
    rows, idx, counts = [v.cpu() for v in spec["compact"]]
    return float(item.detach()), grad, rows.float().numpy(), idx.numpy(), counts.numpy()


def inputs(name):
    cfg = Z[f"{name}/cfg"]
    return {k: Z[f"in{int(cfg[0])}/{k}"] for k in ("emb", "teacher", "gt_center", "mask_gt", "fg", "gt_idx", "mixed")}, cfg


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", CASES)
def test_kernel_vs_restatement(name, dtype):
    """loss word, compact rows, their (image, anchor) index and the row count, case by case over the reference's fixture.  The teacher
    map alternates between NCHW fp32 and NHWC in the compute dtype."""
    y3d.set_compute_dtype(dtype)
    try:
        i, cfg = inputs(name)
        nhwc = CASES.index(name) % 2 == 1
        tdt = dtype if nhwc else torch.float32
        item, grad, rows, idx, counts = run_kernel(i, cfg, dtype, nhwc, tdt)
        ref_in = dict(i)
        if dtype == torch.bfloat16:  # the kernel sees rounded inputs: so does the restatement
            ref_in["emb"] = torch.from_numpy(i["emb"]).bfloat16().float().numpy()
        if tdt == torch.bfloat16:
            ref_in["teacher"] = torch.from_numpy(i["teacher"]).bfloat16().float().numpy()
        loss, g, ref_rows = DR.forward_head(ref_in["emb"], ref_in["teacher"], i["gt_center"], i["mask_gt"], i["fg"], i["gt_idx"], i["mixed"],
                                            tuple(Z["img_wh"]), cfg[2], float(Z["weight"]), DR.CRITERIA[int(cfg[1])], bool(cfg[3]))
        loss, g = loss / TSS, g / TSS
        B = i["fg"].shape[0]
        n = int(counts[B])
        print(f"{name} {dtype}: item {item:.7f} ref {loss:.7f} rel {abs(item - loss) / abs(loss):.2e}; rows {n}")
        assert n == len(ref_rows) == int(counts[B + 1]), "row count"
        assert [tuple(r) for r in idx[:n].tolist()] == ref_rows, "(image, anchor) index: the foreground set of the participating images, in order"
        part = [b for b in range(B) if i["mask_gt"][b].any() and not (cfg[3] and i["mixed"][b])]
        assert counts[:B].tolist() == [int(i["fg"][b].sum()) if b in part else 0 for b in range(B)]
        assert abs(item - loss) <= 1e-3 * abs(loss)
        ref_compact = np.stack([g[b, :, a] for b, a in ref_rows])
        if dtype == torch.float32:
            e = rel(rows[:n], ref_compact)
            print(f"   fp32 rows rel {e:.2e}")
            assert e <= 1e-3 and rel(grad, g) <= 1e-3
        else:
            bound = 2.0 ** -8 * np.abs(ref_compact).max(1, keepdims=True)
            worst = float((np.abs(rows[:n] - ref_compact) / bound).max())
            print(f"   bf16 rows: worst error / (2^-8 row max) = {worst:.3f}")
            assert worst <= 1.0
    finally:
        y3d.set_compute_dtype(torch.bfloat16)


def test_fully_mixed_batch_and_image_without_foreground():
    y3d.set_compute_dtype(torch.float32)
    try:
        i, cfg = inputs("soft_t2_nomix_c128")
        item, grad, _, _, counts = run_kernel(i, cfg, torch.float32, False, torch.float32, mixed=np.ones(4, bool))
        assert item == 0.0 and not grad.any() and counts[4] == 0
        # image 1 has an object but no foreground anchor: it contributes 0 (the reference: NaN), the others are unchanged
        i, cfg = inputs("cos_t2_mix_c128")
        fg = i["fg"].copy()
        fg[1] = False
        item, grad, _, _, counts = run_kernel(i, cfg, torch.float32, False, torch.float32, fg=fg)
        loss, g, rows = DR.forward_head(i["emb"], i["teacher"], i["gt_center"], i["mask_gt"], fg, i["gt_idx"], i["mixed"], tuple(Z["img_wh"]), cfg[2],
                                        float(Z["weight"]), "cos", False)
        assert np.isfinite(item) and abs(item - loss / TSS) <= 1e-3 * loss / TSS and counts[1] == 0 and not grad[1].any() and rel(grad, g / TSS) <= 1e-3
    finally:
        y3d.set_compute_dtype(torch.bfloat16)


def _crit(strides, **hyp):
    head = SimpleNamespace(stride=torch.tensor(strides), nc=3, no=38)
    return PL.DetectLoss3d(SimpleNamespace(model=[head], args=SimpleNamespace(**dict(y3d.tasks.DEFAULT_HYP, **hyp))))


@pytest.mark.parametrize("shared", [False, True], ids=["two_calls", "shared_maps"])
def test_detectloss3d_with_distillation_vs_reference_fixture(shared):
    """a whole reference DetectLoss3d call with `distillation: True` (stub teacher): the 14 items, the gradients wrt the head maps and
    the embeddings; items 0-5 of each set are the bits of the same call with distillation off.  `shared`: the head sets as channel
    halves of one map per level (the DualLoss3dFn path), else the two-call path."""
    y3d.set_compute_dtype(torch.float32)
    try:
        g, g0 = load_golden("loss3d_distill"), load_golden("loss3d")
        strides = [float(s) for s in g0["strides"]]
        T, w, crit, nomix = [float(v) for v in g["hyp"]]
        hyp = dict(distillation_temp=T, distillation_weight=w, distillation_loss=DR.CRITERIA[int(crit)], distillation_no_mixup=bool(nomix))
        H, W = [int(v) for v in g["img_hw"]]
        batch = {k: v.to(DEV) for k, v in g0["batch"].items()}
        batch["img"] = torch.zeros(g["teacher"].shape[0], 3, H, W, device=DEV)
        batch["teacher_emb"] = g["teacher"].to(DEV)
        res = {}
        for on in (True, False):
            c = _crit(strides, distillation=on, **hyp)
            if shared:
                bases = [ops._dense_any(torch.cat((a, b), 1).to(DEV), torch.float32).requires_grad_(True) for a, b in zip(g0["o2o"], g0["o2m"])]
                o2o, o2m = [t[:, :38] for t in bases], [t[:, 38:] for t in bases]
                leaves = bases
            else:
                o2m = [ops._dense_any(t.to(DEV), torch.float32).requires_grad_(True) for t in g0["o2m"]]
                o2o = [ops._dense_any(t.to(DEV), torch.float32).requires_grad_(True) for t in g0["o2o"]]
                leaves = o2m + o2o
            e_m = [ops._dense_any(t.to(DEV), torch.float32).requires_grad_(True) for t in g["e_o2m"]]
            e_o = [ops._dense_any(t.to(DEV), torch.float32).requires_grad_(True) for t in g["e_o2o"]]
            preds = {"one2many": o2m, "one2one": o2o, "o2m_embs": e_m, "o2o_embs": e_o}
            if shared:
                preds["_y3d_maps"] = bases
            loss, items = c(preds, batch)
            loss.backward()
            torch.cuda.synchronize()
            if shared:
                gm, go = [t.grad[:, 38:] for t in bases], [t.grad[:, :38] for t in bases]
            else:
                gm, go = [t.grad for t in o2m], [t.grad for t in o2o]
            res[on] = (loss.detach().cpu(), items.cpu(), gm, go, [t.grad for t in e_m], [t.grad for t in e_o])
        loss, items, gm, go, gem, geo = res[True]
        print("items", items.tolist(), "\nref  ", g["items"].tolist())
        assert items.numel() == 14 and rel(items.numpy(), g["items"].numpy()) <= 1e-3
        assert (np.abs(items.numpy() - g["items"].numpy()) <= 1e-3 * np.abs(g["items"].numpy()) + 1e-6).all()
        assert rel(loss.numpy(), g["loss"].numpy()) <= 1e-3
        it_off = res[False][1]
        assert it_off.numel() == 12 and torch.equal(items[0:6], it_off[0:6]) and torch.equal(items[7:13], it_off[6:12])
        for name, mine, ref in (("d/d o2m", gm, g["g_o2m"]), ("d/d o2o", go, g["g_o2o"]), ("d/d e_o2m", gem, g["ge_o2m"]), ("d/d e_o2o", geo, g["ge_o2o"])):
            for a, b in zip(mine, ref):
                e = rel(a.float().cpu().numpy(), b.numpy())
                print(f"{name}: {e:.2e}")
                assert e <= 1e-3, name
        assert all(t is None for t in res[False][4] + res[False][5]), "distillation off: the embeddings take no gradient"
    finally:
        y3d.set_compute_dtype(torch.bfloat16)


def graph_nodes(t):
    """names of the autograd nodes reachable from tensor t"""
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        todo += [n for n, _ in f.next_functions]
    return {type(f).__name__ for f in seen}


def _head(widths, dev=DEV):
    torch.manual_seed(7)
    chan = {k + "_c": widths[1] for k in ("o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")}
    chan["cls_c"] = widths[0]
    hd = M.v10Detect3d(3, (32, 64), False, chan, False, False, False, False, 2, False, False, 3, 3)
    hd.stride = torch.tensor([8.0, 16.0])
    hd.bias_init()  # plausible depths and sizes, so that both head sets find foreground anchors
    hd = hd.to(dev).train()
    with torch.no_grad():
        for p_ in hd.parameters():
            p_.add_(0.02 * torch.randn_like(p_))
    return hd


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_branch"])
@pytest.mark.parametrize("widths", [(64, 64), (128, 64)], ids=["uniform", "mixed_widths"])
def test_gradient_path_into_the_head(widths, fused):
    """(parameter and input gradients of a step with distillation on) - (those of the same step with it off) = the gradients obtained by
    back-propagating ONLY the restatement's embedding gradient through the head: the backward is linear in its upstream gradient for a
    fixed forward.  Fused head: the rows arrive through ops.InjectRowsFn (no dense gradient of z1's size); per-branch head: plain
    autograd.  Tolerance: that of test_hip_modules.test_head3d_bn_projection_fusion_matches_unfused in fp32 (3 x 2e-4 of the largest
    value, gradients below 1e-3 of the largest on that scale).  The distillation weight is raised so that the difference of the two
    steps stands well above the rounding of either."""
    from bench import synth_batch
    y3d.set_compute_dtype(torch.float32)
    try:
        hd = _head(widths)
        hd.fused = fused
        B, C = 3, widths[1]
        xs0 = [torch.randn(B, 32, 24, 24, device=DEV), torch.randn(B, 64, 12, 12, device=DEV)]
        batch = synth_batch(B, 192, 192, 5, DEV)
        batch["mixed"] = torch.tensor([0, 1, 0], dtype=torch.uint8, device=DEV)
        batch["teacher_emb"] = torch.randn(B, C, 7, 11, device=DEV)
        hyp = dict(distillation_temp=2.0, distillation_weight=200.0, distillation_loss="soft", distillation_no_mixup=True)
        res = {}
        for on in (True, False):
            hd.distill = False
            model = SimpleNamespace(model=[hd], args=SimpleNamespace(**dict(y3d.tasks.DEFAULT_HYP, distillation=on, **hyp)))
            crit = PL.DetectLoss3d(model)
            hd.zero_grad(set_to_none=True)
            xs = [x.clone().requires_grad_(True) for x in xs0]
            out = hd(xs)
            assert ("_y3d_distill" in out) == (on and fused)
            loss, items = crit(out, batch)
            nodes = graph_nodes(loss)
            assert any("InjectRows" in n for n in nodes) == (on and fused) and any("DistillFn" in n for n in nodes) == on, nodes
            if on and fused:  # the sparse path is taken: both head sets left their rows in every level's slot ...
                assert all(len(s.get("entries", ())) == 2 for s in out["_y3d_distill"]), "DetectLoss3d fell back to dense slice autograd"
            loss.backward()
            if on and fused:  # ... and InjectRowsFn's backward consumed them, with the scale DistillFn's backward had left
                assert all("entries" not in s for s in out["_y3d_distill"])
            res[on] = ({k: v.grad.float().clone() for k, v in hd.named_parameters() if v.grad is not None}, [x.grad.float().clone() for x in xs], items)
            if on:
                asg = [c.last_assignment for c in (crit.one2many, crit.one2one)]
                embs = [[e.detach().float().cpu() for e in out[k]] for k in ("o2m_embs", "o2o_embs")]
                gt, _ = crit.one2one.targets(batch, B, 24, 24, DEV)
        assert res[True][2].numel() == 14 and float(res[True][2][6]) > 0 and float(res[True][2][13]) > 0
        # the restatement's embedding gradient of both sets, scaled as the step scales it: (item / tss) * B
        gt = gt.cpu()
        ups = []
        for (fg, gi, ts), es in zip(asg, embs):
            emb = torch.cat([e.reshape(B, C, -1) for e in es], 2).numpy()
            _, ge, rows = DR.forward_head(emb, batch["teacher_emb"].cpu().numpy(), gt[..., 9:11].numpy(), (gt[..., 1:5].sum(-1) > 0).numpy(), fg.cpu().numpy(),
                                          gi.cpu().numpy(), batch["mixed"].cpu().numpy(), (192, 192), 2.0, 200.0, "soft", True)
            assert rows and all(b != 1 for b, _ in rows), "the mixed image takes no part"
            ge = torch.from_numpy(ge * B / max(float(ts.sum()), 1.0)).float()
            ups.append([ge[:, :, :576].reshape(B, C, 24, 24).to(DEV), ge[:, :, 576:].reshape(B, C, 12, 12).to(DEV)])
        hd.distill = False
        hd.zero_grad(set_to_none=True)
        xs = [x.clone().requires_grad_(True) for x in xs0]
        out = hd(xs)
        sum((e.float() * u).sum() for k, up in zip(("o2m_embs", "o2o_embs"), ups) for e, u in zip(out[k], up)).backward()
        ref_p = {k: v.grad.float() for k, v in hd.named_parameters() if v.grad is not None}
        ref_x = [x.grad.float() if x.grad is not None else torch.zeros_like(x) for x in xs]
        tol = 3 * 2e-4
        scale = max(float(v.abs().max()) for v in ref_p.values())
        floor = 1e-3 * scale
        worst = 0.0
        for k, gon in res[True][0].items():
            d = gon - res[False][0][k]
            r = ref_p.get(k, torch.zeros_like(d))
            e = float((d - r).abs().max() / max(float(r.abs().max()), floor))
            worst = max(worst, e)
            assert e <= tol, f"{k}: {e:.3e}"
        assert any(float(v.abs().max()) > 0 for k, v in ref_p.items()) and scale > 0
        for a, b0, r in zip(res[True][1], res[False][1], ref_x):
            e = float(((a - b0) - r).abs().max() / max(float(r.abs().max()), 1e-3 * max(float(t.abs().max()) for t in ref_x)))
            worst = max(worst, e)
            assert e <= tol, f"dx: {e:.3e}"
        print(f"widths {widths} fused {fused}: worst relative error of the gradient difference {worst:.3e}")
    finally:
        y3d.set_compute_dtype(torch.bfloat16)


def _one_step(prepare):
    """one full training step (forward, loss, backward, clip, optimizer step) of N-3D with `distillation: False` from a fixed seed
    -> (state_dict, momentum buffers, items, autograd node names, head output keys, the head's switch)"""
    from bench import synth_batch
    from yolov10_3d_amd.optim import build_optimizer
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(3)
    model = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()
    opt = build_optimizer(model, lr=0.01)
    head = model.model[-1]
    head.restack()
    prepare(model)
    batch = synth_batch(2, 256, 256, 20, DEV)
    preds = model.predict(batch["img"])
    loss, items = model.loss(batch, preds)
    nodes = graph_nodes(loss)
    loss.backward()
    opt.step(max_norm=10.0)
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in model.state_dict().items()}, opt.state.flat.clone(), items.clone(), nodes, set(preds), head.distill)


def test_distillation_off_leaves_the_step_as_it_was():
    """with `distillation: False` one full step gives the same bits - every parameter, BatchNorm buffer and momentum word, and the 12
    items - whether or not the new code was ever reachable: on an untouched model; after a distillation-on criterion was built on
    the model and replaced by an off one (the head's switch goes back); and with the head's switch forced on under the off criterion
    (InjectRowsFn in the graph, nothing for it to add).  In the first two the graph holds no node of the feature and the head makes
    no slot."""
    def untouched(model):
        pass

    def built_and_replaced(model):
        model.args.distillation = True
        model.criterion = model.init_criterion()
        assert model.model[-1].distill is True
        model.args.distillation = False
        model.criterion = model.init_criterion()

    def forced(model):
        model.criterion = model.init_criterion()
        model.model[-1].distill = True

    ref = _one_step(untouched)
    assert ref[2].numel() == 12 and not hasattr(PL, "_SCAL_TAP") and ref[5] is False
    assert not any("InjectRows" in n or "Distill" in n for n in ref[3]) and "_y3d_distill" not in ref[4]
    assert float(ref[1].float().abs().max()) > 0, "the step moved nothing: the comparison would be empty"
    for prepare in (built_and_replaced, forced):
        got = _one_step(prepare)
        assert not hasattr(PL, "_SCAL_TAP") and not any("Distill" in n for n in got[3])
        if prepare is built_and_replaced:
            assert got[5] is False and not any("InjectRows" in n for n in got[3]) and "_y3d_distill" not in got[4]
        else:
            assert any("InjectRows" in n for n in got[3]) and "_y3d_distill" in got[4]
        assert torch.equal(got[2], ref[2]), f"{prepare.__name__}: loss items differ"
        for k, v in ref[0].items():
            assert torch.equal(v, got[0][k]), f"{prepare.__name__}: state {k} differs after one step"
        assert torch.equal(got[1], ref[1]), f"{prepare.__name__}: momentum buffers differ"


def test_teacher_errors():
    from bench import synth_batch
    y3d.set_compute_dtype(torch.bfloat16)
    hd = _head((64, 64))
    model = SimpleNamespace(model=[hd], args=SimpleNamespace(**dict(y3d.tasks.DEFAULT_HYP, distillation=True)))
    crit = PL.DetectLoss3d(model)
    batch = synth_batch(2, 192, 192, 5, DEV)
    batch["mixed"] = torch.zeros(2, dtype=torch.uint8, device=DEV)
    xs = [torch.randn(2, 32, 24, 24, device=DEV), torch.randn(2, 64, 12, 12, device=DEV)]
    prev = PL.set_teacher(None)
    try:
        with pytest.raises(y3d.Y3DError, match=r"teacher_emb.*set_teacher"):
            crit(hd(xs), batch)
        with pytest.raises(ValueError, match=r"32 channels.*64 wide"):
            crit(hd(xs), dict(batch, teacher_emb=torch.zeros(2, 32, 4, 4, device=DEV)))
        with pytest.raises(y3d.Y3DError, match="HIP device"):
            crit(hd(xs), dict(batch, teacher_emb=torch.zeros(2, 64, 4, 4)))
        with pytest.raises(ValueError, match=r"holds 1 images, the batch 2"):  # a stale map after a short batch must not be read out of bounds
            crit(hd(xs), dict(batch, teacher_emb=torch.zeros(1, 64, 4, 4, device=DEV)))
        with pytest.raises(ValueError, match=r"3 `mixed` flags for 2 images"):
            crit(hd(xs), dict(batch, teacher_emb=torch.zeros(2, 64, 4, 4, device=DEV), mixed=torch.zeros(3, dtype=torch.uint8, device=DEV)))
        calls = []
        PL.set_teacher(lambda img: (calls.append(img.shape) or None, torch.randn(img.shape[0], 64, 6, 6, device=DEV)))
        loss, items = crit(hd(xs), batch)
        assert len(calls) == 1 and items.numel() == 14 and bool(torch.isfinite(items).all())  # one call per step, shared by both head sets
        # a batch without boxes: zeros(7) per set
        empty = {k: (v[:0] if k in ("batch_idx", "cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res") else v)
                 for k, v in batch.items()}
        _, it = crit.one2one(hd(xs)["one2one"], empty, embeddings=None)
        assert it.numel() == 7 and not it.any()
    finally:
        PL.set_teacher(prev)


def test_graphed_train_step_with_teacher_map_replays_the_eager_step():
    """graph.GraphedTrainStep with `teacher_emb` in the batch: two steps on two different batches leave parameters, BatchNorm statistics,
    momentum buffers and the 14 loss items where two eager steps leave them, bit for bit (no float atomic reaches the loss or the
    gradient)"""
    from bench import synth_batch
    from yolov10_3d_amd.graph import GraphedTrainStep
    from yolov10_3d_amd.optim import build_optimizer
    y3d.set_compute_dtype(torch.bfloat16)
    batches = [synth_batch(2, 256, 256, 20 + j, DEV) for j in range(2)]
    for j, b in enumerate(batches):
        g = torch.Generator().manual_seed(50 + j)
        b["mixed"] = torch.tensor([j, 0], dtype=torch.uint8, device=DEV)
        b["teacher_emb"] = torch.randn(2, 128, 9, 9, generator=g).to(DEV)
    res = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(3)
        model = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()
        model.args.distillation = True
        opt = build_optimizer(model, lr=0.01)
        model.model[-1].restack()
        items = []
        if mode == "eager":
            for b in batches:
                loss, it = model(b)
                loss.backward()
                opt.step(max_norm=10.0)
                opt.zero_grad()
                items.append(it.float().cpu())
        else:
            step = GraphedTrainStep(model, opt, batches[0])
            for b in batches:
                loss, it = step(b)
                items.append(it.float().cpu().clone())
        torch.cuda.synchronize()
        res[mode] = (items, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone())
        del loss
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert a.numel() == 14 and float(a[6]) > 0 and torch.equal(a, b), (a, b)
    for k, v in res["eager"][1].items():
        assert torch.equal(v, res["graph"][1][k]), f"state {k} differs after two steps"
    assert torch.equal(res["eager"][2], res["graph"][2]), "momentum buffers differ"


def test_graphed_train_step_with_registered_teacher_replays_the_eager_step():
    """graph.GraphedTrainStep with a teacher callable registered and no `teacher_emb` in the batch: the callable runs outside the captured
    graph, once before every replay, on that replay's images; two steps on two batches end where two eager steps end, bit for bit.
    The step keeps the callable it was built with: un-registering it afterwards does not break the replays."""
    from bench import synth_batch
    from yolov10_3d_amd.graph import GraphedTrainStep
    from yolov10_3d_amd.optim import build_optimizer
    y3d.set_compute_dtype(torch.bfloat16)
    batches = [synth_batch(2, 256, 256, 30 + j, DEV) for j in range(2)]
    for j, b in enumerate(batches):
        b["mixed"] = torch.tensor([0, j], dtype=torch.uint8, device=DEV)
    proj = torch.randn(128, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    calls = []

    def teacher(img):  # a deterministic function of the images: (depth_maps, embeddings)
        calls.append(1)
        pooled = torch.nn.functional.adaptive_avg_pool2d(img.float(), (6, 10))
        return None, torch.einsum("cj,bjhw->bchw", proj, pooled).contiguous() * 8.0

    prev = PL.set_teacher(teacher)
    try:
        res = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(3)
            model = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()
            model.args.distillation = True
            opt = build_optimizer(model, lr=0.01)
            model.model[-1].restack()
            items = []
            if mode == "eager":
                for b in batches:
                    n0 = len(calls)
                    loss, it = model(b)
                    assert len(calls) == n0 + 1, "one teacher call per step, shared by both head sets"
                    loss.backward()
                    opt.step(max_norm=10.0)
                    opt.zero_grad()
                    items.append(it.float().cpu())
            else:
                step = GraphedTrainStep(model, opt, batches[0])
                assert "teacher_emb" in step.static and step.teacher_fn is teacher
                PL.set_teacher(None)  # the step holds its own reference
                for b in batches:
                    n0 = len(calls)
                    loss, it = step(b)
                    assert len(calls) == n0 + 1, "the teacher runs once per replay, outside the graph"
                    items.append(it.float().cpu().clone())
            torch.cuda.synchronize()
            res[mode] = (items, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone())
            del loss
        for a, b in zip(res["eager"][0], res["graph"][0]):
            assert a.numel() == 14 and float(a[6]) > 0 and torch.equal(a, b), (a, b)
        assert not torch.equal(res["eager"][0][0], res["eager"][0][1])
        for k, v in res["eager"][1].items():
            assert torch.equal(v, res["graph"][1][k]), f"state {k} differs after two steps"
        assert torch.equal(res["eager"][2], res["graph"][2]), "momentum buffers differ"
    finally:
        PL.set_teacher(prev)


def test_teacher_layouts_the_vector_loads_cannot_take():
    """a contiguous NCHW teacher map of 1 x 1 pixels has a channel stride of 1 without being an aligned channel-last map, and a
    channel-last view may have strides that are no multiples of 4: both are served by the strided loads"""
    y3d.set_compute_dtype(torch.float32)
    try:
        i, cfg = inputs("mse_t1_mix_c64")
        i = dict(i)
        i["teacher"] = np.ascontiguousarray(i["teacher"][:, :, 2:3, 5:6])
        item, grad, _, _, _ = run_kernel(i, cfg, torch.float32, False, torch.float32)
        loss, g, _ = DR.forward_head(i["emb"], i["teacher"], i["gt_center"], i["mask_gt"], i["fg"], i["gt_idx"], i["mixed"], tuple(Z["img_wh"]), cfg[2],
                                     float(Z["weight"]), "mse", False)
        assert abs(item - loss / TSS) <= 1e-3 * loss / TSS and rel(grad, g / TSS) <= 1e-3
        # channel-last storage with a 6-element tail per pixel: unit channel stride, pixel stride 70
        i, cfg = inputs("mse_t1_mix_c64")
        t = torch.from_numpy(i["teacher"])
        B, C, h, w = t.shape
        store = torch.zeros(B, h, w, C + 6)
        store[..., :C] = t.permute(0, 2, 3, 1)
        view = store.to(DEV)[..., :C].permute(0, 3, 1, 2)
        assert view.stride(1) == 1 and view.stride(3) % 4 != 0
        embs = [e.requires_grad_(True) for e in levels_of(torch.from_numpy(i["emb"]), torch.float32)]
        Bf, A = i["fg"].shape
        spec = dict(embs=[e.detach() for e in embs], teacher=view, gt=padded_gt(i["gt_center"], i["mask_gt"]),
                    fg=torch.from_numpy(i["fg"]).to(DEV).to(torch.uint8), gi=torch.from_numpy(i["gt_idx"]).to(DEV).int(),
                    scal=torch.tensor([TSS, 0.0], device=DEV), mixed=torch.from_numpy(i["mixed"]).to(DEV).to(torch.uint8),
                    img_wh=tuple(int(v) for v in Z["img_wh"]), T=cfg[2], weight=float(Z["weight"]), crit=1, no_mixup=False, cap=Bf * A, slots=None, which=0)
        item = float(PL.DistillFn.apply(spec, *embs).detach())
        loss, _, _ = DR.forward_head(i["emb"], i["teacher"], i["gt_center"], i["mask_gt"], i["fg"], i["gt_idx"], i["mixed"], tuple(Z["img_wh"]), cfg[2],
                                     float(Z["weight"]), "mse", False)
        assert abs(item - loss / TSS) <= 1e-3 * loss / TSS
    finally:
        y3d.set_compute_dtype(torch.bfloat16)
