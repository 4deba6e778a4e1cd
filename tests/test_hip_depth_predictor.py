"""GPU: modules.DepthPredictor end to end against the float64 restatement and the reference's recorded results
(tests/depth_predictor_ref.py, tests/golden/depth_predictor.npz), and its wiring into the 3D head, DetectLoss3d and train.Trainer.

Tolerances.  The constants below are yardsticks measured on the CPU by tests/test_depth_predictor_ref_host.py
(test_tolerance_constants_cover_the_yardsticks; one thread), max |a - ref| / max |ref| over the three cases, forward tensors (logits,
features, weighted_depth) and gradients apart: for float32 the restated module run in torch float32 against its float64 run, for bfloat16
the restatement that rounds every tensor the device stores in bfloat16 against float64.  The device may sum in another, equally valid
order: it is allowed four times the yardstick (the factor of tests/test_hip_fgdm_loss.py), not another algorithm.  The bfloat16 gradient
yardstick is large because the cotangent is white noise: the gradients are sums with heavy cancellation, and a ReLU mask that flips
under rounding moves them by whole terms.  The float32 sums of the CPU kernels depend on the CPU they run on (vector width, blocking), so
the float32 yardstick is not one number: measured with one thread on the two kinds of machine this suite runs on it was 5.008e-7 /
2.320e-6 and 4.790e-7 / 2.393e-6 (forward / gradients); the constants are the larger of each, the bfloat16 ones (float64 arithmetic and
explicit roundings: 5.969e-3 / 1.887e-1 on both) as measured."""
import os

import numpy as np
import pytest
import torch

from conftest import has_gpu

import depth_predictor_ref as R

F32_OUT_DIST, F32_GRAD_DIST = 5.01e-7, 2.40e-6
BF16_OUT_DIST, BF16_GRAD_DIST = 5.97e-3, 1.89e-1
FACTOR = 4

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a HIP device")]
DEV = "cuda"
RES = (320, 256)
FIT = dict(epochs=2, batch=2, nbs=4, warmup_epochs=0, optimizer="SGD", lr0=0.01)


@pytest.fixture(autouse=True)
def _bf16_after():
    import yolov10_3d_amd as y3d
    yield
    y3d.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def refs():
    """per case: parameters, inputs and the float64 restatement on the float32 inputs and on their bfloat16 rounding; computed once"""
    from yolov10_3d_amd import modules as M
    out = {}
    for case in R.CASES:
        torch.manual_seed(R.SEED)
        sd = R.redraw_affine(M.DepthPredictor(case["ch"])).state_dict()
        feats, cot = R.case_inputs(case)
        out[case["name"]] = (sd, feats, cot, {torch.float32: R.run(sd, feats, cot), torch.bfloat16: R.run(sd, [R.bf16(f) for f in feats], R.bf16(cot))})
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c["name"] for c in R.CASES])
def test_end_to_end(case, dtype, refs):
    import yolov10_3d_amd as y3d
    from yolov10_3d_amd import modules as M, ops
    y3d.set_compute_dtype(dtype)
    sd, feats, cot, ref = refs[case["name"]]
    ref = ref[dtype]
    m = M.DepthPredictor(case["ch"])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    x = [ops.to_nhwc(f.to(DEV), dtype).requires_grad_(True) for f in feats]
    logits, weighted, features = m(x, return_embeddings=True)
    assert logits.shape == (case["B"], 81, *case["p4"]) and weighted.shape == (case["B"], *case["p4"]) and features.shape == (case["B"], 128, *case["p4"])
    assert logits.dtype == dtype and weighted.dtype == torch.float32 and not weighted.requires_grad
    assert len(m(x)) == 2
    (logits.float() * cot.to(DEV).to(dtype).float()).sum().backward()
    torch.cuda.synchronize()
    got = {"logits": logits, "features": features, "weighted_depth": weighted}
    got.update({f"d_feat{i}": t.grad for i, t in enumerate(x)})
    got.update({f"d_{k}": p.grad for k, p in m.named_parameters() if p.requires_grad})
    assert set(got) == set(ref) and m.depth_bin_values.grad is None
    out_tol, grad_tol = ((F32_OUT_DIST, F32_GRAD_DIST) if dtype == torch.float32 else (BF16_OUT_DIST, BF16_GRAD_DIST))
    z = np.load(R.GOLDEN)
    bad = []
    for k, r in ref.items():
        g = got[k].detach().float().cpu().double().numpy()
        assert g.shape == tuple(r.shape) and np.isfinite(g).all(), k
        tol = FACTOR * (grad_tol if k.startswith("d_") else out_tol)
        d = R.rel_max(g, r.numpy())
        # the reference's own float32 run (the fixture's samples) is one float32 yardstick away from float64 itself
        dfix = R.rel_max(R.sample(g), z[f"{case['name']}/{k}/sample"])
        fix_tol = tol + (F32_GRAD_DIST if k.startswith("d_") else F32_OUT_DIST)
        print(f"{case['name']} {dtype} {k}: restatement {d:.3e} (bound {tol:.3e}), fixture {dfix:.3e} (bound {fix_tol:.3e})")
        if d > tol or dfix > fix_tol:
            bad.append((k, d, dfix))
    assert not bad, bad
    # the classifier's pad columns: zero logits, and no gradient into the padded weight rows the module keeps
    base = logits._base
    assert base is not None and base.shape[-1] == 88 and not base[..., 81:].any()  # the (B, h, w, 88) buffer
    wpad, bpad = m._pads(logits.device)
    assert wpad.shape[0] == 88 and not wpad[81:].any() and not bpad[81:].any()
    assert m.depth_classifier.weight.grad.shape == (81, 128, 1, 1)


def test_host_tensors_are_refused():
    from yolov10_3d_amd import modules as M
    from yolov10_3d_amd._lib import Y3DError
    m = M.DepthPredictor((8, 8, 8)).to(DEV)
    with pytest.raises(Y3DError, match="no CPU fallback"):
        m([torch.zeros(1, 8, 8, 8), torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 2, 2)])


# ---- wiring: head, loss, trainer ---------------------------------------------------------------------------------------------------
def new_model(fgdm, seed=3):
    import yolov10_3d_amd as y3d
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(seed)
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    cfg["fgdm_predictor"] = bool(fgdm)
    model = y3d.YOLOv10_3DDetectionModel(cfg).to(DEV).train()
    model.args.fgdm_loss = bool(fgdm)
    model.model[-1].restack()
    return model


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from kitti_labels_tree import fixture, write_tree
    from test_hip_depth_map import write_masks
    from yolov10_3d_amd import kitti
    z = fixture()
    z4 = {k: z[k][:4] for k in ("label_text", "calib_text", "frame_wh")}
    root = write_tree(str(tmp_path_factory.mktemp("fgdm_tree")), z4, images=True)
    write_masks(root, z4)
    return kitti.DeviceSplit(root, device=DEV, load_depth_maps=True)


def one_batch(tree):
    from yolov10_3d_amd import kitti
    b = next(iter(tree.epoch(2, kitti.data_args(load_depth_maps=True), mode="train", shuffle=True, seed=0, resolution=RES)))
    return dict(b, img=b["img"].permute(0, 3, 1, 2))


def step(model, batch, taps=None):
    """loss, items and gradients of one step; `taps`: also the head's input maps (with their gradients) and the predictor's logits"""
    model.zero_grad(set_to_none=True)
    seen, hooks = {}, []
    head = model.model[-1]
    if taps:
        def pre(mod, args):
            xs = list(args[0])
            for t in xs:
                t.retain_grad()
            seen["x"] = xs
        hooks.append(head.register_forward_pre_hook(pre))
        if getattr(head, "fgdm_pred", False):
            hooks.append(head.fgdm_predictor.register_forward_hook(lambda mod, a, out: seen.__setitem__("logits", out[0])))
    if hasattr(model, "criterion"):
        del model.criterion
    loss, items = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}
    return loss.detach(), items.detach(), grads, seen


def test_loss_items_and_gradients(tree):
    from yolov10_3d_amd import loss as PL
    batch = one_batch(tree)
    assert batch["depth_map"].shape == (2, RES[1], RES[0])
    on = new_model(True)
    off = new_model(False, seed=4)
    off.load_state_dict({k: v for k, v in on.state_dict().items() if ".fgdm_predictor." not in k}, strict=True)
    off.model[-1].restack()
    l1, i1, g1, s1 = step(on, batch, taps=True)
    l0, i0, g0, s0 = step(off, batch, taps=True)
    assert i0.numel() == 12 and i1.numel() == 13 and PL.loss_names(on.args)[-1] == "fgdm" and torch.equal(i1[:12], i0)
    logits = s1["logits"]
    assert logits.shape == (2, 81, RES[1] // 16, RES[0] // 16)
    f = PL.ForegroundDepthMapLoss(on)(logits.detach(), batch["depth_map"]) * 2.0
    assert torch.equal(l1, l0 + f) and torch.equal(i1[12], f) and float(f) > 0, "total = switch-off total + 2 * fgdm, not times B"
    for k, g in g1.items():
        if ".fgdm_predictor." in k and "depth_bin_values" not in k:
            assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, k
    assert g1[[k for k in g1 if k.endswith("depth_bin_values")][0]] is None
    # the neck maps get the predictor's gradient on top of the head's: the head's own parameters see the same gradient either way ...
    head_keys = [k for k in g0 if k.startswith(f"model.{len(on.model) - 1}.")]
    assert head_keys and all(torch.equal(g1[k], g0[k]) for k in head_keys)
    # ... and every level map's gradient is the switch-off one plus the predictor's (one bfloat16 rounding of the sum apart)
    on.zero_grad(set_to_none=True)
    xs = [x.detach().requires_grad_(True) for x in s1["x"]]
    lg = on.model[-1].fgdm_predictor(xs)[0]
    (PL.ForegroundDepthMapLoss(on)(lg, batch["depth_map"]) * 2.0).backward()
    for x1, x0, xp in zip(s1["x"], s0["x"], xs):
        assert xp.grad is not None and xp.grad.abs().max() > 0
        want = x0.grad.float() + xp.grad.float()
        assert (x1.grad.float() - want).abs().max() <= 2.0 ** -7 * want.abs().max(), "head gradient + predictor gradient"
        assert not torch.equal(x1.grad, x0.grad)


def test_switches_off_change_nothing(tree):
    """a head built with the predictor but switched off, and the loss without fgdm_loss, make the results of a model without it, bit for bit"""
    batch = one_batch(tree)
    on = new_model(True)
    off = new_model(False, seed=4)
    off.load_state_dict({k: v for k, v in on.state_dict().items() if ".fgdm_predictor." not in k}, strict=True)
    off.model[-1].restack()
    on.model[-1].fgdm_pred = False
    on.args.fgdm_loss = False
    l1, i1, g1, _ = step(on, batch)
    l0, i0, g0, _ = step(off, batch)
    assert torch.equal(l1, l0) and torch.equal(i1, i0) and i0.numel() == 12
    assert all(torch.equal(g1[k], g0[k]) for k in g0)
    assert all(g1[k] is None for k in g1 if ".fgdm_predictor." in k)


class Interrupted(Exception):
    pass


class Split320:
    def __init__(self, sp, stop_at=None):
        self.sp, self.stop_at = sp, stop_at

    def __len__(self):
        return len(self.sp)

    def epoch(self, batch, args, shuffle=True, seed=0):
        if seed == self.stop_at:
            raise Interrupted()
        return self.sp.epoch(batch, args, mode="train", shuffle=shuffle, seed=seed, resolution=RES)


def run_state(t):
    torch.cuda.synchronize()
    return {"model": {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()},
            "ema": {k: v.detach().cpu().clone() for k, v in t.ema.ema.state_dict().items()},
            "opt": t.opt.state.flat.cpu().clone(), "history": [dict(h) for h in t.history]}


def same_run(a, b, what):
    for part in ("model", "ema"):
        for k, v in a[part].items():
            assert torch.equal(v, b[part][k]), f"{what}: {part} {k} differs"
    assert torch.equal(a["opt"], b["opt"]) and a["history"] == b["history"], what


def test_trainer_two_epochs(tree, tmp_path):
    from yolov10_3d_amd import kitti, train
    args = lambda: kitti.data_args(load_depth_maps=True)  # noqa: E731
    save_dir = str(tmp_path / "straight")
    t = train.Trainer(new_model(True), Split320(tree), None, save_dir=save_dir, data_args=args(), **FIT)
    start = {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()}
    t.fit()
    a = run_state(t)
    assert len(a["history"]) == 2 and all("fgdm" in h and np.isfinite(h["fgdm"]) and h["fgdm"] > 0 for h in a["history"])
    assert list(a["history"][0])[1:14] == t.names and t.names[-1] == "fgdm"
    assert "train/fgdm" in open(os.path.join(save_dir, "results.csv")).readline()
    moved = [k for k in start if ".fgdm_predictor." in k and not torch.equal(start[k], a["model"][k])]
    frozen = [k for k in start if k.endswith("depth_bin_values")]
    # (a GroupNorm weight starts at exactly 1 and a two-step update below half an ulp of 1 leaves it there: those five are not asked to
    # move; their gradients are checked in test_loss_items_and_gradients)
    must = [k for k in start if ".fgdm_predictor." in k and not k.endswith(("depth_bin_values", ".1.weight", ".4.weight"))]
    assert len(must) == 17 and set(must) <= set(moved), sorted(set(must) - set(moved))
    assert torch.equal(start[frozen[0]], a["model"][frozen[0]]), "the bin values are frozen"
    # the EMA walks every floating-point state_dict tensor, as the reference's does: e * d + (1 - d) * m of a constant is the constant up
    # to the rounding of the two products
    assert torch.allclose(a["ema"][frozen[0]], start[frozen[0]], rtol=4 * 2.0 ** -23, atol=0) and not torch.equal(a["ema"][moved[0]], start[moved[0]])
    t2 = train.Trainer(new_model(True), Split320(tree), None, data_args=args(), **FIT)
    t2.fit()
    same_run(run_state(t2), a, "second run against the first")
    # interrupted before epoch 1, resumed from the file
    sd = str(tmp_path / "interrupted")
    t3 = train.Trainer(new_model(True), Split320(tree, stop_at=1), None, save_dir=sd, data_args=args(), **FIT)
    with pytest.raises(Interrupted):
        t3.fit()
    t4 = train.Trainer(new_model(True, seed=11), Split320(tree), None, resume=os.path.join(sd, "weights", "last.pt"), data_args=args(), **FIT)
    assert t4.start_epoch == 1
    t4.fit()
    same_run(run_state(t4), a, "resumed against straight")
