"""Host: the float64 loss reference and the case table of tests/loss_ref.py, without a GPU.

* `loss3d_terms` / `loss2d_terms`, fed the oracle's own assignment, reproduce `restate.loss3d_one` / `loss2d_one` (items and autograd
  gradients) on both golden fixtures to fp32 rounding: the new reference is tied to the one that is tied to the upstream project;
* every (case, dtype) of the table clears the assignment margin `MARGIN_FLOOR` on the oracle's metrics, its deciding metrics differ from
  float64 by no more than `METRIC_ROUNDING` (the measurement the floor is 16 x of), and it really contains what it is in the table for;
* the zero-foreground divergence of the 3D loss is pinned: NaN upstream in items 0 and 3, zero here and on the device."""
import pytest
import torch

import loss_ref as LR
from conftest import load_golden
from oracle import restate as RS  # the checker


def _fixture_case(fam, g, topk):
    strides = tuple(float(s) for s in g["strides"])
    H, W = g["o2m"][0].shape[2:]
    nc = g["o2m"][0].shape[1] - (35 if fam == "3d" else 64)
    return dict(name=f"golden_{fam}", fam=fam, hw=(int(H * strides[0]), int(W * strides[0])), strides=strides, nc=nc, topk=topk, gains=None,
                mode="default", boxes=None, edit=None, seed=0)


@pytest.mark.parametrize("fam,key,topk", [("3d", "o2m", 8), ("3d", "o2o", 1), ("2d", "o2m", 10), ("2d", "o2o", 1)])
def test_terms_reproduce_restate_on_the_golden_fixtures(fam, key, topk):
    g = load_golden("loss3d" if fam == "3d" else "loss2d")
    case = _fixture_case(fam, g, topk)
    maps, batch = [t.float() for t in g[key]], g["batch"]
    B = maps[0].shape[0]
    items32, grads32, aux = LR.restate_run(case, maps, batch)
    a = LR.assign(case, maps, batch, B)
    assert torch.equal(a["fg"], aux["fg_mask"]) and torch.equal(a["gt_idx"], aux["target_gt_idx"]) and a["fg"].any()
    if "target_scores" in aux:
        assert torch.equal(a["t_sc"], aux["target_scores"])
    items64, grads64 = LR.reference(case, maps, (a["fg"], a["gt_idx"], a["t_sc"]), a["gpad"])
    err = float(((items32.double() - items64).abs() / items64.abs()).max())
    groups = LR.groups3d(case["nc"]) if fam == "3d" else LR.groups2d(case["nc"])
    gerr = max(e for e, _ in LR.group_errors(grads32, grads64, groups).values())
    print(f"{fam} {key}: items {err:.2e}, gradient groups {gerr:.2e}")
    assert err < 2e-6 and gerr < 2e-5  # fp32 rounding of sums over ~1e3 anchors / of one element chain


RESTATE_ERR = {}


@pytest.mark.parametrize("name,dname", LR.case_ids(), ids=[f"{n}-{d}" for n, d in LR.case_ids()])
def test_case_clears_the_margin_and_holds_what_it_is_there_for(name, dname):
    case = LR.BY_NAME[name]
    fam, nc, topk = case["fam"], case["nc"], case["topk"]
    H, W = case["hw"]
    batch, B = LR.make_batch(case)
    maps = LR.make_maps(case, LR.DTYPES[dname])
    a = LR.assign(case, maps, batch, B)
    fg, gi = a["fg"], a["gt_idx"]
    # the metrics restated in loss_ref are the oracle's: its top-k and conflict rules on them give its assignment
    fg2, gi2, multi = LR.replay(a["align"], a["second"], a["gmask"], a["mask_gt"], topk)
    assert torch.equal(fg2, fg) and torch.equal(gi2, gi)
    a64, s64 = LR.metrics64(case, maps, batch, a)
    ga, gb, ties = LR.assignment_margin(a["align"], a["second"], a["mask_gt"], topk, a["gmask"], a["twins"])
    ma = float(ga.min()) if ga.numel() else float("inf")
    mb = float(gb.min()) if gb.numel() else float("inf")
    shapes, strides = LR.level_shapes(case["hw"], case["strides"]), list(case["strides"])
    cat = LR.flatten(maps)
    rnd = LR.metric_rounding(a["align"], a["second"], a64, s64, a["mask_gt"], topk, a["gmask"])
    print(f"{name}[{dname}]: fg {int(fg.sum())}, multiply selected {int((multi > 1).sum())} (exact ties {ties}), gaps top-k {ma:.2e} conflict {mb:.2e}, "
          f"fp32 vs float64 metric {rnd:.2e}")
    assert rnd <= LR.METRIC_ROUNDING, "the floor was derived from a smaller rounding difference than this case shows"
    assert min(ma, mb) > LR.MARGIN_FLOOR, "a decision of this case is closer to a tie than host and device arithmetic may differ: take another seed"
    # ---- what the case is in the table for ----
    gpad, box = a["gpad"], a["gpad"][..., 1:5]
    A = fg.shape[1]
    assert A == sum(h * w for h, w in shapes) and len(maps) == len(strides)
    labels = batch["cls"].view(-1).long()
    assert set(labels.tolist()) == set(range(min(nc, labels.numel()))) or nc > labels.numel()
    owns = lambda b, r: bool((fg[b] & (gi[b] == r)).any())  # noqa: E731
    if case["boxes"] == "no_fg":
        assert not fg.any() and a["mask_gt"].sum() == 3 and not a["gmask"].any()
    else:
        assert fg.any()
    if case["boxes"] == "tiny":
        assert box[0, 0, 2] - box[0, 0, 0] < 2.01 and not a["gmask"][0, 0].any() and not owns(0, 0)
        assert all(owns(b, r) for b in range(B) for r in range(gpad.shape[1]) if a["mask_gt"][b, r] and (b, r) != (0, 0))
    if case["boxes"] == "empty_image":
        assert B == 3 and not a["mask_gt"][1].any() and not fg[1].any() and fg[0].any() and fg[2].any()
    if case["boxes"] == "capacity":
        assert gpad.shape[1] == 64 and a["mask_gt"][0].all() and a["mask_gt"][1].sum() == 1
    if case["boxes"] == "border":
        assert (box[..., 0] < 0).any() and (box[..., 3] > H).any()
    if case["boxes"] == "dup_nested":
        assert torch.equal(gpad[0, 0, 1:], gpad[0, 1, 1:]) and gpad[0, 0, 0] != gpad[0, 1, 0] and (multi > 1).any()
        if fam == "2d" or case["mode"] == "box_only":
            assert ties > 0, "duplicated rows are meant to tie exactly in the conflict resolution"
    if "hires" in name:
        assert A * 4 > 96 * 1024
    if case["edit"] == "saturate":
        cls = cat[..., :nc] if fam == "3d" else cat[..., 64:]
        assert float(cls.abs().max()) == 30.0 and (fam == "2d" or float(cat[..., nc + 9:nc + 21].abs().max()) == 30.0)
    if fam == "2d":
        anc, st = LR.anchors(shapes, strides)
        t_box = LR._take(gpad, gi)[..., 1:5] / st
        ltrb = torch.cat((anc - t_box[..., :2], t_box[..., 2:] - anc), -1)[fg]
        d = cat[..., :64].view(B, A, 4, 16).softmax(3).matmul(torch.arange(16.0))
        pb = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)[fg]
        tb = t_box[fg]
        p_in_t = (pb[:, :2] > tb[:, :2]).all(1) & (pb[:, 2:] < tb[:, 2:]).all(1)
        t_in_p = (pb[:, :2] < tb[:, :2]).all(1) & (pb[:, 2:] > tb[:, 2:]).all(1)
        if case["edit"] == "dfl_clamp":
            assert (ltrb > 15 - 0.01).any(), "no foreground anchor has a clamped DFL target"
        if case["edit"] == ("tilt", -0.6):
            assert p_in_t.any()
        if case["edit"] == ("tilt", 0.6):
            assert t_in_p.any()
        if name == "l2_nc3_k10":
            assert (~p_in_t & ~t_in_p).any()
    # ---- restate's fp32 host gradient against the float64 reference (the figure a tighter fp32 bound would be derived from) ----
    if case["mode"] == "default" and not (fam == "3d" and case["boxes"] == "no_fg") and dname == "fp32":
        items32, grads32, _ = LR.restate_run(case, maps, batch)
        items64, grads64 = LR.reference(case, maps, (fg, gi, a["t_sc"]), gpad)
        groups = LR.groups3d(nc) if fam == "3d" else LR.groups2d(nc)
        gerr = max(e for e, _ in LR.group_errors(grads32, grads64, groups).values())
        ierr = float(((items32.double() - items64).abs() / items64.abs().clamp(min=1e-30)).max())
        RESTATE_ERR[name] = gerr
        print(f"{name}: restate fp32 vs float64: items {ierr:.2e}, gradient groups {gerr:.2e} (largest so far {max(RESTATE_ERR.values()):.2e})")
        assert ierr < 1e-5 and gerr < 1e-4


def test_zero_foreground_divergence_is_pinned():
    """boxes but no foreground anchor: upstream (and `restate.loss3d_one`) give NaN in items 0 and 3 ("mean" L1 of empty tensors); the HIP
    kernel and `loss3d_terms` give 0 there and agree with upstream in the other four.  The 2D loss has the guard: [0, bce, 0] everywhere."""
    case = LR.BY_NAME["l3_no_fg"]
    batch, B = LR.make_batch(case)
    maps = LR.make_maps(case)
    a = LR.assign(case, maps, batch, B)
    _, items32, aux = RS.loss3d_one(maps, batch, list(case["strides"]), case["nc"], case["topk"])
    assert not aux["fg_mask"].any()
    assert torch.isnan(items32).tolist() == [True, False, False, True, False, False]
    items64, grads64 = LR.reference(case, maps, (a["fg"], a["gt_idx"], a["t_sc"]), a["gpad"])
    assert items64[0] == 0 and items64[3] == 0 and items64[1] > 0
    keep = [1, 2, 4, 5]
    assert torch.allclose(items32[keep].double(), items64[keep], rtol=1e-5, atol=0)
    assert all(not g[:, case["nc"]:].any() for g in grads64)
    case2 = LR.BY_NAME["l2_no_fg"]
    maps2 = LR.make_maps(case2)
    a2 = LR.assign(case2, maps2, batch, B)
    items2, _, aux2 = LR.restate_run(case2, maps2, batch)
    ref2, _ = LR.reference(case2, maps2, (a2["fg"], a2["gt_idx"], a2["t_sc"]), a2["gpad"])
    assert not aux2["fg_mask"].any() and items2[0] == 0 and items2[2] == 0 and torch.allclose(items2.double(), ref2, rtol=1e-5, atol=0)


def test_case_table_is_well_formed():
    names = [c["name"] for c in LR.CASES]
    assert len(set(names)) == len(names)
    whys = " ".join(c["what"] for c in LR.CASES)
    for k in range(1, 8):
        assert f"Why {k}" in whys, f"no case names item {k} of the issue's list of unreached code"
    for c in LR.CASES:
        assert max(len(p) for p in LR.BOXES[c["boxes"]]) <= 64 and len(LR.BOXES[c["boxes"]]) <= 4
