"""GPU: the 2D losses with `max_boxes` set - more than 64 ground-truth boxes per image on the crowded route of csrc/tal_loss2d.hip
(y3d_tal2d_assign_crowded: no (B, n, A) plane, boxes look at the grid cells under them, anchors resolve by claim counts).

The cases are tests/crowded_cases.py's; the references and the bounds are those of tests/test_hip_losses.py, read from there:
fg_mask and target_gt_idx equal to the oracle's (`oracle.restate.tal2d`, any box count) at every anchor and target_scores within 1e-4
(`assert_assignment`), after the case has shown on the oracle's own metrics that none of its decisions is closer than
`loss_ref.MARGIN_FLOOR` to flipping (`assert_margins`); loss items and per-group map gradients against the float64 reference within
`TOL` (`compare`).  Where the two routes take the same batch their integer outputs are equal and their floats agree within the same bounds.
"""
import pytest
import torch

import crowded_cases as CC
import loss_ref as LR
import test_hip_losses as THL  # its checkers and its bounds, not its tests

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import loss as PL  # noqa: E402

DEV = THL.DEV
TOL = THL.TOL  # (items, gradient groups) per dtype
SCORES_TOL = 1e-4  # the bound of THL.assert_assignment on target_scores, relative to their largest entry


def run_case(case, dname, max_boxes):
    """one head set of a case through v8DetectionLoss -> (B, maps, oracle assignment, device assignment, loss, items, map gradients)"""
    dtype = LR.DTYPES[dname]
    batch, B, maps, a = CC.build(case, dname)
    THL.assert_margins(a, case, f"{case['name']}[{dname}]")
    y3d.set_compute_dtype(dtype)
    crit = PL.v8DetectionLoss(LR.model_of(case), tal_topk=case["topk"], max_boxes=max_boxes)
    dm = THL.device_maps(maps, dtype)
    loss, items = crit(dm, {k: v.to(DEV) for k, v in batch.items()})
    loss.backward()
    PL.check_target_overflow(wait=True)
    return B, maps, a, THL.last_assignment(crit), loss, items, [m.grad for m in dm]


@pytest.mark.parametrize("name,dname", CC.case_ids(), ids=[f"{n}-{d}" for n, d in CC.case_ids()])
def test_crowded_case_vs_oracle_and_float64_reference(name, dname):
    """every crowded case: assignment equal to the oracle's at every anchor, items and per-group gradients within the bounds.  The
    c65_* cases (65 boxes in one image under max_boxes=128) are the smallest batch the package could not train on before."""
    case = CC.BY_NAME[name]
    what = f"{name}[{dname}]"
    n_max = max(len(p) for p in CC.BOXES[case["boxes"]])
    assert PL.TARGET_CAP < n_max <= case["max_boxes"]
    B, maps, a, dev, loss, items, grads = run_case(case, dname, case["max_boxes"])
    A = a["fg"].shape[1]
    if name == "c70_lds":
        assert A == 8400 and A * 4 <= 96 * 1024, "the metrics of a box's cells are meant to stay in LDS"
    if name == "c65_global":
        assert A == 33600 and A * 4 > 96 * 1024, "the metric row must not fit the top-k kernel's LDS budget"
    if name.startswith(("c129", "c512")):
        assert int((a["multi"] > 1).sum()) * 2 > int(a["fg"].sum()), "most foreground anchors are meant to be claimed by several boxes"
    THL.assert_assignment(dev, a, what)
    assert dev[0].any()
    assert abs(float(loss) - B * float(items.sum())) <= 1e-5 * abs(float(loss)) + 1e-12
    THL.compare(case, dname, B, maps, a, dev, items, grads, float(B), what)


@pytest.mark.parametrize("name,dname", CC.case_ids(CC.BOTH_ROUTES), ids=[f"{n}-{d}" for n, d in CC.case_ids(CC.BOTH_ROUTES)])
def test_both_routes_agree_up_to_64_boxes(name, dname):
    """the same batch through max_boxes=None (64 rows, the dense kernels) and max_boxes=128 (the crowded route): fg_mask and
    target_gt_idx identical, target_scores / items / gradients within the bounds of the float64 comparison"""
    case = {c["name"]: c for c in CC.BOTH_ROUTES}[name]
    it_tol, g_tol = TOL[dname]
    B, maps, a, dev0, loss0, items0, grads0 = run_case(case, dname, None)
    _, _, _, dev1, loss1, items1, grads1 = run_case(case, dname, 128)
    THL.assert_assignment(dev0, a, f"{name}[{dname}] dense")
    assert torch.equal(dev0[0], dev1[0]) and torch.equal(dev0[1], dev1[1]), "the routes disagree on fg_mask / target_gt_idx"
    assert dev0[0].any()
    err = float((dev0[2] - dev1[2]).abs().max() / dev0[2].abs().max().clamp(min=1e-4))
    print(f"{name}[{dname}]: target_scores differ by {err:.2e} between the routes")
    assert err <= SCORES_TOL
    THL.check_items(items1, items0.detach().double().cpu(), it_tol, f"{name}[{dname}] crowded vs dense")
    g0, g1 = [g.detach().double().cpu() for g in grads0], [g.detach().double().cpu() for g in grads1]
    THL.check_groups(g1, g0, LR.groups2d(case["nc"]), g_tol, dev0[0], f"{name}[{dname}] crowded vs dense")


def test_row_bound_changes_nothing_on_the_crowded_route():
    """assignment and items with `n_used` from pad_targets equal those with n_used = None (all 128 rows walked)"""
    case = CC.BY_NAME["c65_nc80_k10"]
    batch, B, maps, a = CC.build(case, "fp32")
    y3d.set_compute_dtype(torch.float32)
    crit = PL.v8DetectionLoss(LR.model_of(case), tal_topk=case["topk"], max_boxes=128)
    db = {k: v.to(DEV) for k, v in batch.items()}
    H, W = maps[0].shape[2:]
    g, n_used = crit.targets(db, B, H, W, DEV)
    PL.check_target_overflow(wait=True)
    assert int(n_used) == 65 and g.shape == (B, 128, 5)
    out = []
    for nu in (n_used, None):
        dm = [m.detach() for m in THL.device_maps(maps, torch.float32)]
        cfg = PL.LossCfg2d(crit.stride[:len(dm)], crit.nc, crit.topk, 0.5, 6.0, (1.0, 1.0, 1.0))
        out.append([t.cpu() for t in PL.Loss2dFn.apply(cfg, g, nu, *dm)[1:5]])
    for x, y, nm in zip(out[0], out[1], ("items", "fg_mask", "target_gt_idx", "target_scores")):
        assert torch.equal(x, y), f"{nm} depends on the padded row bound"
    assert out[0][1].any()


def test_v10_loss_pads_once_and_both_sets_take_the_capacity(monkeypatch):
    """v10DetectLoss(model, max_boxes=128): one pad_targets call per step, both head sets on 128-row targets"""
    case = CC.BY_NAME["c65_nc80_k10"]
    batch, B, maps, a = CC.build(case, "fp32")
    y3d.set_compute_dtype(torch.float32)
    crit = PL.v10DetectLoss(LR.model_of(case), max_boxes=128)
    assert crit.max_boxes == crit.one2many.max_boxes == crit.one2one.max_boxes == 128 and (crit.one2many.topk, crit.one2one.topk) == (10, 1)
    calls = []
    orig = PL.pad_targets
    monkeypatch.setattr(PL, "pad_targets", lambda *args, **kw: calls.append(kw.get("cap")) or orig(*args, **kw))
    preds = {"one2many": THL.device_maps(maps, torch.float32), "one2one": THL.device_maps(maps, torch.float32)}
    loss, items = crit(preds, {k: v.to(DEV) for k, v in batch.items()})
    loss.backward()
    PL.check_target_overflow(wait=True)
    assert calls == [128] and items.shape == (6,) and torch.isfinite(items).all()
    THL.assert_assignment(THL.last_assignment(crit.one2many), a, "v10 one2many")


def test_crowded_overflow_names_the_capacity_in_use():
    """300 boxes in one image under max_boxes=256: reported once, naming 256 and 300 (tests/test_hip_bench_path.py's overflow test at 64)"""
    PL.check_target_overflow(wait=True)
    rows = torch.zeros(300 + 3, 6, device=DEV)
    rows[:300, 0] = 1  # image 1 has 300 boxes, image 0 has 3
    rows[:, 2:] = 0.5
    gt, n_used = PL.pad_targets(rows, 2, 5, (64.0, 64.0), cap=256)
    assert int(n_used) == 256 and gt.shape == (2, 256, 5)
    with pytest.raises(y3d.Y3DError, match=r"300 ground-truth boxes.*256 per image") as exc:
        PL.check_target_overflow(wait=True)
    assert "max_objs" not in str(exc.value)
    PL.check_target_overflow(wait=True)  # reported once
    gt, n_used = PL.pad_targets(rows[100:], 2, 5, (64.0, 64.0), cap=256)  # 200 + 3 boxes: fine
    PL.check_target_overflow(wait=True)
    assert int(n_used) == 200


def _batch_2d(per_image, hw, nc, seed):
    """a 2D training batch (img, batch_idx, cls, bboxes xywh in [0, 1]) from per-image pixel boxes"""
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    rows = [(b, box) for b, boxes in enumerate(per_image) for box in boxes]
    px = torch.tensor([box for _, box in rows], dtype=torch.float32).view(-1, 4)
    batch = {"img": torch.rand(len(per_image), 3, H, W, generator=g), "batch_idx": torch.tensor([float(b) for b, _ in rows]),
             "cls": torch.randint(0, nc, (len(rows), 1), generator=g).float(), "bboxes": px / torch.tensor([W, H, W, H], dtype=torch.float32)}
    return {k: v.to(DEV) for k, v in batch.items()}


def test_graphed_step_replays_a_crowded_image():
    """graph.GraphedTrainStep on a tiny 2D model with max_boxes=128: the label capacity defaults to 128 per image, and replays of a
    5-box, a 100-box and another small batch leave items, parameters and momentum where the eager steps leave them - bit for bit, the
    agreement tests/test_hip_modules.py::test_graphed_train_step_matches_eager_steps asks of the default path"""
    from yolov10_3d_amd.graph import GraphedTrainStep
    from yolov10_3d_amd.optim import build_optimizer
    y3d.set_compute_dtype(torch.bfloat16)
    hw, nc = CC.SMALL, 20
    batches = [_batch_2d([CC.crowd(3, hw, 20), CC.crowd(2, hw, 21)], hw, nc, 1), _batch_2d(CC.BOXES["crowd100"], hw, nc, 2),
               _batch_2d([CC.crowd(70, hw, 22), CC.crowd(1, hw, 23)], hw, nc, 3)]
    assert [int((b["batch_idx"] == 0).sum()) for b in batches] == [3, 100, 70]
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=nc, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    res = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(3)
        model = y3d.YOLOv10DetectionModel(cfg).to(DEV).train()
        model.args.max_boxes = 128
        opt = build_optimizer(model, lr=0.01)
        items = []
        if mode == "eager":
            for b in batches:
                loss, it = model(b)
                loss.backward()
                opt.step(max_norm=10.0)
                opt.zero_grad()
                items.append(it.float().cpu())
            assert model.criterion.max_boxes == 128
        else:
            step = GraphedTrainStep(model, opt, batches[0])
            assert step.cap == 128 * 2
            for b in batches:
                loss, it = step(b)
                items.append(it.float().cpu().clone())
        torch.cuda.synchronize()
        PL.check_target_overflow(wait=True)
        res[mode] = (items, {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone())
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a, b)
    for k, v in res["eager"][1].items():
        assert torch.equal(v, res["graph"][1][k]), f"state {k} differs after three steps"
    assert torch.equal(res["eager"][2], res["graph"][2]), "momentum buffers differ"
