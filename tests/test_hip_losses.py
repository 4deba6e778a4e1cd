"""GPU: the task-aligned assigners and the loss kernels (csrc/tal_common.h, tal_loss3d.hip, tal_loss2d.hip) per channel group and at their edges.

Every case of the table in tests/loss_ref.py runs through the product's loss classes and is compared with two references:

* assignment (fg_mask, target_gt_idx: equal at EVERY anchor; target_scores: 1e-4) against `oracle.restate.tal3d` / `tal2d` on the host.
  Before the device result is looked at, the case must show on the oracle's own metrics that none of its decisions is closer than
  `loss_ref.MARGIN_FLOOR` to flipping (3.5e-4 = 16 x the largest fp32-vs-float64 difference of a deciding metric, 2.2e-5; ties that are exact by construction are
  the tie rule's business and are excluded) - tests/test_loss_ref_host.py asserts the same for every case without a GPU;
* loss items and gradient against `loss_ref.loss3d_terms` / `loss2d_terms` (float64, autograd) fed the DEVICE's assignment and the same
  (bf16-rounded, in bf16 mode) logits.  The gradient is compared per channel group and per level (`check_groups`), each group normalised by
  its own largest reference entry: over a whole 38-channel map the 3D-offset channels outweigh the uncertainty, heading-residual and
  class channels by two to three orders, and a wrong sign there passes a whole-map max-norm.

Tolerances are the project's own: fp32 1e-3 on items and on every group; bf16 items 1e-3, gradients 1e-2 (stored in bf16).  `restate`'s own
fp32 host gradients differ from the float64 reference by up to 1.3e-6 of a group's largest entry over these cases
(tests/test_loss_ref_host.py prints it); the fp32 bound stays at 1e-3 unless the device errors are seen to sit 30 x below it.
"""
import pytest
import torch
import torch.nn.functional as F

import loss_ref as LR

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import loss as PL  # noqa: E402
from oracle import restate as RS  # noqa: E402  (the checker)

DEV = "cuda"
TOL = {"fp32": (1e-3, 1e-3), "bf16": (1e-3, 1e-2)}  # (items, gradient groups)


def check_groups(grads, refs, groups, tol, fg=None, what="", zero=()):
    """grads / refs: per level (B, no, H, W).  Max-norm relative error per channel group and per level, each normalised by that group's own
    largest reference entry (floor: 1e-6 x the largest entry of the whole map).  Groups named in `zero` must be exactly 0 on the device;
    every other group must have a non-zero reference in some level when foreground exists.  -> {group: largest error over the levels}"""
    assert all(torch.isfinite(g).all() for g in grads), f"{what}: non-finite gradient"
    errs = LR.group_errors(grads, refs, groups)
    worst = {}
    for (lvl, name), (e, idx) in errs.items():
        worst[name] = max(worst.get(name, 0.0), e)
    print(f"{what}: largest error per group:", {k: f"{v:.2e}" for k, v in worst.items()})
    c0 = 0
    for name, width in groups:
        sl = slice(c0, c0 + width)
        c0 += width
        if name in zero:
            assert all(not g[:, sl].any() for g in grads), f"{what}: group {name} has a zero gain but a non-zero gradient"
        elif fg is not None and fg.any():
            assert any(bool(r[:, sl].any()) for r in refs), f"{what}: the reference gradient of group {name} is zero in every level: the case exercises nothing"
    for (lvl, name), (e, idx) in errs.items():
        if e > tol:
            b, c, hy, hx = idx
            a = sum(g.shape[2] * g.shape[3] for g in grads[:lvl]) + hy * grads[lvl].shape[3] + hx
            info = f" fg {bool(fg[b, a])}" if fg is not None else ""
            raise AssertionError(f"{what}: group {name} level {lvl}: relative error {e:.3e} > {tol}; worst at image {b} channel {c} anchor {a} "
                                 f"(y {hy}, x {hx}){info}: device {float(grads[lvl][b, c, hy, hx]):.6e} reference {float(refs[lvl][b, c, hy, hx]):.6e}")
    return worst


def check_items(items, ref, tol, what):
    items, ref = items.detach().double().cpu(), ref.double()
    assert torch.isfinite(items).all(), f"{what}: items {items.tolist()}"
    err = (items - ref).abs() / ref.abs().clamp(min=1e-6 * float(ref.abs().max()) + 1e-30)
    print(f"{what}: items {[f'{v:.6g}' for v in items.tolist()]} relative errors {[f'{v:.1e}' for v in err.tolist()]}")
    assert float(err.max()) <= tol, f"{what}: items {items.tolist()} vs {ref.tolist()}: relative error {float(err.max()):.3e} > {tol}"


def criterion(case, **over):
    cls = PL.DDDetectionLoss if case["fam"] == "3d" else PL.v8DetectionLoss
    return cls(LR.model_of(case, **over), tal_topk=case["topk"])


def device_maps(maps, dtype):
    return [y3d.ops._dense_any(m.to(DEV), dtype).requires_grad_(True) for m in maps]


def last_assignment(crit):
    fg, gi, ts = crit.last_assignment
    return fg.cpu(), gi.cpu(), ts.cpu()


def assert_margins(a, case, what):
    ga, gb, _ = LR.assignment_margin(a["align"], a["second"], a["mask_gt"], case["topk"], a["gmask"], a["twins"])
    for g, kind in ((ga, "k-th / (k+1)-th metric of a box"), (gb, "two largest overlaps of a multiply-selected anchor")):
        assert not g.numel() or float(g.min()) > LR.MARGIN_FLOOR, f"{what}: input too close to a tie ({kind}: gap {float(g.min()):.2e})"


def assert_assignment(dev, a, what):
    fg, gi, ts = dev
    bad = (fg != a["fg"]) | (gi != a["gt_idx"])
    if bad.any():
        b, i = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} anchors differ from the oracle; first: image {b} anchor {i}: device fg {bool(fg[b, i])} gt "
                             f"{int(gi[b, i])}, oracle fg {bool(a['fg'][b, i])} gt {int(a['gt_idx'][b, i])}")
    err = float((ts - a["t_sc"]).abs().max() / a["t_sc"].abs().max().clamp(min=1e-4))
    assert err <= 1e-4, f"{what}: target_scores differ from the oracle by {err:.2e}"


def prepare(name, dname):
    case = LR.BY_NAME[name]
    dtype = LR.DTYPES[dname]
    batch, B = LR.make_batch(case)
    maps = LR.make_maps(case, dtype)
    a = LR.assign(case, maps, batch, B)
    assert_margins(a, case, f"{name}[{dname}]")
    return case, dtype, batch, B, maps, a


def compare(case, dname, B, maps, a, dev_assign, items, grads, scale, what):
    """items and gradient of one head set against the float64 reference on the device's assignment; grads = scale * d(sum items)/d(map)"""
    it_tol, g_tol = TOL[dname]
    ref_items, ref_grads = LR.reference(case, maps, dev_assign, a["gpad"])
    check_items(items, ref_items, it_tol, what)
    fam, nc = case["fam"], case["nc"]
    groups = LR.groups3d(nc) if fam == "3d" else LR.groups2d(nc)
    gains = case["gains"] or {}
    zero = []
    if fam == "3d":
        z3 = dict(loss2d=("o2d", "s2d"), cls=("cls",), depth=("dep", "unc"), offset3d=("o3d",), size3d=("s3d",), heading=("hbin", "hres"))
        zero = [g for k, v in gains.items() if v == 0 for g in z3[k]]
    elif gains.get("cls", 1) == 0:
        zero = ["cls"]
    grads = [g.detach().double().cpu() for g in grads]
    assert all(torch.isfinite(g).all() for g in grads), f"{what}: non-finite gradient"
    fg = dev_assign[0]
    worst = check_groups(grads, [r * scale for r in ref_grads], groups, g_tol, fg, what, zero)
    # background anchors: regression gradients exactly 0
    reg = slice(nc, nc + 35) if fam == "3d" else slice(0, 64)
    flat = LR.flatten(grads)[..., reg]
    assert not flat[~fg].any(), f"{what}: a background anchor has a non-zero regression gradient"
    return worst


@pytest.mark.parametrize("name,dname", LR.case_ids(), ids=[f"{n}-{d}" for n, d in LR.case_ids()])
def test_case_vs_oracle_and_float64_reference(name, dname):
    """every row of the case table: assignment equal to the oracle's at every anchor, items and per-group gradients within the bounds"""
    case, dtype, batch, B, maps, a = prepare(name, dname)
    what = f"{name}[{dname}]"
    if "hires" in name:
        assert a["fg"].shape[1] * 4 > 96 * 1024, "the metric row must not fit the top-k kernel's LDS budget"
    y3d.set_compute_dtype(dtype)
    crit = criterion(case)
    dm = device_maps(maps, dtype)
    loss, items = crit(dm, {k: v.to(DEV) for k, v in batch.items()})
    loss.backward()
    PL.check_target_overflow(wait=True)
    dev = last_assignment(crit)
    assert_assignment(dev, a, what)
    if name.endswith("no_fg"):
        assert not dev[0].any() and float(items[0]) == 0 and float(items.sum()) == float(items[1])
    assert abs(float(loss) - B * float(items.sum())) <= 1e-5 * abs(float(loss)) + 1e-12
    compare(case, dname, B, maps, a, dev, items, [m.grad for m in dm], float(B), what)


@pytest.mark.parametrize("fam", ["3d", "2d"])
@pytest.mark.parametrize("boxes", ["tiny", "capacity"])
def test_row_bound_from_pad_targets_changes_nothing(fam, boxes):
    """assignment and items with `n_used` from pad_targets equal those with n_used = None (all 64 rows walked)"""
    case = LR.BY_NAME[("l3_" if fam == "3d" else "l2_") + boxes]
    batch, B = LR.make_batch(case)
    maps = LR.make_maps(case)
    y3d.set_compute_dtype(torch.float32)
    crit = criterion(case)
    db = {k: v.to(DEV) for k, v in batch.items()}
    H, W = maps[0].shape[2:]
    g, n_used = crit.targets(db, B, H, W, DEV)
    PL.check_target_overflow(wait=True)
    assert int(n_used) == max(len(p) for p in LR.BOXES[case["boxes"]])
    out = []
    for nu in (n_used, None):
        dm = [m.detach() for m in device_maps(maps, torch.float32)]
        if fam == "3d":
            r = PL.Loss3dFn.apply(crit.cfg(len(dm)), g, nu, db["calib"], db["mean_sizes"], *dm)
        else:
            cfg = PL.LossCfg2d(crit.stride[:len(dm)], crit.nc, crit.topk, 0.5, 6.0, (RS.HYP["box"], RS.HYP["cls"], RS.HYP["dfl"]))
            r = PL.Loss2dFn.apply(cfg, g, nu, *dm)
        out.append([t.cpu() for t in r[1:5]])
    for x, y, nm in zip(out[0], out[1], ("items", "fg_mask", "target_gt_idx", "target_scores")):
        assert torch.equal(x, y), f"{nm} depends on the padded row bound"
    assert out[0][1].any()


@pytest.mark.parametrize("fam", ["3d", "2d"])
@pytest.mark.parametrize("boxes", ["empty_image", "capacity"])
def test_pad_targets_kernel_vs_oracle_on_interleaved_rows(fam, boxes):
    """pad_targets on rows whose images are interleaved, with an image without rows and with a full one: the oracle's rows, bit for bit"""
    case = LR.BY_NAME[("l3_" if fam == "3d" else "l2_") + boxes]
    batch, B = LR.make_batch(case)
    bi = batch["batch_idx"]
    assert (bi[1:] < bi[:-1]).any(), "rows are meant to be interleaved"
    H, W = case["hw"]
    width = 17 if fam == "3d" else 5
    rows = LR.rows_of(batch, fam)
    ref = RS.pad_targets(rows, B, width, torch.tensor([W, H, W, H], dtype=torch.float32))
    got, n_used = PL.pad_targets(rows.to(DEV), B, width, (float(W), float(H)))
    PL.check_target_overflow(wait=True)
    nm = ref.shape[1]
    assert int(n_used) == nm and got.shape[1] == PL.TARGET_CAP
    assert torch.equal(got[:, :nm].cpu(), ref) and not got[:, nm:].any()


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_no_box_at_all(dname):
    """`batch_idx` of length 0.  2D: items [0, bce, 0] and the dense class gradient of F.binary_cross_entropy_with_logits in float64;
    3D: graph-less zeros (utils/loss.py:873-877)"""
    dtype = LR.DTYPES[dname]
    y3d.set_compute_dtype(dtype)
    it_tol, g_tol = TOL[dname]
    for name in ("l2_nc3_k10", "l2_nc80_kitti", "l3_nc2_k8"):
        case = LR.BY_NAME[name]
        batch, B = LR.make_batch(case)
        batch = {k: (v[:0] if v.shape[0] == batch["batch_idx"].shape[0] and k not in ("calib", "mean_sizes") else v).to(DEV) for k, v in batch.items()}
        maps = LR.make_maps(case, dtype)
        dm = device_maps(maps, dtype)
        loss, items = criterion(case)(dm, batch)
        if case["fam"] == "3d":
            assert not loss.requires_grad and float(loss) == 0 and items.shape == (6,) and not items.any()
            continue
        loss.backward()
        leaves = [m.double().requires_grad_(True) for m in maps]
        sc = LR.flatten(leaves)[..., 64:]
        bce = F.binary_cross_entropy_with_logits(sc, torch.zeros_like(sc), reduction="none").sum()
        (bce * B).backward()
        check_items(items, torch.stack((bce.detach() * 0, bce.detach(), bce.detach() * 0)), it_tol, f"{name}[{dname}] no box")
        assert abs(float(loss) - B * float(bce)) <= it_tol * B * float(bce)
        grads = [m.grad.double().cpu() for m in dm]
        check_groups(grads, [x.grad for x in leaves], LR.groups2d(case["nc"]), g_tol, None, f"{name}[{dname}] no box")
        assert not LR.flatten(grads)[..., :64].any()


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
@pytest.mark.parametrize("fam", ["3d", "2d"])
def test_upstream_gradient_scales_single_sets(fam, dname):
    """(2.5 * loss_o2m + 0.25 * loss_o2o).backward(): the autograd backward multiplies each set's stored gradient by its own d_total"""
    names = ("l3_dual_o2m", "l3_dual_o2o") if fam == "3d" else ("l2_nc3_k10", "l2_nc3_k1")
    y3d.set_compute_dtype(LR.DTYPES[dname])
    runs = []
    for name in names:
        case, dtype, batch, B, maps, a = prepare(name, dname)
        crit = criterion(case)
        dm = device_maps(maps, dtype)
        loss, items = crit(dm, {k: v.to(DEV) for k, v in batch.items()})
        runs.append((case, B, maps, a, crit, dm, loss, items))
    (2.5 * runs[0][6] + 0.25 * runs[1][6]).backward()
    for (case, B, maps, a, crit, dm, loss, items), wgt in zip(runs, (2.5, 0.25)):
        dev = last_assignment(crit)
        assert_assignment(dev, a, case["name"])
        compare(case, dname, B, maps, a, dev, items, [m.grad for m in dm], wgt * B, f"{case['name']}[{dname}] x {wgt}")


def _dual_setup(dname):
    y3d.set_compute_dtype(LR.DTYPES[dname])
    sets = [prepare(n, dname) for n in ("l3_dual_o2o", "l3_dual_o2m")]
    (c1, dtype, batch, B, m1, a1), (cm, _, _, _, mm, am) = sets
    no = c1["nc"] + 35
    assert no % 2 == 1, "the one-to-many half is meant to start at an odd element offset"
    bases = [y3d.ops._dense_any(torch.cat((x, y), 1).to(DEV), dtype).requires_grad_(True) for x, y in zip(m1, mm)]
    return c1, cm, dtype, batch, B, m1, mm, a1, am, no, bases


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_dual_path_both_sets_in_one_gradient_tensor(dname, monkeypatch):
    """DetectLoss3d on the head's own (B, 2 * no, H, W) maps (`_y3d_maps`): DualLoss3dFn writes both sets' gradient rows into one tensor
    (gsw = 2 * no, base pointers offset by no = 37 elements); each half against its own single-set float64 reference"""
    c1, cm, dtype, batch, B, m1, mm, a1, am, no, bases = _dual_setup(dname)
    calls = []
    orig = PL.DualLoss3dFn.apply
    monkeypatch.setattr(PL.DualLoss3dFn, "apply", staticmethod(lambda *args: calls.append(1) or orig(*args)))
    crit = PL.DetectLoss3d(LR.model_of(cm))
    assert crit.one2many.topk == cm["topk"] and crit.one2one.topk == c1["topk"]
    preds = {"one2one": [b[:, :no] for b in bases], "one2many": [b[:, no:] for b in bases], "_y3d_maps": bases}
    loss, items = crit(preds, {k: v.to(DEV) for k, v in batch.items()})
    assert calls == [1], "the dual path was not taken"
    loss.backward()
    assert abs(float(loss) - B * float(items.sum())) <= 1e-5 * abs(float(loss))
    for case, maps, a, c, it, half in ((cm, mm, am, crit.one2many, items[:6], slice(no, 2 * no)), (c1, m1, a1, crit.one2one, items[6:], slice(0, no))):
        dev = last_assignment(c)
        assert_assignment(dev, a, case["name"])
        compare(case, dname, B, maps, a, dev, it, [b.grad[:, half] for b in bases], float(B), f"dual {case['name']}[{dname}]")


@pytest.mark.parametrize("dname", ["fp32", "bf16"])
def test_dual_path_upstream_gradient_scales_per_set(dname):
    """DualLoss3dFn.backward: (2.5 * total_o2m + 0.25 * total_o2o).backward() scales each half of the shared tensor by its own factor"""
    c1, cm, dtype, batch, B, m1, mm, a1, am, no, bases = _dual_setup(dname)
    crit = PL.DetectLoss3d(LR.model_of(cm))
    db = {k: v.to(DEV) for k, v in batch.items()}
    g, n_used = crit.one2one.targets(db, B, bases[0].shape[2], bases[0].shape[3], DEV)
    nl = len(bases)
    t1, i1, fg1, gi1, ts1, _, tm, im, fgm, gim, tsm, _ = PL.DualLoss3dFn.apply(crit.one2one.cfg(nl), crit.one2many.cfg(nl), g, n_used, db["calib"],
                                                                               db["mean_sizes"], *bases)
    (2.5 * tm + 0.25 * t1).backward()
    for case, maps, a, dev, it, half, wgt in ((cm, mm, am, (fgm, gim, tsm), im, slice(no, 2 * no), 2.5), (c1, m1, a1, (fg1, gi1, ts1), i1, slice(0, no), 0.25)):
        dev = (dev[0].bool().cpu(), dev[1].long().cpu(), dev[2].cpu())
        assert_assignment(dev, a, case["name"])
        compare(case, dname, B, maps, a, dev, it, [b.grad[:, half] for b in bases], wgt, f"dual {case['name']}[{dname}] x {wgt}")
