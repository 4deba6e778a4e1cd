"""Host: the opt-in capacity of the 2D losses (`max_boxes`) without a GPU - its validation, the new ABI symbols and the memory condition
of the crowded route's scratch, and the case table of tests/crowded_cases.py on the oracle alone (every case clears the assignment
margin and holds what it is in the table for)."""
from types import SimpleNamespace

import pytest
import torch

import crowded_cases as CC
import loss_ref as LR
from yolov10_3d_amd import _lib
from yolov10_3d_amd import loss as PL


def _model(**args):
    return LR.model_of(LR.BY_NAME["l2_nc3_k10"], **args)


def test_max_boxes_default_and_accepted_values():
    assert PL.v8DetectionLoss(_model()).max_boxes is None and PL.v10DetectLoss(_model()).max_boxes is None
    for v in (128, 192, 256, 320, 384, 448, 512):
        assert PL.v8DetectionLoss(_model(), max_boxes=v).max_boxes == v
        assert PL.v8DetectionLoss(_model(max_boxes=v)).max_boxes == v  # read from model.args
        crit = PL.v10DetectLoss(_model(), max_boxes=v)
        assert crit.max_boxes == crit.one2many.max_boxes == crit.one2one.max_boxes == v
    assert PL.v8DetectionLoss(_model(max_boxes=256), max_boxes=128).max_boxes == 128  # the argument wins
    assert PL.v10DetectLoss(_model(max_boxes=256)).one2one.max_boxes == 256


@pytest.mark.parametrize("bad", [0, 1, 64, 65, 100, 127, 129, 576, 1024, -128, 128.0, "128", True])
def test_max_boxes_outside_the_range_is_refused(bad):
    with pytest.raises(ValueError, match=r"multiple of 64 in 128\.\.512"):
        PL.v8DetectionLoss(_model(), max_boxes=bad)
    with pytest.raises(ValueError, match=r"multiple of 64 in 128\.\.512"):
        PL.v10DetectLoss(_model(max_boxes=bad))


def test_new_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    assert "y3d_tal2d_assign_crowded" in protos and "y3d_tal2d_scratch_floats" in protos
    assert protos["y3d_tal2d_assign_crowded"] == protos["y3d_tal2d_assign"], "the crowded entry point takes y3d_tal2d_assign's arguments"
    assert len(protos["y3d_tal2d_scratch_floats"][1]) == 4
    L = _lib.lib()  # binds every declared symbol: AttributeError if one is not exported
    assert callable(L.tal2d_assign_crowded) and isinstance(L.tal2d_scratch_floats(2, 128, 420, 10), int)


def test_crowded_scratch_does_not_grow_with_boxes_times_anchors():
    f = _lib.lib().tal2d_scratch_floats
    # the issue's condition at B = 32, 512 boxes, 640 x 640: O(B * A + B * n * topk), where the dense planes alone are 2 * 32 * 512 * 8400 floats
    assert 0 < f(32, 512, 8400, 10) <= 32 * 8400 * 8 + 32 * 512 * 64
    assert f(32, 512, 8400, 10) * 50 < 2 * 32 * 512 * 8400
    assert f(32, 512, 33600, 10) > 0  # 1280 x 1280: far from the 2^31 refusal the dense route is close to
    base = (4, 128, 8400, 10)
    for i, grid in enumerate(((1, 2, 4, 32, 64), (64, 128, 256, 512), (420, 8400, 33600, 134400), (1, 10, 16))):
        vals = [f(*(base[:i] + (v,) + base[i + 1:])) for v in grid]
        assert all(v > 0 for v in vals) and vals == sorted(vals), f"not monotone in argument {i}: {vals}"
    assert f(1 << 12, 512, 1 << 20, 10) == -1  # past 2^31 floats: refused, not wrapped


@pytest.mark.parametrize("name,dname", CC.case_ids(CC.CASES + CC.BOTH_ROUTES), ids=[f"{n}-{d}" for n, d in CC.case_ids(CC.CASES + CC.BOTH_ROUTES)])
def test_crowded_case_clears_the_margin_and_holds_what_it_is_there_for(name, dname):
    case = {c["name"]: c for c in CC.CASES + CC.BOTH_ROUTES}[name]
    batch, B, maps, a = CC.build(case, dname)
    ma, mb, ties = CC.margins(case, a)
    fg, multi, gpad = a["fg"], a["multi"], a["gpad"]
    print(f"{name}[{dname}]: {gpad.shape[1]} rows, fg {int(fg.sum())}, multiply selected {int((multi > 1).sum())} (exact ties {ties}), "
          f"gaps top-k {ma:.2e} conflict {mb:.2e}")
    assert min(ma, mb) > LR.MARGIN_FLOOR, "a decision of this case is closer to a tie than host and device arithmetic may differ: take another seed"
    fg2, gi2, _ = LR.replay(a["align"], a["second"], a["gmask"], a["mask_gt"], case["topk"])
    assert torch.equal(fg2, fg) and torch.equal(gi2, a["gt_idx"]) and fg.any()
    if case in CC.BOTH_ROUTES:
        assert gpad.shape[1] <= PL.TARGET_CAP
        return
    counts = [len(p) for p in CC.BOXES[case["boxes"]]]
    assert PL.TARGET_CAP < max(counts) == gpad.shape[1] <= case["max_boxes"] and case["max_boxes"] in PL.CROWDED_CAPS
    box = gpad[0, :, 1:5]
    valid = a["mask_gt"][0, :, 0] > 0
    assert bool(a["twins"][0][valid][:, valid].sum() > valid.sum()), "no duplicated box"
    assert bool((valid & (a["gmask"][0].sum(-1) == 0)).any()), "no box without an anchor centre inside"
    H, W = case["hw"]
    assert bool(((box[:, 0] < 0) | (box[:, 1] < 0) | (box[:, 2] > W) | (box[:, 3] > H)).any()), "no box over the border"
    assert ties > 0, "no exact tie between duplicated rows in the conflict resolution"
    if name.startswith("c65_nc"):
        assert counts == [65, 0] and not fg[1].any()
    if name.startswith(("c129", "c512")):
        assert int((multi > 1).sum()) * 2 > int(fg.sum())


def test_overflow_message_keeps_the_kitti_wording_for_64_only(monkeypatch):
    """check_target_overflow names the capacity in use; `max_objs` is mentioned for the default 64 rows alone"""
    ev = SimpleNamespace(synchronize=lambda: None, query=lambda: True)
    for cap, n, kitti in ((64, 70, True), (256, 300, False)):
        monkeypatch.setattr(PL, "_OVERFLOW_PENDING", [(ev, torch.tensor([n], dtype=torch.int32), cap)])
        with pytest.raises(PL.Y3DError, match=f"{n} ground-truth boxes") as exc:
            PL.check_target_overflow(wait=True)
        msg = str(exc.value)
        assert str(cap) in msg and str(n - cap) in msg and ("max_objs" in msg) == kitti
        PL.check_target_overflow(wait=True)  # reported once
