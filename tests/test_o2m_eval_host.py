"""CPU: the one-to-many eval fixtures (tests/o2m_eval_ref.py) meet, recomputed from the files alone, every condition their tool
asserts and tests/test_hip_o2m_eval.py relies on; keyword plumbing, refusals and error texts of `raw_rows3d`, `Validator3d`,
`Predictor3d`, the head's shape probe and the `--use-o2m-depth` flag of tools/validate.py, on host stubs."""
import importlib.util
import inspect
import os
import types

import pytest
import torch

from conftest import ROOT

import o2m_eval_ref as F
import val_tail_ref as V

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, modules as M, predict, val
from yolov10_3d_amd import loss as PL


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag", F.TAGS)
def test_fixture_loads_and_holds_what_the_tool_stores(tag):
    g = F.load(tag)
    k1, k2, nl = [int(v) for v in g["meta"]]
    assert (k1, k2, nl) == {"k33": (3, 3, 3), "k31": (3, 1, 2)}[tag]
    A = sum(s * s for s in F.SIZES[:nl])
    assert A >= F.KM and [tuple(x.shape) for x in g["x"]] == [(2, c, s, s) for c, s in zip((16, 32, 64), F.SIZES[:nl])]
    assert tuple(g["y"].shape) == tuple(g["y_m"].shape) == (2, 38, A)
    assert tuple(g["rowsO"].shape) == tuple(g["fused"].shape) == (2, F.MAX_DET, 37) and tuple(g["rowsM"].shape) == (2, F.KM, 37)
    assert all(t.dtype == torch.float32 for t in (g["y"], g["y_m"], g["rowsO"], g["rowsM"], g["fused"]))
    assert any(k.startswith("model.0.o2o_heads.") for k in g["state"]) and any(k.startswith("model.0.o2m_heads.") for k in g["state"])
    assert g["sklearn_version"].numel() == 3 and g["numpy_version"].numel() == 3
    # the rebuilt level maps: the decode leaves every channel but nc .. nc + 6 as it is, and changes those
    flat = torch.cat([m.reshape(2, 38, -1) for m in g["maps_m"]], 2)
    other = [c for c in range(38) if not 3 <= c < 9]
    assert torch.equal(flat[:, other], g["y_m"][:, other]) and not torch.equal(flat[:, 3:9], g["y_m"][:, 3:9])
    # the one-to-many set is not the one-to-one set, and parameters are the bf16-representable values the tool documents
    w_o, w_m = g["state"]["model.0.o2o_heads.6.0.0.conv.weight"], g["state"]["model.0.o2m_heads.6.0.0.conv.weight"]
    assert not torch.equal(w_o, w_m) and torch.equal(w_m, w_m.bfloat16().float())
    # the reference's rows are what its post-process makes of its outputs (labels are whole numbers below nc; fused = rowsO but the depth)
    assert bool(((g["rowsO"][..., 36] >= 0) & (g["rowsO"][..., 36] < 3) & (g["rowsO"][..., 36] == g["rowsO"][..., 36].round())).all())
    keep = [c for c in range(37) if c != 33]
    assert torch.equal(g["fused"][..., keep], g["rowsO"][..., keep]) and not torch.equal(g["fused"][..., 33], g["rowsO"][..., 33])


def test_fixtures_meet_the_tools_conditions():
    stats = {tag: F.conditions(tag) for tag in F.TAGS}
    print(stats)
    for tag, s in stats.items():
        assert s["fused"] > 0 and s["under_tau"] <= 0.05 * s["fused"], (tag, s)   # the cap val_tail_ref uses for mixed weights
        assert 2 * s["three_voters"] >= s["rows"], (tag, s)
        assert s["iou_gap"] > 1e-6 and s["weight_gap"] > 1e-3, (tag, s)
        assert s["score_ties"] == 0, (tag, s)  # the reference's top-k leaves the order of ties open
        assert s["restated_equal"], f"{tag}: oracle.restate.kde_fuse_depth is not the validator's output"
    assert any(s["lonely"] >= 1 for s in stats.values()), stats


@pytest.mark.parametrize("tag", F.TAGS)
def test_reference_output_passes_the_fusion_check(tag):
    """the reference's own fused rows pass `check_fusion` with no row off its pick: the rule the GPU test applies is one the reference meets"""
    g = F.load(tag)
    worst, off_pick = V.check_fusion(g["fused"], g["rowsO"], F.fusion_rows(tag), V.TAU_MIXED, tag)
    assert worst == 0.0 and off_pick == 0


# ---------------------------------------------------------------------------------------------------------------- plumbing
def tiny_head(**kw):
    chan = {k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")}
    hd = M.v10Detect3d(3, (16, 32, 64), False, chan, kw.get("use_predecessors", False), True, False, False, 3, False, False, 3, 3)
    hd.stride = torch.tensor([8.0, 16.0, 32.0])
    return hd


class StubModel:
    """what the validators and predictors read of a model before the first launch; calling it is an error"""

    def __init__(self, head, device="cuda"):
        self.model, self.yaml, self.names, self.training = [head], {"nc": 3}, {0: "Car", 1: "Pedestrian", 2: "Cyclist"}, False
        self.stride, self._device, self.calls = head.stride, torch.device(device), 0

    def parameters(self):
        yield types.SimpleNamespace(device=self._device)

    def eval(self):
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def __call__(self, img):
        self.calls += 1
        raise AssertionError("the forward was reached")


def test_head_probe_and_switch_default():
    hd = tiny_head().eval()
    assert M.v10Detect3d.eval_one2many is False and hd.eval_one2many is False
    xs = [torch.zeros(2, c, s, s) for c, s in zip((16, 32, 64), (8, 4, 2))]
    off = hd(xs)
    assert list(off) == ["one2one", "o2o_embs"]
    hd.eval_one2many = True
    on = hd(xs)
    assert list(on) == ["one2one", "o2o_embs", "one2many"]
    y, maps = on["one2many"]
    assert y.device.type == "meta" and tuple(y.shape) == (2, 38, 84) == tuple(on["one2one"][0].shape)
    assert [tuple(m.shape) for m in maps] == [(2, 38, 8, 8), (2, 38, 4, 4), (2, 38, 2, 2)]
    assert list(hd.train()(xs)) == ["one2many", "one2one", "o2m_embs", "o2o_embs", "depth_maps"]  # training: as before, switch or not
    del hd.o2m_heads
    with pytest.raises(y3d.Y3DError, match="no one-to-many branches"):
        hd._one2many_heads()


def test_row_chain_refusals_come_before_the_forward():
    sig = inspect.signature(predict.raw_rows3d).parameters
    assert sig["use_o2m_depth"].default is False and sig["depth_maps"].default is None
    assert (predict.O2M_FACTOR, predict.O2M_ROWS_MAX) == (5, V.FUSION_KM_MAX)
    model = StubModel(tiny_head())
    img = torch.zeros(1, 3, 64, 64)  # maps 8^2 / 4^2 / 2^2: 84 anchors
    assert predict.anchors_of(model, img) == 84 and predict.anchors_of(model, torch.zeros(2, 3, 256, 320)) == 1680
    for max_det, match in ((50, "84 anchors"), (17, "84 anchors"), (781, "at most 3902")):
        with pytest.raises(y3d.Y3DError, match=match):
            predict.raw_rows3d(model, img, max_det, use_o2m_depth=True)
    with pytest.raises(y3d.Y3DError, match="at most 3902"):  # whatever the image size
        predict.raw_rows3d(model, torch.zeros(1, 3, 2048, 2048), 781, use_o2m_depth=True)
    assert model.calls == 0 and model.model[-1].eval_one2many is False
    predict.check_o2m(16, 84)      # 80 rows of 84 anchors
    predict.check_o2m(780, 3902)   # the fusion kernel's last size
    with pytest.raises(AssertionError, match="forward was reached"):
        predict.raw_rows3d(model, img, 16, use_o2m_depth=True)
    assert model.model[-1].eval_one2many is False  # set for the call only
    with pytest.raises(y3d.Y3DError, match="one-to-many output"):
        predict.o2m_rows3d(torch.zeros(1, 38, 84), torch.zeros(1, 38, 80), 16, 3)
    for bad in ((torch.zeros(2, 5, 37), torch.zeros(3, 4, 4)), (torch.zeros(2, 5, 37), torch.zeros(2, 4)), (torch.zeros(5, 37), torch.zeros(1, 4, 4))):
        with pytest.raises(y3d.Y3DError, match="depth_from_map: expected"):
            kitti.depth_from_map(*bad)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        kitti.depth_from_map(torch.zeros(2, 5, 37), torch.zeros(2, 4, 4))


def test_validator3d_keywords():
    sig = inspect.signature(val.Validator3d).parameters
    assert all(sig[k].default is None for k in ("use_o2m_depth", "use_dino_depth", "depth_fn"))
    head = tiny_head()
    model = StubModel(head)
    v = val.Validator3d(model, "/nowhere")
    assert (v.use_o2m_depth, v.use_dino_depth, v.depth_fn) == (False, False, None)
    args = kitti.data_args()
    args.use_o2m_depth, args.use_dino_depth = True, True
    v = val.Validator3d(model, "/nowhere", args=args)
    assert (v.use_o2m_depth, v.use_dino_depth) == (True, True)
    v = val.Validator3d(model, "/nowhere", args=args, use_o2m_depth=False, use_dino_depth=False)
    assert (v.use_o2m_depth, v.use_dino_depth) == (False, False)
    with pytest.raises(y3d.Y3DError, match="depth_fn must be a callable"):
        val.Validator3d(model, "/nowhere", depth_fn=3)
    # no depth callable: loss.teacher_map's wording, before the dataset is touched
    prev = PL.set_teacher(None)
    try:
        v = val.Validator3d(model, "/nowhere", use_dino_depth=True)
        with pytest.raises(y3d.Y3DError, match=r"loss\.set_teacher\(fn\), \(depth_maps, embeddings\) = fn\(img\); the DINOv2 teacher itself is not part"):
            v()
        fn = lambda img: (None, None)
        PL.set_teacher(fn)
        assert v._depth_callable() is fn
        own = lambda img: (None, None)
        assert val.Validator3d(model, "/nowhere", use_dino_depth=True, depth_fn=own)._depth_callable() is own
    finally:
        PL.set_teacher(prev)
    # the head's switch is set for the run and put back, also when the run fails; one-to-many wins over the depth map
    seen = []

    def batches(dino):
        seen.append((head.eval_one2many, dino))
        raise RuntimeError("stop")

    for o2m, was in ((True, False), (False, True)):
        head.eval_one2many = was
        v = val.Validator3d(model, "/nowhere", use_o2m_depth=o2m, use_dino_depth=True, depth_fn=own)
        v._run_batches = batches
        with pytest.raises(RuntimeError, match="stop"):
            v()
        assert head.eval_one2many is was
    assert seen == [(True, None), (False, own)]
    head.eval_one2many = False


def test_predictor3d_keyword_reaches_the_row_chain(monkeypatch):
    assert inspect.signature(predict.Predictor3d).parameters["use_o2m_depth"].default is False
    model = StubModel(tiny_head())
    got = []

    def rows(model, img, max_det, **kw):
        got.append((max_det, kw))
        raise RuntimeError("stop")

    monkeypatch.setattr(predict, "raw_rows3d", rows)
    for flag in (False, True):
        p = predict.Predictor3d(model, max_det=20, resolution=(64, 64), use_o2m_depth=flag)
        assert p.use_o2m_depth is flag
        with pytest.raises(RuntimeError, match="stop"):
            p._rows(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), None, True)
    assert got == [(20, {"use_o2m_depth": False}), (20, {"use_o2m_depth": True})]


def test_validate_tool_flag():
    spec = importlib.util.spec_from_file_location("y3d_validate_tool", os.path.join(ROOT, "tools", "validate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["yolov10n_3D.yaml", "--data", "/nowhere"]
    assert tool.parser().parse_args(base).use_o2m_depth is False
    assert tool.parser().parse_args(base + ["--use-o2m-depth"]).use_o2m_depth is True
    with pytest.raises(SystemExit):  # a 2D model has no one-to-many depth
        tool.main(["yolov10n.yaml", "--data", "/nowhere", "--use-o2m-depth"])
