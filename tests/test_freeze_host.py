"""Host only: the freeze rule (`train.freeze_layer_names`, `train.apply_freeze`) against the separately written restatement of the
reference's lines in freeze_ref.py on all twelve shipped yamls, its refusals, and `load_pretrained_body` on the CPU."""
import copy
import glob
import os

import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import tasks, train
from yolov10_3d_amd._lib import Y3DError

import freeze_ref as FR

YAMLS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(tasks.CFG_DIR, "v10*", "*.yaml")))
SETTINGS = [None, 0, 1, 11, [4, 13], [23], list(range(24))]


def build(name):
    torch.manual_seed(0)
    return (y3d.YOLOv10_3DDetectionModel if "_3D" in name else y3d.YOLOv10DetectionModel)(name)


@pytest.fixture(scope="module")
def models():
    return {n: build(n) for n in YAMLS}


def test_the_twelve_yamls_are_there():
    assert len(YAMLS) == 12, YAMLS


def test_layer_names():
    assert train.freeze_layer_names(None) == [".dfl"] == FR.layer_names(None)
    assert train.freeze_layer_names(0) == [".dfl"]
    assert train.freeze_layer_names(2) == ["model.0.", "model.1.", ".dfl"] == FR.layer_names(2)
    assert train.freeze_layer_names([4, 13]) == ["model.4.", "model.13.", ".dfl"] == FR.layer_names([4, 13])
    assert train.freeze_layer_names(range(3)) == FR.layer_names(3)


@pytest.mark.parametrize("name", YAMLS)
def test_apply_freeze_agrees_with_the_restated_rule(models, name):
    model = models[name]
    assert len(model.model) == 24
    keys = [k for k, _ in model.named_parameters()]
    floating = [p.dtype.is_floating_point for p in model.parameters()]
    for freeze in SETTINGS:
        arrived = [p.requires_grad for p in model.parameters()]
        want = FR.frozen_flags(keys, floating, arrived, freeze)
        if not any(w for w, k in zip(want, keys) if not k.endswith(FR.KEEPS)):
            with pytest.raises(Y3DError, match="leaves no trainable parameter"):
                train.apply_freeze(model, freeze)
            assert [p.requires_grad for p in model.parameters()] == arrived, "a refused freeze changed a flag"
            continue
        frozen = train.apply_freeze(model, freeze)
        got = [p.requires_grad for p in model.parameters()]
        assert got == want, (name, freeze, [k for k, a, b in zip(keys, got, want) if a != b][:5])
        assert frozen == FR.frozen_keys(keys, freeze)
        assert all(not dict(zip(keys, got))[k] for k in frozen)
        if "_3D" not in name:
            assert "model.23.dfl.conv.weight" in frozen, "the 2D models' .dfl weight is frozen under every setting"
    train.apply_freeze(model, None)


def test_model_1_does_not_catch_model_11(models):
    model = models["yolov10n_3D.yaml"]
    frozen = train.apply_freeze(model, [1])
    assert frozen and all(k.startswith("model.1.") for k in frozen)
    named = dict(model.named_parameters())
    assert all(p.requires_grad for k, p in named.items() if k.startswith(("model.10.", "model.11.", "model.13.", "model.16.", "model.19.")))
    assert any(k.startswith("model.13.") for k in named)
    train.apply_freeze(model, None)


def test_a_hand_cleared_flag_comes_back(models):
    model = models["yolov10n_3D.yaml"]
    named = dict(model.named_parameters())
    named["model.3.conv.weight"].requires_grad = False
    named["model.2.cv1.bn.bias"].requires_grad = False
    train.apply_freeze(model, [4])
    assert named["model.3.conv.weight"].requires_grad and named["model.2.cv1.bn.bias"].requires_grad
    assert not named["model.4.cv1.conv.weight"].requires_grad
    train.apply_freeze(model, None)
    assert named["model.4.cv1.conv.weight"].requires_grad


def test_depth_bin_values_stays_off():
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    cfg["fgdm_predictor"] = True
    model = y3d.YOLOv10_3DDetectionModel(cfg)
    key = "model.23.fgdm_predictor.depth_bin_values"
    named = dict(model.named_parameters())
    assert key in named and not named[key].requires_grad
    for freeze in (None, 11, [23]):
        train.apply_freeze(model, freeze)
        assert not named[key].requires_grad, freeze
    train.apply_freeze(model, 11)
    assert named["model.23.fgdm_predictor.proj.0.weight"].requires_grad


@pytest.mark.parametrize("freeze, message", [(24, "leaves no trainable parameter"), (list(range(24)), "leaves no trainable parameter"),
                                             ([30], "layer 30 does not exist"), (25, "layer 24 does not exist"), ([4, 24], "layer 24 does not exist"),
                                             (True, "a bool is not a layer count"), (False, "a bool is not a layer count"),
                                             ([1, True], "non-negative ints"), (-1, "cannot be negative"), ("11", "pass None, an int")])
def test_refusals(models, freeze, message):
    model = models["yolov10n.yaml"]
    before = [p.requires_grad for p in model.parameters()]
    with pytest.raises(Y3DError, match=message):
        train.apply_freeze(model, freeze)
    assert [p.requires_grad for p in model.parameters()] == before


def test_flags_survive_a_restack_both_ways():
    """freezing and unfreezing the head layer both survive v10Detect3d.restack() (it re-points `.data` of the same Parameter objects)"""
    model = build("yolov10n_3D.yaml")
    head = model.model[-1]
    train.apply_freeze(model, [23])
    head.restack()
    assert all(not p.requires_grad for p in head.parameters())
    assert all(p.requires_grad for k, p in model.named_parameters() if not k.startswith("model.23."))
    train.apply_freeze(model, [4])
    head.restack()
    assert all(p.requires_grad for p in head.parameters())
    head.restack()
    train.apply_freeze(model, [23])
    assert all(not p.requires_grad for p in head.parameters())
    frozen = train.apply_freeze(copy.deepcopy(model), [23])
    assert len(frozen) == len(list(head.parameters()))


# ---- load_pretrained_body ----------------------------------------------------------------------------------------------------------------
def state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def unchanged(model, before):
    now = model.state_dict()
    return list(now) == list(before) and all(torch.equal(now[k], v) for k, v in before.items())


@pytest.fixture()
def pair():
    torch.manual_seed(1)
    src = y3d.YOLOv10DetectionModel("yolov10n.yaml")
    for b in src.buffers():  # running statistics that differ from a fresh model's
        if b.is_floating_point():
            b.uniform_(0.5, 1.5)
    torch.manual_seed(2)
    return src, y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")


def check_body(dst, src_sd, before, n):
    body = [k for k in before if not k.startswith("model.23.")]
    assert n == len(body) > 0
    now = dst.state_dict()
    for k in body:
        assert torch.equal(now[k], src_sd[k]), k
    assert any(not torch.equal(before[k], src_sd[k]) for k in body)
    for k in before:
        if k.startswith("model.23."):
            assert torch.equal(now[k], before[k]), f"head tensor {k} changed"


def test_body_from_a_2d_model(pair):
    from yolov10_3d_amd import ops
    src, dst = pair
    before, epoch = state(dst), ops.WEIGHT_EPOCH
    n = dst.load_pretrained_body(src)
    check_body(dst, src.state_dict(), before, n)
    assert ops.WEIGHT_EPOCH != epoch, "load_pretrained_body ends with bump_weight_epoch()"
    assert all(k.split(".")[1] != "23" for k in before if not k.startswith("model.23."))


def test_body_from_a_state_dict_and_files(pair, tmp_path):
    src, dst = pair
    before = state(dst)
    sd = state(src)
    check_body(dst, sd, before, dst.load_pretrained_body(sd))
    # a file written by torch.save(state_dict)
    torch.manual_seed(2)
    dst = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")
    path = str(tmp_path / "body.pt")
    torch.save(sd, path)
    check_body(dst, sd, before, dst.load_pretrained_body(path))
    # a file laid out as the trainer's: "ema" first, else "model"; numpy's random state rides along as train.Trainer.checkpoint keeps it
    import numpy as np
    kind, keys, *rest = np.random.get_state()
    ema = {k: (v + 1 if v.is_floating_point() else v) for k, v in sd.items()}
    for name, ck, want in (("ema.pt", {"epoch": 0, "ema": ema, "model": sd, "rng": {"numpy": (kind, torch.from_numpy(keys.astype(np.int64)), *rest)}, "train_args": {"freeze": [1]}}, ema),
                           ("model.pt", {"epoch": 0, "ema": None, "model": sd}, sd)):
        torch.manual_seed(2)
        dst = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")
        torch.save(ck, str(tmp_path / name))
        check_body(dst, want, before, dst.load_pretrained_body(str(tmp_path / name)))


def test_body_refusals_leave_the_model_unchanged(pair, tmp_path):
    src, dst = pair
    before = state(dst)
    with pytest.raises(Y3DError, match=r"model\.\d+\..*another scale or yaml"):
        dst.load_pretrained_body(y3d.YOLOv10DetectionModel("yolov10s.yaml"))
    assert unchanged(dst, before)
    with pytest.raises(Y3DError, match=r"model\.\d+\..*another scale or yaml"):
        dst.load_pretrained_body(y3d.YOLOv10DetectionModel("yolov10s.yaml").state_dict())
    assert unchanged(dst, before)
    sd = state(src)
    del sd["model.22.cv2.bn.running_var"]  # the last body layer: everything before it would have been copied by a lazy check
    with pytest.raises(Y3DError, match="the source has no model.22.cv2.bn.running_var"):
        dst.load_pretrained_body(sd)
    assert unchanged(dst, before)
    sd = state(src)
    sd["model.3.conv.weight"] = sd["model.3.conv.weight"][:, :-1]
    with pytest.raises(Y3DError, match="model.3.conv.weight is"):
        dst.load_pretrained_body(sd)
    assert unchanged(dst, before)
    path = str(tmp_path / "module.pt")
    torch.save(src, path)
    with pytest.raises(Y3DError, match="export a state_dict"):
        dst.load_pretrained_body(path)
    assert unchanged(dst, before)
    with pytest.raises(Y3DError, match="no state_dict found"):
        dst.load_pretrained_body({"epoch": 3})
    assert unchanged(dst, before)


def test_a_layer_of_another_module_type_is_named():
    """a source whose layer 4 is a Conv where this model has a C2f (another yaml) raises, naming the layer"""
    dst = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")
    src = y3d.YOLOv10DetectionModel("yolov10n.yaml")
    src.model[4] = copy.deepcopy(src.model[3])
    before = state(dst)
    with pytest.raises(Y3DError, match=r"model\.4"):
        dst.load_pretrained_body(src)
    assert unchanged(dst, before)


def test_the_command_line_parses_freeze():
    import importlib.util
    spec = importlib.util.spec_from_file_location("y3d_tools_train", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    p = tool.parser()
    assert p.parse_args(["m.yaml", "--data", "d"]).freeze is None and p.parse_args(["m.yaml", "--data", "d"]).pretrained_body is None
    assert p.parse_args(["m.yaml", "--data", "d", "--freeze", "11"]).freeze == 11
    a = p.parse_args(["m.yaml", "--data", "d", "--freeze", "0,1,2", "--pretrained-body", "x.pt"])
    assert a.freeze == [0, 1, 2] and a.pretrained_body == "x.pt"
    with pytest.raises(SystemExit):
        p.parse_args(["m.yaml", "--data", "d", "--freeze", "a,b"])
