"""GPU: `train.Trainer(freeze=)` on the KITTI tree of tests/test_hip_train.py (5 frames at 320 x 256, B = 2, two windows of two
micro-batches and a short last batch per epoch): fit against the loop written out with `apply_freeze` and the public parts, the
checkpoint's `freeze`, resume (bit for bit; a disagreeing explicit freeze is refused before any launch), and the command line's
`--freeze` / `--pretrained-body`.  Every comparison is torch.equal, as in tests/test_hip_train.py."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, optim, train, val
from yolov10_3d_amd._lib import Y3DError

import train_ref as R
from kitti_labels_tree import fixture, write_tree

pytestmark = pytest.mark.gpu

DEV = "cuda"
RES = (320, 256)
FIT = dict(epochs=2, batch=2, nbs=4, warmup_epochs=0, optimizer="SGD", lr0=0.01)
FRAMES = 5
FREEZE = 11


def _trace_tool():
    spec = importlib.util.spec_from_file_location("make_golden_ops_trace", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools",
                                                                                        "make_golden_ops_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Interrupted(Exception):
    pass


class Split320:
    """a kitti.DeviceSplit that builds its training batches at 320 x 256; `stop_at`: the epoch seed at which the run is interrupted"""

    def __init__(self, sp, stop_at=None):
        self.sp, self.stop_at = sp, stop_at

    def __len__(self):
        return len(self.sp)

    def epoch(self, batch, args, shuffle=True, seed=0):
        if seed == self.stop_at:
            raise Interrupted()
        return self.sp.epoch(batch, args, mode="train", shuffle=shuffle, seed=seed, resolution=RES)


def new_model(seed=3):
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(seed)
    return y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    z = fixture()
    z5 = {k: z[k][:FRAMES] for k in ("label_text", "calib_text", "frame_wh")}
    root = write_tree(str(tmp_path_factory.mktemp("freeze_tree")), z5, images=True)
    return root, kitti.DeviceSplit(root, device=DEV), kitti.DeviceSplit(root, mode="val", device=DEV)


def validator_factory(val_split):
    return lambda m: val.Validator3d(m, val_split, batch=4, plots=False, resolution=RES)


def run_state(t):
    torch.cuda.synchronize()
    return {"model": {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()},
            "ema": {k: v.detach().cpu().clone() for k, v in t.ema.ema.state_dict().items()},
            "opt": t.opt.state.flat.cpu().clone(), "counters": t.opt.state.norm_clip.cpu().clone(), "updates": t.ema.updates,
            "best_fitness": t.best_fitness, "history": [dict(h) for h in t.history]}


@pytest.fixture(scope="module")
def straight(tree, tmp_path_factory):
    root, sp, vsp = tree
    save_dir = str(tmp_path_factory.mktemp("frozen_straight"))
    model = new_model()
    start = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    t = train.Trainer(model, Split320(sp), validator_factory(vsp), save_dir=save_dir, freeze=FREEZE, **FIT)
    frozen = list(t.frozen)
    assert t.accum is not None and [r[4] for r in t.plan] == [False, True, False, True, False, True]
    t.fit()
    return run_state(t), save_dir, frozen, start


def test_fit_with_freeze_equals_the_loop_written_out(tree, straight):
    root, sp, vsp = tree
    got, save_dir, frozen, start = straight
    model = new_model()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    assert train.apply_freeze(model, FREEZE) == frozen and len(frozen) > 50
    opt = optim.build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=0.0005 * 2 * 2 / 4, iterations=4, device_momentum=True)
    model.model[-1].restack()
    ema = optim.ModelEMA(model)
    ema.ema.model[-1].restack()
    sched = optim.Schedule(opt, 2, 3, lrf=0.01, warmup_epochs=0, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=4, batch=2)
    acc = optim.GradAccumulator(model.parameters())
    assert len(acc.params) == len(list(model.parameters())) - len(frozen)
    validator = validator_factory(vsp)(ema.ema)
    rows = R.do_train_rows(FRAMES, 2, 2, 4, 0)
    args = kitti.data_args()
    names = y3d.loss.loss_names(model.args)
    history = []
    for epoch in range(2):
        model.train()
        acc.reset()
        tloss = None
        for i, b in enumerate(sp.epoch(2, args, mode="train", shuffle=True, seed=epoch, resolution=RES)):
            _, _, ni, _, stepped = rows[3 * epoch + i]
            sched.iteration(ni, epoch)
            b = dict(b, img=b["img"].permute(0, 3, 1, 2))
            loss, items = model(b)
            loss.backward()
            del loss
            acc.add()
            items = items.detach().float()
            tloss = items.clone() if tloss is None else (tloss * i + items) / (i + 1)
            if stepped:
                acc.bind()
                opt.step(max_norm=10.0)
                acc.reset()
                ema.update(model, guard=opt.last_norm)
        validator()
        history.append(dict(zip(names, (float(v) for v in tloss.cpu()))))
        sched.epoch_end(epoch)
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), got["model"][k]), f"model {k}"
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v.cpu(), got["ema"][k]), f"EMA {k}"
    assert torch.equal(opt.state.flat.cpu(), got["opt"]) and ema.updates == got["updates"] == 3
    assert len(got["history"]) == 2
    for h, g in zip(history, got["history"]):
        assert all(g[k] == v and np.isfinite(v) for k, v in h.items()), (h, g)
    # the frozen parameters are what they were; their BatchNorm statistics and the trainable layers moved
    for k in frozen:
        assert torch.equal(got["model"][k], start[k]), f"frozen {k} moved"
    assert not torch.equal(got["model"]["model.4.cv1.bn.running_mean"], start["model.4.cv1.bn.running_mean"])
    assert not torch.equal(got["ema"]["model.4.cv1.bn.running_mean"], start["model.4.cv1.bn.running_mean"]), "the EMA follows the running statistics"
    assert any(not torch.equal(v, start[k]) for k, v in got["model"].items() if k.startswith("model.13.") and k.endswith("conv.weight"))


def test_checkpoint_carries_the_freeze_and_resume_continues_bit_for_bit(tree, straight, tmp_path):
    root, sp, vsp = tree
    want, save_dir, frozen, _ = straight
    ck = torch.load(os.path.join(save_dir, "weights", "last.pt"), map_location="cpu", weights_only=False)
    assert set(ck) == set(train.CKPT_KEYS) and ck["train_args"]["freeze"] == FREEZE
    # the file is read with weights_only=True by load_pretrained_body, which takes its EMA
    fresh = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")
    n = fresh.load_pretrained_body(os.path.join(save_dir, "weights", "last.pt"))
    body = [k for k in ck["ema"] if not k.startswith("model.23.")]
    assert n == len(body) and all(torch.equal(fresh.state_dict()[k].float(), ck["ema"][k].float()) for k in body)
    save = str(tmp_path / "interrupted")
    t = train.Trainer(new_model(), Split320(sp, stop_at=1), validator_factory(vsp), save_dir=save, freeze=FREEZE, **FIT)
    with pytest.raises(Interrupted):
        t.fit()
    last = os.path.join(save, "weights", "last.pt")
    assert torch.load(last, map_location="cpu", weights_only=False)["train_args"]["freeze"] == FREEZE
    # a disagreeing explicit freeze: refused before any launch (and before the model's flags are touched)
    model = new_model(seed=11)
    sink = []
    with _trace_tool().recording(sink):
        with pytest.raises(Y3DError, match="disagrees with the checkpoint"):
            train.Trainer(model, Split320(sp), validator_factory(vsp), resume=last, freeze=3, **FIT)
    assert sink == [] and all(p.requires_grad for p in model.parameters())
    # no explicit freeze: the checkpoint's; the same explicit one is accepted too
    t = train.Trainer(model, Split320(sp), validator_factory(vsp), resume=last, **FIT)
    assert t.frozen == frozen and t.train_args["freeze"] == FREEZE and t.start_epoch == 1
    assert [k for k, p in model.named_parameters() if not p.requires_grad] == frozen
    t.fit()
    got = run_state(t)
    for part in ("model", "ema"):
        for k, v in got[part].items():
            assert torch.equal(v, want[part][k]), f"resumed: {part} {k} differs"
    assert torch.equal(got["opt"], want["opt"]) and got["updates"] == want["updates"] and got["best_fitness"] == want["best_fitness"]
    assert got["history"] == want["history"]
    assert torch.equal(got["counters"][2:5], want["counters"][2:5])
    train.Trainer(new_model(seed=11), Split320(sp), None, resume=last, freeze=FREEZE, **FIT)


def test_command_line_freeze_and_pretrained_body(tree, tmp_path, capsys):
    root, sp, vsp = tree
    torch.manual_seed(21)
    src = y3d.YOLOv10DetectionModel("yolov10n.yaml")
    body = str(tmp_path / "body2d.pt")
    sd = {k: v.detach().clone() for k, v in src.state_dict().items()}
    torch.save(sd, body)
    spec = importlib.util.spec_from_file_location("y3d_tools_train", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "train.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    save = str(tmp_path / "cli")
    tool.main(["yolov10n_3D.yaml", "--data", root, "--epochs", "1", "--batch", "2", "--nbs", "4", "--warmup-epochs", "0", "--optimizer", "SGD",
               "--lr0", "0.01", "--save-dir", save, "--freeze", "11", "--pretrained-body", body])
    out = capsys.readouterr().out
    assert "body tensors from" in out and "1 epochs" in out
    ck = torch.load(os.path.join(save, "weights", "last.pt"), map_location="cpu", weights_only=False)
    assert ck["train_args"]["freeze"] == 11 and ck["epoch"] == 0
    named = [k for k, _ in y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").named_parameters()]
    frozen = [k for k in named if any(k.startswith(f"model.{i}.") for i in range(11))]
    assert len(frozen) > 50
    for k in frozen:
        assert torch.equal(ck["model"][k], sd[k]), f"{k}: the frozen tensor is not the file's"
    assert any(not torch.equal(ck["model"][k], sd[k]) for k in named if k.startswith("model.13.") and k in sd), "the neck was not trained"
