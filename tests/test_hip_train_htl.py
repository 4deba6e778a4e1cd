"""GPU: `train.Trainer` with hierarchical task learning (htl) on yolov10n_3D at 320 x 256, four KITTI frames, B = 2 (two micro-batches and
one optimizer step per epoch), 8 epochs: the first epoch whose 3D items get a weight is 6 (utils/htl.py:34, 41).

Every comparison is bit for bit: the trainer, the loop written out with the public pieces, and a resumed run make the same launches on the
same data in the same order."""
import os
import random

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, optim, train
from yolov10_3d_amd._lib import Y3DError

import htl_ref as H
import train_ref as R
from kitti_labels_tree import fixture, write_tree

pytestmark = pytest.mark.gpu

DEV = "cuda"
RES = (320, 256)
FRAMES, EPOCHS = 4, 8
FIT = dict(epochs=EPOCHS, batch=2, nbs=4, warmup_epochs=0, optimizer="SGD", lr0=0.01)
NAMES = list(H.NAMES)


class Interrupted(Exception):
    pass


class Split320:
    """a kitti.DeviceSplit that builds its training batches at 320 x 256; `stop_at`: the epoch seed at which the run is interrupted; `seeds`:
    the seeds asked for, in order"""

    def __init__(self, sp, stop_at=None):
        self.sp, self.stop_at, self.seeds = sp, stop_at, []

    def __len__(self):
        return len(self.sp)

    def epoch(self, batch, args, shuffle=True, seed=0):
        if seed == self.stop_at:
            raise Interrupted()
        self.seeds.append(seed)
        return self.sp.epoch(batch, args, mode="train", shuffle=shuffle, seed=seed, resolution=RES)


def new_model(seed=3, **args):
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(seed)
    model = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()
    for k, v in args.items():
        setattr(model.args, k, v)
    model.model[-1].restack()
    return model


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    z = fixture()
    z4 = {k: z[k][:FRAMES] for k in ("label_text", "calib_text", "frame_wh")}
    root = write_tree(str(tmp_path_factory.mktemp("htl_tree")), z4, images=True)
    return kitti.DeviceSplit(root, device=DEV)


def run_state(t):
    torch.cuda.synchronize()
    return {"model": {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()},
            "ema": {k: v.detach().cpu().clone() for k, v in t.ema.ema.state_dict().items()},
            "opt": t.opt.state.flat.cpu().clone(), "counters": t.opt.state.norm_clip.cpu().clone(), "updates": t.ema.updates,
            "history": [dict(h) for h in t.history], "htl": t.htl.state_dict() if t.htl is not None else None}


def same_run(a, b, what):
    for part in ("model", "ema"):
        for k, v in a[part].items():
            assert torch.equal(v, b[part][k]), f"{what}: {part} {k} differs"
    assert torch.equal(a["opt"], b["opt"]), f"{what}: optimizer state differs"
    assert a["updates"] == b["updates"] and a["history"] == b["history"], f"{what}: history differs"
    for k, v in a["htl"].items():
        assert torch.equal(v, b["htl"][k]) if torch.is_tensor(v) else v == b["htl"][k], f"{what}: htl state {k} differs"


@pytest.fixture(scope="module")
def straight(tree, tmp_path_factory):
    save_dir = str(tmp_path_factory.mktemp("htl_straight"))
    split = Split320(tree)
    t = train.Trainer(new_model(), split, None, save_dir=save_dir, htl=True, **FIT)
    t.fit()
    return run_state(t), save_dir, split.seeds


def test_fit_equals_the_loop_written_out(tree, straight):
    got, save_dir, seeds = straight
    assert seeds == [(0 - 1) % (1 << 32)] + list(range(EPOCHS)), "the e0 pass draws its own order, then one per epoch"
    model = new_model()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    opt = optim.build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=0.0005 * 2 * 2 / 4, iterations=EPOCHS, device_momentum=True)
    ema = optim.ModelEMA(model)
    ema.ema.model[-1].restack()
    sched = optim.Schedule(opt, EPOCHS, 2, lrf=0.01, warmup_epochs=0, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=4, batch=2)
    acc = optim.GradAccumulator(model.parameters())
    rows = R.do_train_rows(FRAMES, 2, EPOCHS, 4, 0)
    assert [r[4] for r in rows] == [False, True] * EPOCHS
    args = kitti.data_args()
    hw = train.HtlWeights(DEV)
    model.criterion = model.init_criterion()
    model.criterion.set_item_weights(hw.table)

    def batches(seed):
        for b in tree.epoch(2, args, mode="train", shuffle=True, seed=seed, resolution=RES):
            yield dict(b, img=b["img"].permute(0, 3, 1, 2))

    # engine/trainer.py:498-512: train mode, no_grad, the items summed and divided by the number of batches
    model.train()
    total, n = None, 0
    with torch.no_grad():
        for b in batches((0 - 1) % (1 << 32)):
            loss, items = model(b)
            assert not loss.requires_grad
            total = items.float().clone() if total is None else total + items.float()
            n += 1
    assert n == 2
    ei = total / n
    history = []
    for epoch in range(EPOCHS):
        hw.update(ei, epoch)
        model.train()
        acc.reset()
        tloss = None
        for i, b in enumerate(batches(epoch)):
            _, _, ni, _, stepped = rows[2 * epoch + i]
            sched.iteration(ni, epoch)
            loss, items = model(b)
            loss.backward()
            del loss
            acc.add()
            items = items.detach().float()
            tloss = items.clone() if tloss is None else (tloss * i + items) / (i + 1)
            ei = items  # the LAST micro-batch's items feed the next update, not the epoch mean (:398)
            if stepped:
                acc.bind()
                opt.step(max_norm=10.0)
                acc.reset()
                ema.update(model, guard=opt.last_norm)
        h = dict(zip(NAMES, (float(v) for v in tloss.cpu())))
        h.update({f"htl/{k}": float(v) for k, v in zip(NAMES, hw.table.cpu())})
        history.append(h)
        sched.epoch_end(epoch)
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), got["model"][k]), f"model {k}"
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v.cpu(), got["ema"][k]), f"EMA {k}"
    assert torch.equal(opt.state.flat.cpu(), got["opt"]) and ema.updates == got["updates"] == EPOCHS
    for e, (h, g) in enumerate(zip(history, got["history"])):
        assert all(g[k] == v and np.isfinite(v) for k, v in h.items()), (e, h, g)
    sd = hw.state_dict()
    assert all(torch.equal(v, got["htl"][k]) if torch.is_tensor(v) else v == got["htl"][k] for k, v in sd.items())


def test_weights_follow_the_reference_schedule(straight):
    """epochs 0-5: exactly [1.5, 1.5, 0, 0, 0, 0] x 2; epochs 6 and 7: every 3D item has a non-zero weight and the twelve sum to 6; the steps
    were applied; the columns are in results.csv and the state in the checkpoint"""
    got, save_dir, _ = straight
    hist = got["history"]
    assert [h["epoch"] for h in hist] == list(range(EPOCHS))
    for h in hist[:6]:
        assert [h[f"htl/{k}"] for k in NAMES] == [1.5, 1.5, 0, 0, 0, 0] * 2, h
    for h in hist[6:]:
        w = [h[f"htl/{k}"] for k in NAMES]
        print(f"epoch {h['epoch']}: weights {[f'{v:.4g}' for v in w]}")
        assert all(np.isfinite(v) and v > 0 for v in w) and abs(sum(w) - 6) < 1e-5, w
    assert got["htl"]["count"] == 5 and got["htl"]["have_init"] == 1 and got["htl"]["status"] == 0
    assert float(got["counters"][3]) == EPOCHS and float(got["counters"][4]) == 0, "steps applied / skipped"
    lines = open(os.path.join(save_dir, "results.csv")).read().splitlines()
    assert len(lines) == EPOCHS + 1 and "htl/dep_om" in lines[0] and "train/box_om" in lines[0]
    ck = torch.load(os.path.join(save_dir, "weights", "last.pt"), map_location="cpu", weights_only=False)
    assert set(ck) == set(train.CKPT_KEYS) | {"htl"} and set(ck["htl"]) == {"state", "items"} and ck["htl"]["items"].shape == (12,)


def test_resume_continues_bit_for_bit(tree, straight, tmp_path):
    want, _, _ = straight
    save_dir = str(tmp_path / "interrupted")
    t = train.Trainer(new_model(), Split320(tree, stop_at=4), None, save_dir=save_dir, htl=True, **FIT)
    with pytest.raises(Interrupted):
        t.fit()
    last = os.path.join(save_dir, "weights", "last.pt")
    assert torch.load(last, map_location="cpu", weights_only=False)["epoch"] == 3
    split = Split320(tree)
    t = train.Trainer(new_model(seed=11), split, None, resume=last, htl=True, **FIT)  # other weights: everything comes from the file
    assert t.start_epoch == 4
    t.fit()
    assert split.seeds == [4, 5, 6, 7], "a resumed run restores the state instead of repeating the e0 pass"
    same_run(run_state(t), want, "resumed against straight")
    # a checkpoint of a run without htl holds no state to continue from
    ck = torch.load(last, map_location="cpu", weights_only=False)
    del ck["htl"]
    torch.save(ck, last)
    with pytest.raises(Y3DError, match="no htl state"):
        train.Trainer(new_model(), Split320(tree), None, resume=last, htl=True, **FIT)


def count_calls(names):
    """counting wrappers around entries of the library binding -> (counts, undo)"""
    L = y3d.lib()
    counts, orig = {n: 0 for n in names}, {}
    for n in names:
        fn = getattr(L, n)
        orig[n] = fn

        def wrapped(*a, _n=n, _fn=fn):
            counts[_n] += 1
            return _fn(*a)

        setattr(L, n, wrapped)

    def undo():
        for n, fn in orig.items():
            setattr(L, n, fn)

    return counts, undo


def test_htl_unset_makes_the_calls_of_before(tree):
    """`htl=None` with `model.args.htl` off: no table, no weighted entry, no update launch, no e0 pass; the history equals the plain loop
    written out (tests/test_hip_train.py checks that loop against the trainer for model and optimizer state)"""
    fit = dict(FIT, epochs=2)
    counts, undo = count_calls(("loss3d", "loss3d_weighted", "htl_update"))
    try:
        split = Split320(tree)
        model = new_model()
        t = train.Trainer(model, split, None, **fit)
        t.fit()
        assert t.htl is None and split.seeds == [0, 1]
        assert counts == {"loss3d": 2 * 2 * 2, "loss3d_weighted": 0, "htl_update": 0}, counts
        assert model.criterion.one2one.item_w is None and model.criterion.one2many.item_w is None
        assert not any(k.startswith("htl/") for k in t.history[0])
        got = [dict(h) for h in t.history]
        # ... and with htl on the same loop takes the other entry for every head set, the e0 pass included, and one update per epoch
        for k in counts:
            counts[k] = 0
        t = train.Trainer(new_model(), Split320(tree), None, htl=True, **fit)
        t.fit()
        assert counts == {"loss3d": 0, "loss3d_weighted": 2 * 2 * 3, "htl_update": 2}, counts
    finally:
        undo()
    model = new_model()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    opt = optim.build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=0.0005 * 2 * 2 / 4, iterations=2, device_momentum=True)
    sched = optim.Schedule(opt, 2, 2, lrf=0.01, warmup_epochs=0, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=4, batch=2)
    acc = optim.GradAccumulator(model.parameters())
    args = kitti.data_args()
    for epoch in range(2):
        model.train()
        acc.reset()
        tloss = None
        for i, b in enumerate(tree.epoch(2, args, mode="train", shuffle=True, seed=epoch, resolution=RES)):
            sched.iteration(2 * epoch + i, epoch)
            loss, items = model(dict(b, img=b["img"].permute(0, 3, 1, 2)))
            assert abs(float(loss.detach()) - 2 * float(items.sum())) < 1e-5 * abs(float(loss.detach()))  # times B
            loss.backward()
            del loss
            acc.add()
            items = items.detach().float()
            tloss = items.clone() if tloss is None else (tloss * i + items) / (i + 1)
            if i == 1:
                acc.bind()
                opt.step(max_norm=10.0)
                acc.reset()
        sched.epoch_end(epoch)
        assert all(got[epoch][k] == float(v) for k, v in zip(NAMES, tloss.cpu())), epoch


def test_refusals(tree):
    # a model that is not on a HIP device (tests/test_train_host.py has the same without a GPU)
    cpu = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml")
    with pytest.raises(NotImplementedError, match="htl"):
        train.Trainer(cpu, Split320(tree), None, htl=True, **FIT)
    # a 2D model
    m2 = y3d.YOLOv10DetectionModel("yolov10n.yaml").to(DEV)
    with pytest.raises(NotImplementedError, match="htl.*2D"):
        train.Trainer(m2, Split320(tree), None, htl=True, **FIT)
    m2.args.htl = True
    with pytest.raises(NotImplementedError, match="htl"):
        train.Trainer(m2, Split320(tree), None, **FIT)
    # distillation together with htl: by the argument and by model.args
    with pytest.raises(NotImplementedError, match="htl with distillation"):
        train.Trainer(new_model(distillation=True), Split320(tree), None, htl=True, **FIT)
    with pytest.raises(NotImplementedError, match="htl with distillation"):
        train.Trainer(new_model(distillation=True, htl=True), Split320(tree), None, **FIT)
    # htl=False overrides model.args
    t = train.Trainer(new_model(htl=True), Split320(tree), None, htl=False, **FIT)
    assert t.htl is None


def test_a_non_finite_weight_raises_at_the_epochs_end(tree):
    """a status bit left by the update (here: planted in the state, as a NaN weight of the table) raises Y3DError naming the items, at the
    epoch's read-back; the optimizer's skip rule kept the steps from being applied"""
    t = train.Trainer(new_model(), Split320(tree), None, htl=True, **dict(FIT, epochs=2))
    nan_items = torch.full((12,), float("nan"), device=DEV)
    t._ei = nan_items  # the e0 pass is taken as done; NaN items only enter the ring at epoch 0 ...
    t.htl.update(nan_items, 0)
    for _ in range(4):
        t.htl.update(nan_items, 0)  # ... a full ring of them makes the weights of the run's first update NaN
    p0 = [p.detach().clone() for p in t.model.parameters()]
    with pytest.raises(Y3DError, match="htl weights not finite in epoch 0: box_om, cls_om, dep_om"):
        t.fit()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(p0, t.model.parameters())), "a step with NaN weights moved a parameter"
    assert float(t.opt.last_norm[4]) == 1 and float(t.opt.last_norm[3]) == 0
