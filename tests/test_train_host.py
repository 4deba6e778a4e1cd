"""No GPU: the host side of the training loop (yolov10-3d_amd/train.py) against the restatement of tests/train_ref.py - the iteration plan,
the weight-decay and iteration formulas, the stopping and best-fitness rules, the checkpoint keys, the refusals - and the table builder of
optim.GradAccumulator."""
import math

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import optim, train
from yolov10_3d_amd._lib import Y3DError

import train_ref as R

CASES = [dict(n=5, batch=2, nbs=4, warmup_epochs=0, epochs=3), dict(n=120, batch=2, nbs=8, warmup_epochs=3, epochs=3),
         dict(n=64, batch=64, nbs=64, warmup_epochs=3.0, epochs=3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c['n']}-b{c['batch']}-nbs{c['nbs']}")
def test_plan_equals_the_restated_loop(case):
    want = R.do_train_rows(**case)
    got = train.plan(case["n"], case["batch"], case["epochs"], case["nbs"], case["warmup_epochs"])
    assert [tuple(r) for r in got] == want
    assert len(want) == math.ceil(case["n"] / case["batch"]) * case["epochs"]


def test_the_cases_hold_what_they_are_chosen_for():
    """from the restatement alone: case 0 has a window of two micro-batches and drops one at an epoch boundary; case 1 ramps 1 -> 4;
    case 2 never accumulates"""
    rows = R.do_train_rows(**CASES[0])
    sizes, dropped = R.windows(rows)
    assert 2 in sizes and {r[3] for r in rows} == {2}
    assert dropped and dropped[0] == (0, 2), dropped  # the third batch of epoch 0 waits for a partner that the next epoch never gives it
    assert 1 in sizes  # ... so the first step of epoch 1 holds one micro-batch
    rows = R.do_train_rows(**CASES[1])
    acc = [r[3] for r in rows]
    assert acc[0] == 1 and acc[-1] == 4 and sorted(set(acc)) == [1, 2, 3, 4] and acc == sorted(acc)
    assert max(R.windows(rows)[0]) == 4
    rows = R.do_train_rows(**CASES[2])
    assert {r[3] for r in rows} == {1} and all(r[4] for r in rows)


def test_weight_decay_and_iterations():
    for batch, nbs, wd in [(32, 64, 5e-4), (16, 64, 5e-4), (2, 4, 1e-3), (64, 64, 5e-4), (96, 64, 5e-4), (3, 64, 5e-4)]:
        accumulate = max(round(nbs / batch), 1)
        assert train.scaled_weight_decay(wd, batch, nbs) == wd * batch * accumulate / nbs
    assert train.scaled_weight_decay(5e-4, 32, 64) == 5e-4 and train.scaled_weight_decay(5e-4, 96, 64) == 5e-4 * 96 / 64
    for n, batch, nbs, epochs in [(5, 2, 4, 3), (7481, 32, 64, 400), (100, 128, 64, 10), (64, 64, 64, 1)]:
        assert train.optimizer_iterations(n, batch, epochs, nbs) == math.ceil(n / max(batch, nbs)) * epochs
    assert train.optimizer_iterations(7481, 32, 400, 64) == 117 * 400  # > 10000: `auto` takes SGD


@pytest.mark.parametrize("patience", [0, 1, 3])
def test_stopping_and_best_fitness_rules(patience):
    rng = np.random.default_rng(patience)
    series = [None, 0.0, 0.0, 0.2, 0.1, 0.2, 0.15, 0.1, 0.05, 0.3] + [float(v) for v in rng.random(12).round(1)]
    a, b = train.EarlyStopping(patience), R.Stopper(patience)
    best_a = best_b = None
    for e, f in enumerate(series):
        assert a(e + 1, f) == b(e + 1, f)
        assert (a.best_fitness, a.best_epoch, a.possible_stop, a.patience) == (b.best_fitness, b.best_epoch, b.possible_stop, b.patience)
        if f is not None:
            best_a, best_b = train.better_fitness(best_a, f), R.best_fitness_rule(best_b, f)
            assert best_a == best_b
    c = train.EarlyStopping(patience)
    c.load_state_dict(a.state_dict())
    assert c.state_dict() == a.state_dict()


def test_when_the_loop_validates():
    for epochs, period in [(30, 4), (3, 1), (12, 5)]:
        for epoch in range(epochs):
            want = ((epoch + 1) % period == 0 or (epochs - epoch) <= 10) or epoch + 1 == epochs
            assert train.validates(epoch, epochs, period) == want
    assert train.validates(0, 30, 4, possible_stop=True) and train.validates(0, 30, 4, stop=True) and not train.validates(0, 30, 4)


def test_checkpoint_keys():
    assert set(train.CKPT_KEYS) == {"epoch", "best_fitness", "model", "ema", "updates", "optimizer", "train_args", "train_metrics", "history",
                                    "rng", "stopper", "date"}


class FiveImages:
    def __len__(self):
        return 5

    def epoch(self, batch, args, shuffle=True, seed=0):
        raise AssertionError("a refused trainer must not ask for batches")


def tiny_model():
    cfg = y3d.yaml_model_load("yolov10s_3D.yaml")
    cfg.update(scales={"n": [0.33, 0.125, 1024]}, scale="n",
               channels={k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")})
    return y3d.YOLOv10_3DDetectionModel(cfg)


def test_refusals(tmp_path):
    model = tiny_model()
    with pytest.raises(Y3DError, match="HIP device"):
        train.Trainer(model, FiveImages(), epochs=2, batch=2)
    for bad in (dict(batch=0), dict(epochs=0)):
        with pytest.raises(Y3DError, match="batch = "):
            train.Trainer(model, FiveImages(), **{**dict(epochs=2, batch=2), **bad})
    # a finished run, with the reference's message; a file that is no checkpoint of this trainer
    done = {k: None for k in train.CKPT_KEYS}
    done["epoch"] = 1
    path = str(tmp_path / "last.pt")
    torch.save(done, path)
    with pytest.raises(Y3DError, match="training to 2 epochs is finished, nothing to resume"):
        train.Trainer(model, FiveImages(), epochs=2, batch=2, resume=path)
    torch.save({"model": {}}, path)
    with pytest.raises(Y3DError, match="not a checkpoint"):
        train.Trainer(model, FiveImages(), epochs=2, batch=2, resume=path)
    model.args.htl = True
    with pytest.raises(NotImplementedError, match="htl"):
        train.Trainer(model, FiveImages(), epochs=2, batch=2)


def test_accumulator_tables():
    sizes = [1, 3, 4, 5, 255, 256, 257, 1023, 16383, 16384, 16385, 40000]
    offs, total = optim.accum_layout(sizes)
    assert all(o % 4 == 0 for o in offs) and offs[0] == 0
    assert all(a + n <= b for a, n, b in zip(offs, sizes, offs[1:] + [total]))  # no two views overlap
    assert total == sum((n + 3) // 4 * 4 for n in sizes) and total % 4 == 0
    for chunk in (256, 16384):
        ct, co = optim.chunk_map(sizes, chunk)
        seen = [np.zeros(n, np.int64) for n in sizes]
        for t, c in zip(ct, co):
            assert c * chunk < sizes[t]
            seen[t][c * chunk:(c + 1) * chunk] += 1
        assert all((s == 1).all() for s in seen)  # every element once
        assert len(ct) == sum((n + chunk - 1) // chunk for n in sizes)
    # the accumulator sizes its arena from the same lists, for the parameters that take a gradient only
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in sizes[:6]] + [torch.nn.Parameter(torch.zeros(7), requires_grad=False)]
    acc = optim.GradAccumulator(ps)
    assert acc.sizes == sizes[:6] and (acc.offsets, acc.total) == optim.accum_layout(sizes[:6]) and acc.arena is None and acc.count == 0
    with pytest.raises(Y3DError, match="no parameter has a gradient"):
        acc.add()
    ps[0].grad = torch.ones(1)
    with pytest.raises(Y3DError, match="HIP device"):  # no host fallback
        acc.add()


def test_one_chunk_map_and_one_chunk_size():
    """mt.chunk_map against the double loop written out; every module's CHUNK is mt's"""
    from yolov10_3d_amd import ddp, mt, ops
    assert optim.chunk_map is mt.chunk_map
    assert ddp.FlatGradReducer.CHUNK == ops._PackRegistry.CHUNK == optim.CHUNK == mt.CHUNK == 16384
    for chunk in (256, 16384):
        for sizes in ([0], [1], [chunk - 1, chunk, chunk + 1], [3 * chunk + 5, 0, 2]):
            ct, co = [], []
            for t, n in enumerate(sizes):
                for c in range((n + chunk - 1) // chunk):
                    ct.append(t)
                    co.append(c)
            assert mt.chunk_map(sizes, chunk) == (ct, co), (sizes, chunk)
        assert mt.chunk_map([0], chunk) == ([], []) and mt.chunk_map([3 * chunk + 5, 0, 2], chunk) == ([0, 0, 0, 0, 2], [0, 1, 2, 3, 0])
    assert mt.chunk_map([16385, 1]) == ([0, 0, 1], [0, 1, 0])  # the default chunk


def test_a_checkpoints_optimizer_entry_loads_and_writes_back_without_a_device():
    """the `optimizer` entry of a trainer checkpoint, put together by hand as the trainer writes it (torch's layout + "native": the host
    step count and the counters array on the CPU), into a fresh FusedAdam over CPU parameters and out again: nothing is built before the
    first step, so no device is needed"""
    g = torch.Generator().manual_seed(11)
    shapes = [(3, 4), (5,), (2, 3)]
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    groups = [{"lr": 0.004, "weight_decay": 5e-4, "betas": (0.85, 0.99), "eps": 1e-7, "initial_lr": 0.01, "params": [0, 1]},
              {"lr": 0.002, "weight_decay": 0.0, "betas": (0.85, 0.99), "eps": 1e-7, "initial_lr": 0.005, "params": [2]}]
    state = {i: {"step": torch.tensor(7.0), "exp_avg": torch.randn(s, generator=g), "exp_avg_sq": torch.rand(s, generator=g)}
             for i, s in enumerate(shapes)}
    norm_clip = torch.arange(21, dtype=torch.float32) * 0.5  # [norm, coefficient, finite, applied, skipped] + 16 step scalars
    norm_clip[3], norm_clip[4] = 7.0, 2.0
    sd = {"state": state, "param_groups": groups, "native": {"steps": 9, "norm_clip": norm_clip.clone()}}
    opt = optim.FusedAdam([{"params": ps[:2]}, {"params": ps[2:]}], lr=0.1)
    opt.load_state_dict(sd)
    assert opt.state is None and opt.table is None
    out = opt.state_dict(torch_format=True, native=True)
    assert set(out) == {"state", "param_groups", "native"} and sorted(out["state"]) == [0, 1, 2]
    for i, e in state.items():
        assert sorted(out["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        assert all(torch.equal(out["state"][i][k], v) and out["state"][i][k].dtype == v.dtype for k, v in e.items())
    assert out["param_groups"] == groups
    assert out["native"]["steps"] == 9 and torch.equal(out["native"]["norm_clip"], norm_clip)
    assert out["native"]["norm_clip"].device.type == "cpu"
    assert set(opt.state_dict(torch_format=True)) == {"state", "param_groups"}  # the entry is opt-in
    # without the entry, torch's layout alone: the same state, the step count from torch's `step`, no counters yet
    plain = optim.FusedAdam([{"params": ps[:2]}, {"params": ps[2:]}], lr=0.1)
    plain.load_state_dict({"state": state, "param_groups": groups})
    out = plain.state_dict(torch_format=True, native=True)
    assert all(torch.equal(out["state"][i][k], v) for i, e in state.items() for k, v in e.items())
    assert out["native"] == {"steps": 0, "norm_clip": None}
