"""The training loop on the device: the accumulate kernel `y3d_mt_grad_acc` on the test's own tables, `optim.GradAccumulator`, and
`train.Trainer` (fit, checkpoints, resume, a non-finite window).

Every comparison is torch.equal: the routes compared run the same kernels on the same data in the same order, and the accumulate kernel
is one fp32 add per element, rounded once - (0 + g1) + g2 in the arena is g1 + g2 as autograd adds it.  The kernel test places every
tensor inside a sentinel-filled buffer with guard elements on both sides, accumulator and gradient each on a 16-byte boundary or one float
behind it (the 16-byte path runs only for aligned/aligned), sizes on both sides of the float4, workgroup and chunk edges, chunk 256 (the
smallest the ABI takes) and 16384 (the one the package launches)."""
import os
import random

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, ops, optim, train, val
from yolov10_3d_amd._lib import Y3DError

import stem_optim_ref as S
import tail_ref as TR
import train_ref as R
from kitti_labels_tree import fixture, write_tree

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 16383, 16384, 16385, 40000]
GUARD = 8


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------------------
class Slab:
    """tensors of SIZES inside one sentinel-filled fp32 buffer, each `shift` floats behind a 16-byte boundary, GUARD sentinels around"""

    def __init__(self, sizes, shift):
        pos, self.spans = GUARD, []
        for n in sizes:
            pos = (pos + 3) // 4 * 4 + shift
            self.spans.append((pos, n))
            pos += n + GUARD
        self.buf = TR.sentinel((pos + GUARD,), torch.float32, DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + n] for o, n in self.spans]
        assert all(v.data_ptr() % 16 == 4 * shift for v in self.views)
        gap = torch.ones(pos + GUARD, dtype=torch.bool)
        for o, n in self.spans:
            gap[o:o + n] = False
        self.gap = gap.to(DEV)
        self.ptrs = torch.tensor([v.data_ptr() for v in self.views], dtype=torch.int64, device=DEV)

    def put(self, tensors):
        for v, t in zip(self.views, tensors):
            v.copy_(t)
        return self

    def get(self):
        return [v.cpu() for v in self.views]

    def guards_intact(self):
        return bool(TR.untouched(self.buf[self.gap]).all())


def tables(sizes, chunk):
    ct, co = S.chunk_table(sizes, chunk)  # the test's own tables
    return (torch.tensor(sizes, dtype=torch.int64, device=DEV), torch.tensor(ct, dtype=torch.int32, device=DEV),
            torch.tensor(co, dtype=torch.int32, device=DEV), len(ct))


def launch(acc, grad, tb, chunk):
    y3d.lib().mt_grad_acc(acc.ptrs.data_ptr(), grad.ptrs.data_ptr(), tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], chunk,
                          ops.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("shift_g", [0, 1])
@pytest.mark.parametrize("shift_a", [0, 1])
@pytest.mark.parametrize("chunk", [256, 16384])
def test_grad_acc_kernel_adds_every_element_once(chunk, shift_a, shift_g):
    g = torch.Generator().manual_seed(100 * chunk + 10 * shift_a + shift_g)
    a0 = [torch.randn(n, generator=g) for n in SIZES]
    gr = [torch.randn(n, generator=g) * 3 for n in SIZES]
    acc, grad = Slab(SIZES, shift_a).put(a0), Slab(SIZES, shift_g).put(gr)
    tb = tables(SIZES, chunk)
    launch(acc, grad, tb, chunk)
    for t, (got, a, b) in enumerate(zip(acc.get(), a0, gr)):
        assert torch.equal(got, a + b), f"tensor {t} ({SIZES[t]} elements)"
    for t, (got, b) in enumerate(zip(grad.get(), gr)):
        assert torch.equal(got, b), f"the gradient of tensor {t} changed"
    assert acc.guards_intact() and grad.guards_intact(), "a store went outside its tensor"
    launch(acc, grad, tb, chunk)  # a second micro-batch: (a + g) + g
    for t, (got, a, b) in enumerate(zip(acc.get(), a0, gr)):
        assert torch.equal(got, (a + b) + b), f"second add, tensor {t}"
    assert acc.guards_intact() and grad.guards_intact()


def test_grad_acc_kernel_carries_inf_and_nan():
    g = torch.Generator().manual_seed(7)
    sizes = [5, 257, 16385]
    a0 = [torch.randn(n, generator=g) for n in sizes]
    gr = [torch.randn(n, generator=g) for n in sizes]
    a0[0][1], gr[0][2], gr[0][3], a0[0][3] = float("nan"), float("inf"), float("inf"), float("-inf")  # nan, inf, inf - inf = nan
    a0[1][256], gr[1][0] = float("inf"), float("-inf")
    gr[2][16384], a0[2][16383] = float("nan"), float("inf")
    acc, grad = Slab(sizes, 0).put(a0), Slab(sizes, 0).put(gr)
    launch(acc, grad, tables(sizes, 16384), 16384)
    for got, a, b in zip(acc.get(), a0, gr):
        want = a + b
        assert torch.equal(got.isnan(), want.isnan()) and bool(want.isnan().any() or want.isinf().any())
        assert torch.equal(got[~want.isnan()], want[~want.isnan()])
    assert acc.guards_intact() and grad.guards_intact()


def test_grad_acc_launcher_refusals():
    acc, grad = Slab([300], 0).put([torch.zeros(300)]), Slab([300], 0).put([torch.ones(300)])
    tb = tables([300], 256)
    L = y3d.lib()
    with pytest.raises(Y3DError, match="mt_grad_acc"):
        L.mt_grad_acc(acc.ptrs.data_ptr(), grad.ptrs.data_ptr(), tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), 0, 256, ops.stream())
    with pytest.raises(Y3DError, match="mt_grad_acc"):
        L.mt_grad_acc(acc.ptrs.data_ptr(), grad.ptrs.data_ptr(), tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), tb[3], 128, ops.stream())
    torch.cuda.synchronize()
    assert float(acc.views[0].abs().max()) == 0 and acc.guards_intact()


# ---- 2. the accumulator, on yolov10n_3D at 256 x 256, B = 2 -------------------------------------------------
def new_model(seed=3):
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(seed)
    model = y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()
    opt = optim.build_optimizer(model, lr=0.01)
    model.model[-1].restack()
    return model, opt


def snapshot(model, opt):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, opt.state.flat.cpu().clone()


def same_state(a, b, what):
    for k, v in a[0].items():
        assert torch.equal(v, b[0][k]), f"{what}: {k} differs"
    assert torch.equal(a[1], b[1]), f"{what}: the momentum buffers differ"


@pytest.fixture(scope="module")
def batches():
    from bench import synth_batch
    return [synth_batch(2, 256, 256, 40 + j, DEV) for j in range(4)]


@pytest.fixture(scope="module")
def arena_route(batches):
    """two windows of two micro-batches through GradAccumulator (made once, never changed)"""
    model, opt = new_model()
    acc = optim.GradAccumulator(model.parameters())
    out = {"items": [], "after": [], "gkeys": [], "arena_zero": []}
    for w in range(2):
        for b in batches[2 * w:2 * w + 2]:
            loss, items = model(b)
            loss.backward()
            del loss
            acc.add()
            assert all(p.grad is None for p in model.parameters())
            out["items"].append(items.float().cpu().clone())
        assert acc.count == 2
        acc.bind()
        opt.step(max_norm=10.0)
        out["gkeys"].append(list(opt.table.col["grads"].key))
        acc.reset()
        out["arena_zero"].append(float(acc.arena.abs().max()) == 0 and acc.count == 0 and all(p.grad is None for p in model.parameters()))
        out["after"].append(snapshot(model, opt))
    return out


def test_accumulator_equals_autograd_accumulation(batches, arena_route):
    model, opt = new_model()
    for w in range(2):
        for b in batches[2 * w:2 * w + 2]:
            loss, _ = model(b)
            loss.backward()  # autograd adds into the persistent p.grad, tensor by tensor
            del loss
        opt.step(max_norm=10.0)
        opt.zero_grad()
        same_state(snapshot(model, opt), arena_route["after"][w], f"window {w}")
    assert all(arena_route["arena_zero"]), "reset() must leave a zero arena, count 0 and no gradient on the parameters"
    # fixed gradient addresses: the optimizer uploads its gradient pointer table once
    assert arena_route["gkeys"][0] == arena_route["gkeys"][1]


def test_accumulated_step_differs_from_the_first_batch_alone(batches, arena_route):
    model, opt = new_model()
    loss, _ = model(batches[0])
    loss.backward()
    del loss
    opt.step(max_norm=10.0)
    opt.zero_grad()
    one = snapshot(model, opt)
    two = arena_route["after"][0]
    assert any(not torch.equal(v, two[0][k]) for k, v in one[0].items() if v.is_floating_point() and "running" not in k)
    assert not torch.equal(one[1], two[1])


def test_accumulator_on_plain_parameters_with_a_callers_uploader():
    """a parameter without a gradient stays out of the window; a non-contiguous gradient is converted; the caller's PtrUploader is used"""
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in [(5,), (64, 65), (7,), (3, 2)]]
    acc = optim.GradAccumulator(ps)
    up = optim.PtrUploader(3, DEV, depth=1)
    want = [torch.zeros(p.shape) for p in ps]
    for k in range(2):
        for i in (0, 1, 3):
            gr = torch.randn(ps[i].shape, generator=g)
            want[i] = want[i] + gr
            ps[i].grad = gr.to(DEV).t().contiguous().t() if (i == 1 and k == 1) else gr.to(DEV)
        assert k == 0 or not ps[1].grad.is_contiguous()
        acc.add(uploader=up)
    torch.cuda.synchronize()
    assert acc.count == 2 and acc._active == [0, 1, 3] and all(p.grad is None for p in ps)
    assert all(torch.equal(v.cpu(), w) for v, w in zip(acc.views, want))
    assert acc.arena.numel() == 8 + 4160 + 8 + 8 and all(v.data_ptr() % 16 == 0 for v in acc.views)
    acc.bind()
    assert ps[2].grad is None and all(ps[i].grad is acc.views[i] for i in (0, 1, 3))
    with pytest.raises(Y3DError, match="bound"):
        acc.add()
    acc.reset()
    assert float(acc.arena.abs().max()) == 0 and all(p.grad is None for p in ps)
    with pytest.raises(Y3DError, match="uploader holds 3 pointers"):
        ps[0].grad = torch.ones(5, device=DEV)
        acc.add(uploader=up)


def test_accumulator_refuses_a_changed_active_set(batches):
    model, _ = new_model()
    acc = optim.GradAccumulator(model.parameters())
    loss, _ = model(batches[0])
    loss.backward()
    del loss
    acc.add()
    loss, _ = model(batches[1])
    loss.backward()
    del loss
    before = acc.arena.clone()
    acc.params[5].grad = None
    with pytest.raises(Y3DError, match="active set"):
        acc.add()
    torch.cuda.synchronize()
    assert torch.equal(acc.arena, before) and acc.count == 1, "the refusal comes before the launch"
    with pytest.raises(Y3DError, match="nothing was added"):
        optim.GradAccumulator(model.parameters()).bind()


# ---- 4. / 5. Trainer.fit on the KITTI tree at 320 x 256 --------------------------------------------------------------------------------------
RES = (320, 256)
FIT = dict(epochs=2, batch=2, nbs=4, warmup_epochs=0, optimizer="SGD", lr0=0.01)
FRAMES = 5


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


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    z = fixture()
    z5 = {k: z[k][:FRAMES] for k in ("label_text", "calib_text", "frame_wh")}
    root = write_tree(str(tmp_path_factory.mktemp("train_tree")), z5, images=True)
    return root, kitti.DeviceSplit(root, device=DEV), kitti.DeviceSplit(root, mode="val", device=DEV)


def validator_factory(val_split):
    return lambda m: val.Validator3d(m, val_split, batch=4, plots=False, resolution=RES)


def run_state(t):
    torch.cuda.synchronize()
    return {"model": {k: v.detach().cpu().clone() for k, v in t.model.state_dict().items()},
            "ema": {k: v.detach().cpu().clone() for k, v in t.ema.ema.state_dict().items()},
            "opt": t.opt.state.flat.cpu().clone(), "counters": t.opt.state.norm_clip.cpu().clone(), "updates": t.ema.updates,
            "best_fitness": t.best_fitness, "history": [dict(h) for h in t.history]}


def same_run(a, b, what, history=True):
    for part in ("model", "ema"):
        for k, v in a[part].items():
            assert torch.equal(v, b[part][k]), f"{what}: {part} {k} differs"
    assert torch.equal(a["opt"], b["opt"]), f"{what}: optimizer state differs"
    assert a["updates"] == b["updates"] and a["best_fitness"] == b["best_fitness"], what
    if history:
        assert a["history"] == b["history"], f"{what}: history differs"


@pytest.fixture(scope="module")
def straight(tree, tmp_path_factory):
    root, sp, vsp = tree
    save_dir = str(tmp_path_factory.mktemp("straight"))
    model, _ = new_model()
    t = train.Trainer(model, Split320(sp), validator_factory(vsp), save_dir=save_dir, **FIT)
    t.fit()
    return run_state(t), save_dir


def test_fit_equals_the_loop_written_out(tree, straight):
    root, sp, vsp = tree
    got, save_dir = straight
    model, _ = new_model()
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    opt = optim.build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=0.0005 * 2 * 2 / 4, iterations=4, device_momentum=True)
    ema = optim.ModelEMA(model)
    ema.ema.model[-1].restack()  # before the first update: the validator's forward must not re-point the copy's buffers later
    sched = optim.Schedule(opt, 2, 3, lrf=0.01, warmup_epochs=0, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=4, batch=2)
    acc = optim.GradAccumulator(model.parameters())
    validator = validator_factory(vsp)(ema.ema)
    rows = R.do_train_rows(FRAMES, 2, 2, 4, 0)
    assert [r[4] for r in rows] == [False, True, False, True, False, True]
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
        assert b["img"].shape[0] == 1  # the short last batch
        validator()
        history.append(dict(zip(names, (float(v) for v in tloss.cpu()))))
        sched.epoch_end(epoch)
    torch.cuda.synchronize()
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), got["model"][k]), f"model {k}"
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v.cpu(), got["ema"][k]), f"EMA {k}"
    assert torch.equal(opt.state.flat.cpu(), got["opt"]) and ema.updates == got["updates"] == 3
    for h, g in zip(history, got["history"]):
        assert all(g[k] == v and np.isfinite(v) for k, v in h.items()), (h, g)
    assert [h["epoch"] for h in got["history"]] == [0, 1] and all("fitness" in h and "lr/pg0" in h and "metrics/3D" in h for h in got["history"])


def test_fit_writes_its_files_and_validate_loads_them(tree, straight, capsys):
    root, sp, vsp = tree
    want, save_dir = straight
    for f in ("results.csv", "weights/last.pt", "weights/best.pt"):
        assert os.path.exists(os.path.join(save_dir, f)), f
    lines = open(os.path.join(save_dir, "results.csv")).read().splitlines()
    assert len(lines) == 3 and lines[0].split(",")[0].strip() == "epoch" and "train/box_om" in lines[0] and "lr/pg2" in lines[0]
    ck = torch.load(os.path.join(save_dir, "weights", "last.pt"), map_location="cpu", weights_only=False)
    assert set(ck) == set(train.CKPT_KEYS) and ck["epoch"] == 1 and ck["updates"] == 3
    assert all(v.dtype == torch.float32 for v in ck["ema"].values() if v.is_floating_point())
    assert set(ck["optimizer"]) == {"state", "param_groups", "native"} and "momentum_buffer" in ck["optimizer"]["state"][0]
    # tools/validate.py's loader takes the file
    import importlib.util
    spec = importlib.util.spec_from_file_location("y3d_tools_validate", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "validate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["yolov10n_3D.yaml", "--weights", os.path.join(save_dir, "weights", "last.pt"), "--data", root, "--batch", "5", "--no-plots"])
    out = capsys.readouterr().out
    n = len(ck["ema"])
    assert f"loaded {n} of {n} tensors" in out


def test_resume_continues_bit_for_bit(tree, straight, tmp_path):
    root, sp, vsp = tree
    want, _ = straight
    save_dir = str(tmp_path / "interrupted")
    model, _ = new_model()
    t = train.Trainer(model, Split320(sp, stop_at=1), validator_factory(vsp), save_dir=save_dir, **FIT)
    with pytest.raises(Interrupted):
        t.fit()
    last = os.path.join(save_dir, "weights", "last.pt")
    assert torch.load(last, map_location="cpu", weights_only=False)["epoch"] == 0
    model, _ = new_model(seed=11)  # other weights: everything comes from the file
    t = train.Trainer(model, Split320(sp), validator_factory(vsp), resume=last, **FIT)
    assert t.start_epoch == 1
    t.fit()
    got = run_state(t)
    same_run(got, want, "resumed against straight")
    assert torch.equal(got["counters"][2:5], want["counters"][2:5]), "steps applied / skipped"
    with pytest.raises(Y3DError, match="finished, nothing to resume"):
        train.Trainer(model, Split320(sp), resume=os.path.join(straight[1], "weights", "last.pt"), **FIT)


class ListSplit:
    """resident batches served in order"""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return sum(b["img"].shape[0] for b in self.batches)

    def epoch(self, batch, args, shuffle=True, seed=0):
        return iter(self.batches)


def test_fit_without_accumulation_makes_no_arena(batches):
    """nbs = batch: every micro-batch is a step, the trainer builds no accumulator and equals plain steps"""
    model, _ = new_model()
    t = train.Trainer(model, ListSplit(batches[:3]), None, epochs=1, batch=2, nbs=2, warmup_epochs=0, optimizer="SGD", lr0=0.01)
    assert t.accum is None and all(r[3] == 1 and r[4] for r in t.plan)
    t.fit()
    got = snapshot(model, t.opt)
    assert t.ema.updates == 3 and t.fitness is None and len(t.history) == 1
    model, _ = new_model()
    opt = optim.build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=0.0005 * 2 * 1 / 2, iterations=3, device_momentum=True)
    optim.Schedule(opt, 1, 3, lrf=0.01, warmup_epochs=0, nbs=2, batch=2)
    for b in batches[:3]:
        loss, _ = model(b)
        loss.backward()
        del loss
        opt.step(max_norm=10.0)
        opt.zero_grad()
    same_state(got, snapshot(model, opt), "accumulate 1")


# ---- 6. a window with a non-finite micro-batch ---------------------------------------------------------------------------------------------
def test_a_non_finite_window_is_skipped_and_leaves_no_trace(batches):
    bad = dict(batches[0], img=batches[0]["img"].clone())
    bad["img"][1, :, 100:110, 50:60] = float("nan")

    def window(model, opt, ema, acc, pair):
        for b in pair:
            loss, _ = model(b)
            loss.backward()
            del loss
            acc.add()
        acc.bind()
        opt.step(max_norm=10.0)
        acc.reset()
        ema.update(model, guard=opt.last_norm)

    model, opt = new_model()
    ema, acc = optim.ModelEMA(model), optim.GradAccumulator(model.parameters())
    p0 = [p.detach().clone() for p in model.parameters()]
    e0 = [p.detach().clone() for p in ema.ema.parameters()]
    window(model, opt, ema, acc, [bad, batches[1]])
    torch.cuda.synchronize()
    nc = opt.last_norm.cpu()
    assert float(nc[4]) == 1 and float(nc[3]) == 0 and float(nc[2]) == 0 and not np.isfinite(float(nc[0]))
    assert all(torch.equal(a, b) for a, b in zip(p0, model.parameters())), "a skipped step moved a parameter"
    assert all(torch.equal(a, b) for a, b in zip(e0, ema.ema.parameters())), "the EMA followed a skipped step"
    assert float(acc.arena.abs().max()) == 0 and acc.count == 0, "reset() must clear the non-finite sums"
    window(model, opt, ema, acc, batches[2:4])
    got = snapshot(model, opt)
    got_ema = [p.detach().cpu().clone() for p in ema.ema.parameters()]
    assert float(opt.last_norm[3]) == 1 and all(bool(torch.isfinite(p).all()) for p in model.parameters())

    # the same forwards (BatchNorm sees the same batches) without the bad window's gradients
    model, opt = new_model()
    ema, acc = optim.ModelEMA(model), optim.GradAccumulator(model.parameters())
    for b in (bad, batches[1]):
        loss, _ = model(b)
        del loss
    ema.updates += 1  # the skipped update counted
    window(model, opt, ema, acc, batches[2:4])
    want = snapshot(model, opt)
    for k, v in want[0].items():
        assert torch.equal(v, got[0][k]) or (v.is_floating_point() and torch.equal(v.isnan(), got[0][k].isnan())
                                             and torch.equal(v.nan_to_num(0.0), got[0][k].nan_to_num(0.0))), f"{k} differs"
    assert torch.equal(want[1], got[1]), "momentum buffers differ"
    assert all(torch.equal(a, b.detach().cpu()) for a, b in zip(got_ema, ema.ema.parameters()))
