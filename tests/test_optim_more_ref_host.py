"""CPU: the restatements of optim_more_ref.py against torch.optim in float64 (single-tensor path), their float32 forms against the bounds
the device is held to, optim.Schedule against np.interp + torch's LambdaLR, the torch-format state conversion of optim.py against real
torch.optim state dicts, build_optimizer's names, and the coverage that test_hip_optim_more.py's case lists claim."""
import math
import warnings

import numpy as np
import pytest
import torch

import optim_more_ref as M
import test_hip_optim_more as G
from yolov10_3d_amd import optim as O
from yolov10_3d_amd._lib import Y3DError

f32 = lambda x: float(np.float32(x))
KINDS = [M.ADAM, M.ADAMAX, M.NADAM, M.RADAM, M.RMSPROP]
KIND_IDS = [M.NAMES[k] for k in KINDS]
N = 1000


def _rand(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


def _torch_opt(kind, tp, lr, wd, b1, b2, eps, momentum):
    kw = dict(lr=lr, weight_decay=wd, foreach=False)
    if kind == M.RMSPROP:
        return torch.optim.RMSprop([tp], alpha=b2, eps=eps, momentum=momentum, centered=False, **kw)
    cls = {M.ADAM: torch.optim.Adam, M.ADAMAX: torch.optim.Adamax, M.NADAM: torch.optim.NAdam, M.RADAM: torch.optim.RAdam}[kind]
    extra = {"momentum_decay": 4e-3} if kind == M.NADAM else {}
    return cls([tp], betas=(b1, b2), eps=eps, **extra, **kw)


@pytest.fixture
def float64_default():
    """torch.optim.NAdam keeps mu_product in the default dtype: float64 for the comparison in float64"""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


VS_TORCH = [(k, 0.0, wd) for k in KINDS for wd in (0.0, 5e-4)] + [(M.RMSPROP, 0.9, wd) for wd in (0.0, 5e-4)]


@pytest.mark.parametrize("kind,momentum,wd", VS_TORCH, ids=[f"{M.NAMES[k]}-mom{m}-wd{w}" for k, m, w in VS_TORCH])
def test_update_f64_vs_torch_optim(kind, momentum, wd, float64_default):
    """eight consecutive steps; RAdam takes the unrectified arm first and the rectified one later"""
    lr, wd, b1, eps, momentum = (f32(x) for x in (0.002, wd, 0.9, 1e-8, momentum))
    b2 = f32(0.99) if kind == M.RMSPROP else f32(0.999)
    p0 = _rand(N, 1)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = _torch_opt(kind, tp, lr, wd, b1, b2, eps, momentum)
    p, a, b = p0.astype(np.float64), np.zeros(N), np.zeros(N)
    mp, arms = 1.0, []
    for t in range(1, 9):
        g = _rand(N, 30 + t, 0.3)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        scal = M.step_scalars_f64(b1, b2, t, mp, state_dt=np.float64)
        mp = scal[M.MU_PROD]
        arms.append(int(scal[M.RECT_ON]))
        p, a, b = M.UPDATE_F64[kind](p, g, a, b, lr, wd, b1, b2, eps, scal, 1.0, momentum)
        st = opt.state[tp]
        assert float(st["step"]) == t
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-12 * np.abs(p).max(), f"{M.NAMES[kind]} step {t}: parameters"
        keys = O.TORCH_STATE[M.NAMES[kind]][0]
        for arr, key in zip((a, b), keys):
            if key in st:
                ref = st[key].detach().numpy()
                assert np.abs(arr - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), f"{M.NAMES[kind]} step {t}: {key}"
        if kind == M.NADAM:
            assert abs(mp - float(st["mu_product"])) <= 1e-15
    if kind == M.RADAM:
        # rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t) > 5 decides; from the restatement: unrectified for t <= 5, rectified from t = 6
        assert arms == [0, 0, 0, 0, 0, 1, 1, 1], arms
        rho_inf = 2 / (1 - b2) - 1
        assert [int(rho_inf - 2 * t * b2 ** t / (1 - b2 ** t) > 5) for t in range(1, 9)] == arms


def test_step_scalars_fp32_state_is_the_only_difference_to_the_float64_rule():
    """mu_product as fp32 state moves the product by at most 2^-24 relative per step; every other entry does not depend on it"""
    b1, b2 = f32(0.9), f32(0.999)
    mp32 = mp64 = 1.0
    for t in range(1, 9):
        s32 = M.step_scalars_f64(b1, b2, t, mp32)
        s64 = M.step_scalars_f64(b1, b2, t, mp64, state_dt=np.float64)
        mp32, mp64 = float(np.float32(s32[M.MU_PROD])), s64[M.MU_PROD]
        assert abs(mp32 - mp64) <= t * 2.0 ** -24 * mp64
        free = [i for i in range(M.NSCAL) if i not in (M.MU_PROD, M.MU_PROD_NEXT, M.NADAM_G, M.NADAM_M)]
        assert np.array_equal(s32[free], s64[free])
        assert s32[M.BC1] == 1 - b1 ** t and s32[M.BC2_SQRT] == math.sqrt(1 - b2 ** t) and s32[M.T] == t
    first = M.step_scalars_f32(b1, b2, 1, 123.0)  # the state before the first applied step is not read
    assert first[M.MU_PROD] == np.float32(b1 * (1 - 0.5 * 0.96 ** 4e-3))


@pytest.mark.parametrize("nesterov", [1, 0])
@pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["wd0", "wd5e-4"])
def test_sgd_f64_with_a_momentum_per_step_vs_torch_optim(nesterov, wd):
    lr, wd = f32(0.013), f32(wd)
    p0 = _rand(N, 3)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=0.5, nesterov=bool(nesterov), weight_decay=wd, foreach=False)
    p, b = p0.astype(np.float64), np.zeros(N)  # zero buffer, first = 0: torch's first step buf = clone(g)
    for t in range(8):
        mom = f32(np.interp(t, [0, 7], [0.8, 0.937]))
        opt.param_groups[0]["momentum"] = mom
        g = _rand(N, 50 + t)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, b = M.sgd_f64(p, g, b, lr, wd, mom, nesterov, 0)
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-14 * np.abs(p).max()
        assert np.abs(b - opt.state[tp]["momentum_buffer"].numpy()).max() <= 1e-14 * np.abs(b).max()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_float32_restatements_fit_the_bounds_the_device_is_held_to(kind):
    """from the same fp32 inputs and fp32 step scalars: first step (zero state), later steps, both RAdam arms, wd zero and not, the
    clip coefficient, RMSprop with and without momentum, zero gradients on non-zero state"""
    b1, eps = 0.9, 1e-8
    b2 = 0.99 if kind == M.RMSPROP else 0.999
    worst = 0.0
    for case, (t, wd, coef, mom) in enumerate([(1, 0.0, 1.0, 0.9), (1, 5e-4, 0.37, 0.0), (3, 5e-4, 1.0, 0.9), (5, 0.0, 0.37, 0.0),
                                               (6, 5e-4, 1.0, 0.9), (8, 0.0, 0.5, 0.85), (200, 5e-4, 1.0, 0.9)]):
        scal = M.step_scalars_f32(b1, b2, t, 0.4)
        p, g = _rand(N, 100 + case), _rand(N, 200 + case, 0.5)
        if t == 1:
            a, b = np.zeros(N, np.float32), np.zeros(N, np.float32)
        else:
            a = _rand(N, 300 + case, 0.1)
            b = np.abs(_rand(N, 400 + case, 0.05)) if kind != M.RMSPROP else _rand(N, 400 + case, 0.05)
            if kind == M.RMSPROP:
                a = np.abs(a)
        if case == 3:
            g[::3] = 0
        args = (p, g, a, b, 0.01, wd, b1, b2, eps, scal, coef, mom)
        got, ref, tol = M.UPDATE_F32[kind](*args), M.UPDATE_F64[kind](*args), M.update_bound(kind, *args)
        for x, r, tl, name in zip(got, ref, tol, "pab"):
            assert x.dtype == np.float32
            ratio = float((np.abs(x.astype(np.float64) - r) / tl).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{M.NAMES[kind]} case {case} {name}: {ratio:.3g} x the bound"
    print(f"{M.NAMES[kind]}: largest fp32 error {worst:.3g} x the bound")
    assert worst > 1e-3, "a bound a thousand times wider than any error checks nothing"


# ----------------------------------------------------------------------------------------------------------------------- Schedule


def _groups(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g).requires_grad_(True) for n in (3, 4, 5)]
    return [{"params": [ps[0]], "weight_decay": 0.0}, {"params": [ps[1]], "weight_decay": 5e-4}, {"params": [ps[2]], "weight_decay": 0.0}]


@pytest.mark.parametrize("nw", [5, None], ids=["nw5-below-nb", "nw100-above-nb"])
@pytest.mark.parametrize("cos_lr", [False, True], ids=["linear", "cosine"])
def test_schedule_equals_interp_plus_lambdalr(cos_lr, nw):
    """the reference's loop (engine/trainer.py:217-223, 332, 384-393, 468-470) on a torch SGD, every iteration of 5 epochs x 7 batches"""
    epochs, nb, lrf, wm, wbl, nbs, batch, mom, lr0 = 5, 7, 0.01, 0.8, 0.1, 64, 16, 0.937, 0.01
    ref = torch.optim.SGD(_groups(), lr=lr0, momentum=mom, nesterov=True)
    if cos_lr:
        lf = lambda x: max((1 - math.cos(x * math.pi / epochs)) / 2, 0) * (lrf - 1) + 1
    else:
        lf = lambda x: max(1 - x / epochs, 0) * (1.0 - lrf) + lrf
    sched = torch.optim.lr_scheduler.LambdaLR(ref, lr_lambda=lf)
    ours = O.FusedSGD(_groups(), lr=lr0, momentum=mom, nesterov=True, device_momentum=True)
    S = O.Schedule(ours, epochs, nb, lrf, cos_lr, 3.0, wm, wbl, nbs, batch)
    assert S.nw == max(round(3.0 * nb), 100) == 100
    if nw is not None:
        S.nw = nw
    nw = S.nw
    accumulate = max(round(nbs / batch), 1)
    seen_warm = seen_after = False
    for epoch in range(epochs):
        for i in range(nb):
            ni = i + nb * epoch
            if ni <= nw:
                xi = [0, nw]
                accumulate = max(1, int(np.interp(ni, xi, [1, nbs / batch]).round()))
                for j, x in enumerate(ref.param_groups):
                    x["lr"] = np.interp(ni, xi, [wbl if j == 0 else 0.0, x["initial_lr"] * lf(epoch)])
                    if "momentum" in x:
                        x["momentum"] = np.interp(ni, xi, [wm, mom])
                seen_warm = True
            else:
                seen_after = True
            S.iteration(ni, epoch)
            assert S.accumulate(ni) == accumulate
            for j, (x, y) in enumerate(zip(ref.param_groups, ours.param_groups)):
                assert float(x["lr"]) == y["lr"] and float(x["momentum"]) == y["momentum"], (epoch, i, j, x["lr"], y["lr"])
                assert x["initial_lr"] == y["initial_lr"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched.last_epoch = epoch
            sched.step()
        S.epoch_end(epoch)
        for x, y in zip(ref.param_groups, ours.param_groups):
            assert float(x["lr"]) == y["lr"]
    assert seen_warm and seen_after == (nw < epochs * nb - 1)
    # no "momentum" key (device_momentum=False): the reference's `if "momentum" in x` skips the group, and so does Schedule
    plain = O.FusedSGD(_groups(), lr=lr0, momentum=mom)
    O.Schedule(plain, epochs, nb, lrf, cos_lr, 3.0, wm, wbl, nbs, batch).iteration(1, 0)
    assert all("momentum" not in g for g in plain.param_groups) and plain.momentum == mom


# ------------------------------------------------------------------------------------------------------------- torch-format state

TORCH_CLS = {"SGD": (torch.optim.SGD, dict(lr=0.01, momentum=0.9, nesterov=True)), "AdamW": (torch.optim.AdamW, dict(lr=0.002)),
             "Adam": (torch.optim.Adam, dict(lr=0.002)), "Adamax": (torch.optim.Adamax, dict(lr=0.002)),
             "NAdam": (torch.optim.NAdam, dict(lr=0.002)), "RAdam": (torch.optim.RAdam, dict(lr=0.002)),
             "RMSprop": (torch.optim.RMSprop, dict(lr=0.01, momentum=0.9))}
SHAPES = [(7,), (3, 5), (2, 3, 2, 2), (1,)]


def _real_state_dict(name, steps=3, skip_param=None):
    g = torch.Generator().manual_seed(5)
    ps = [torch.randn(sh, generator=g).requires_grad_(True) for sh in SHAPES]
    cls, kw = TORCH_CLS[name]
    opt = cls([{"params": ps[:2]}, {"params": ps[2:], "weight_decay": 5e-4}], **kw)
    for _ in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if i == skip_param else torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict()


@pytest.mark.parametrize("name", sorted(TORCH_CLS))
def test_torch_state_round_trips_bit_for_bit(name):
    sd = _real_state_dict(name)
    flat, step, mu, present = O.torch_state_to_flat(name, sd["state"], SHAPES)
    assert present == [0, 1, 2, 3] and flat.shape == (len(O.TORCH_STATE[name][0]), sum(int(np.prod(s)) for s in SHAPES))
    assert step == (None if name == "SGD" else 3.0) and (mu is not None) == (name == "NAdam")
    back = O.flat_to_torch_state(name, flat, SHAPES, present, step, mu)
    assert sorted(back) == sorted(sd["state"])
    for i, e in sd["state"].items():
        assert sorted(back[i]) == sorted(e), (sorted(back[i]), sorted(e))
        for k, v in e.items():
            w = back[i][k]
            assert w.dtype == v.dtype and w.shape == v.shape and torch.equal(w, v), f"{name} parameter {i} {k}"
    # a parameter that never had a gradient has no entry: it loads as zeros and is not listed
    sd = _real_state_dict(name, skip_param=1)
    assert 1 not in sd["state"]
    flat, _, _, present = O.torch_state_to_flat(name, sd["state"], SHAPES)
    assert present == [0, 2, 3] and not flat[:, 7:22].any() and flat[0, :7].any()
    assert sorted(O.flat_to_torch_state(name, flat, SHAPES, present, 3.0, mu)) == [0, 2, 3]


def test_torch_state_refuses_bad_input():
    sd = _real_state_dict("Adam")
    bad = {i: dict(e) for i, e in sd["state"].items()}
    bad[2]["step"] = torch.tensor(7.0)
    with pytest.raises(Y3DError, match=r"parameter 2: step 7.*one\s+device-side step count"):
        O.torch_state_to_flat("Adam", bad, SHAPES)
    bad = {i: dict(e) for i, e in sd["state"].items()}
    bad[1]["exp_avg_sq"] = torch.zeros(4, 5)
    with pytest.raises(Y3DError, match=r"parameter 1: exp_avg_sq has 20 elements, the parameter 15"):
        O.torch_state_to_flat("Adam", bad, SHAPES)
    for other, mine in (("SGD", "Adam"), ("Adam", "SGD"), ("Adamax", "Adam"), ("Adam", "RMSprop"), ("RMSprop", "Adamax")):
        with pytest.raises(Y3DError, match=rf"parameter 0 has keys .* not the state of {mine}"):
            O.torch_state_to_flat(mine, _real_state_dict(other)["state"], SHAPES)
    nadam = _real_state_dict("NAdam")["state"]
    nadam[3]["mu_product"] = torch.tensor(0.5)
    with pytest.raises(Y3DError, match="parameter 3: mu_product"):
        O.torch_state_to_flat("NAdam", nadam, SHAPES)


# ------------------------------------------------------------------------------------------------------------------ build_optimizer


def test_build_optimizer_names_groups_and_auto():
    """every name build_optimizer takes, "auto" on both sides of 10 000 iterations.  "RMSProp" is the one name of the reference's list it
    does not take (tests/test_host_logic.py pins that it raises): the reference's RMSProp is FusedRMSprop over reference_groups()"""
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 2, 1, bias=False))
    model.nc = 3
    want = {"SGD": O.FusedSGD, "AdamW": O.FusedAdamW, "Adam": O.FusedAdam, "Adamax": O.FusedAdamax, "NAdam": O.FusedNAdam, "RAdam": O.FusedRAdam}
    for name, cls in want.items():
        opt = O.build_optimizer(model, lr=0.01, momentum=0.9, decay=5e-4, name=name)
        assert type(opt) is cls and opt.auto is None
        assert [len(g["params"]) for g in opt.param_groups] == [2, 2, 1] and [g["weight_decay"] for g in opt.param_groups] == [0.0, 5e-4, 0.0]
        assert "momentum" not in opt.param_groups[0]
    rms = O.FusedRMSprop(O.reference_groups(model, 5e-4), lr=0.01, momentum=0.9)
    assert [len(g["params"]) for g in rms.param_groups] == [2, 2, 1] and [g["weight_decay"] for g in rms.param_groups] == [0.0, 5e-4, 0.0]
    assert all(g["momentum"] == 0.9 and g["lr"] == 0.01 for g in rms.param_groups)
    assert [[id(p) for p in g["params"]] for g in rms.param_groups] == [[id(p) for p in g["params"]] for g in opt.param_groups]
    assert "momentum" in O.build_optimizer(model, name="SGD", device_momentum=True).param_groups[2]
    long = O.build_optimizer(model, lr=0.5, momentum=0.5, name="auto", iterations=10001)
    assert type(long) is O.FusedSGD and long.momentum == 0.9 and long.param_groups[0]["lr"] == 0.01 and long.nesterov
    assert long.auto == {"name": "SGD", "lr": 0.01, "momentum": 0.9, "warmup_bias_lr": 0.0}
    short = O.build_optimizer(model, lr=0.5, momentum=0.5, name="auto", iterations=10000)
    lr_fit = round(0.002 * 5 / (4 + 3), 6)
    assert type(short) is O.FusedAdamW and short.betas == (0.9, 0.999) and short.param_groups[1]["lr"] == lr_fit
    assert short.auto == {"name": "AdamW", "lr": lr_fit, "momentum": 0.9, "warmup_bias_lr": 0.0}
    with pytest.raises(NotImplementedError, match="Optimizer 'Lion' not found in list of available optimizers"):
        O.build_optimizer(model, name="Lion")


# ------------------------------------------------------------------------------------------------------------------------ coverage


def test_gpu_case_lists_reach_every_branch():
    """from the lists of test_hip_optim_more.py themselves: wd zero and non-zero, both RAdam arms, the first step, a skipped step, a
    clipped step, RMSprop tensors with and without momentum, tensors on the 16-byte path and off it, both chunk sizes"""
    ts = [t for t in G.PLAN if t is not None]
    assert None in G.PLAN and G.PLAN[0] == 1 and G.PLAN.index(None) > 0
    arms = {int(M.step_scalars_f64(G.HP[0], G.HP[1], t)[M.RECT_ON]) for t in ts}
    assert arms == {0, 1}
    assert any(c != 1.0 for c in G.COEF.values()) and any(G.COEF.get(t, 1.0) == 1.0 for t in ts)
    for chunk in (256, 16384):
        n = len(G.O.SIZES[chunk])
        _, wd = G.O.hyper(n)
        assert 0.0 in wd and any(w != 0 for w in wd)
        mom = G.momenta(n)
        assert 0.0 in mom and any(m > 0 for m in mom)
    assert {c for c, _ in G.CFG} == {256, 16384}
    # Arena: tensor i starts at element offset (i + rot) mod 4 of a 16-byte aligned buffer
    aligned_all = [all((i + r) % 4 == 0 for r in rots) for chunk, rots in G.CFG for i in range(len(G.O.SIZES[chunk]))]
    assert any(aligned_all) and not all(aligned_all), "tensors on the 16-byte path and tensors off it"
    assert any(len(set(rots)) > 1 for _, rots in G.CFG), "arenas whose alignments differ: the mixed case takes the scalar path"
