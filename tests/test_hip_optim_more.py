"""The optimizer kernels added beside mt_sgd / mt_adamw (csrc/optim.hip) through the C ABI with the test's own tables - y3d_mt_step_scalars,
y3d_mt_update (Adam, Adamax, NAdam, RAdam, RMSprop), y3d_mt_sgd_tab - and what optim.py builds on them: FusedAdam / FusedAdamax /
FusedNAdam / FusedRAdam / FusedRMSprop, FusedSGD(device_momentum=True), build_optimizer's names, torch-format checkpoints, captured steps.

* sizes, arenas, sentinels and chunk tables are test_hip_optim.py's (chunk 256 and 16384, sizes on both sides of every chunk edge,
  starts at element offsets 0..3 mod 4, gaps checked after every launch).  The update kernels take 16-byte accesses only when all of
  a tensor's pointers allow: CFG rotates the four arenas together (some tensors on the vector path, some off it) and apart;
* every update kernel, with the step-scalar array supplied by the test, is held to BIT equality with its float32 restatement
  (optim_more_ref.py: one float32 operation per kernel operation; the build uses -ffp-contract=off) and to float64 within the bound
  derived there from the operation count;
* y3d_mt_step_scalars: every value is the float64 restatement rounded to float32, or one float32 ulp from it (the device's double pow /
  sqrt are not correctly rounded; after one rounding nothing wider is admissible).
tests/test_optim_more_ref_host.py pins the restatements to torch.optim on the CPU and checks the coverage of the lists below."""
import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import Y3DError

import optim_more_ref as M
import tail_ref as R
import test_hip_optim as O
from test_hip_eval_tail import assert_bits

DEV = "cuda"
F = np.float32
KINDS = [M.ADAM, M.ADAMAX, M.NADAM, M.RADAM, M.RMSPROP]
KIND_IDS = [M.NAMES[k] for k in KINDS]
# (chunk, rotations of the start offsets of the parameter, gradient and two state arenas)
CFG = [(256, (0, 0, 0, 0)), (256, (1, 1, 1, 1)), (256, (0, 1, 2, 3)), (16384, (2, 2, 2, 2)), (16384, (0, 0, 1, 0))]
CFG_IDS = [f"chunk{c}-rot{''.join(map(str, r))}" for c, r in CFG]
HP = (0.9, 0.999, 1e-8)
# applied-step count of each launch (None: a skipped step - finite flag 0): the first step on zero state, RAdam's unrectified arm up
# to t = 5 and its rectified arm from t = 6
PLAN = [1, 2, None, 5, 6, 7]
COEF = {2: 0.37, 6: 0.81}  # clip coefficient of a step (others 1)


def momenta(n):
    """RMSprop's per-tensor momentum table: every fourth tensor without momentum"""
    return [0.0 if t % 4 == 1 else 0.8 + 0.01 * t for t in range(n)]


def _zeros(sizes):
    return [np.zeros(n) for n in sizes]


# ---- y3d_mt_update ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rots", CFG, ids=CFG_IDS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_update_bit_for_bit_and_float64_bound(kind, chunk, rots):
    """PLAN's launches from the device's own pre-step state: bit equality with UPDATE_F32 and the float64 bound of update_bound, the
    step scalars supplied by the test.  Measured on the device: bit-identical on every element; the largest distance from float64 is
    0.91 - 0.995 of the bound (the half ulp of the final subtraction is a tight term of it)."""
    L, st = y3d.lib(), ops.stream()
    sizes = O.SIZES[chunk]
    rng = np.random.default_rng(chunk + 7 * kind + sum(r << (2 * i) for i, r in enumerate(rots)))
    tb = O.Tables(sizes, chunk)
    b1, b2, eps = HP if kind != M.RMSPROP else (0.0, 0.99, 1e-8)
    mom_h = momenta(len(sizes))
    mom = torch.tensor(mom_h, dtype=torch.float32, device=DEV)
    ap, ag, aa, ab = (O.Arena(sizes, r) for r in rots)
    ap.put(O.rand_list(sizes, rng))
    aa.put(_zeros(sizes)), ab.put(_zeros(sizes))
    sbuf, scal = O.guarded_out(M.NSCAL)
    what = f"mt_update {M.NAMES[kind]} chunk={chunk} rots={rots}"
    worst, mp = 0.0, 1.0
    for t in PLAN:
        g = O.rand_list(sizes, rng, 0.5)
        if t == 5:
            g[2][:] = 0  # zero gradients on a tensor whose state is not zero
        ag.put(g)
        pre = (ap.get(), aa.get(), ab.get())
        if t is None:
            clip = torch.tensor([float("nan"), float("nan"), 0.0, 2.0, 1.0], device=DEV)
            sc_h = None
        else:
            coef = COEF.get(t, 1.0)
            sc_h = M.step_scalars_f32(b1, b2, t, mp)
            mp = float(sc_h[M.MU_PROD])
            scal.copy_(torch.from_numpy(sc_h))
            clip = torch.tensor([5.0, coef, 1.0, float(t), 0.0], device=DEV) if t != 1 else None  # the first launch: null clip pointer
        L.mt_update(kind, ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), aa.ptrs.data_ptr(), ab.ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(),
                    tb.wd.data_ptr(), mom.data_ptr() if kind == M.RMSPROP else None, tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, chunk, b1, b2, eps,
                    None if kind == M.RMSPROP else scal.data_ptr(), clip.data_ptr() if clip is not None else None, st)
        torch.cuda.synchronize()
        for a in (ap, ag, aa, ab):
            a.check_gaps(what)
        assert bool(R.untouched(sbuf[M.NSCAL:]).all())
        post = (ap.get(), aa.get(), ab.get())
        O.same_bits(ag.get(), g, f"{what} t={t}: the gradients must not change")
        if t is None:
            for k, name in enumerate(("p", "state 0", "state 1")):
                O.same_bits(post[k], pre[k], f"{what} skipped step {name}")
            continue
        for i in range(len(sizes)):
            args = (pre[0][i], g[i], pre[1][i], pre[2][i], tb.lr_h[i], tb.wd_h[i], b1, b2, eps, sc_h, COEF.get(t, 1.0), mom_h[i])
            ref, tol = M.UPDATE_F64[kind](*args), M.update_bound(kind, *args)
            for k, name in enumerate(("p", "state 0", "state 1")):
                ratio = float((np.abs(post[k][i].astype(np.float64) - ref[k]) / tol[k]).max())
                assert ratio <= 1.0, f"{what} t={t} tensor {i} {name}: {ratio:.3g} x the float64 bound"
                worst = max(worst, ratio)
        want = [M.UPDATE_F32[kind](pre[0][i], g[i], pre[1][i], pre[2][i], tb.lr_h[i], tb.wd_h[i], b1, b2, eps, sc_h, COEF.get(t, 1.0), mom_h[i])
                for i in range(len(sizes))]
        for k, name in enumerate(("p", "state 0", "state 1")):
            O.same_bits(post[k], [w[k] for w in want], f"{what} t={t} {name}")
    print(f"{what}: largest error {worst:.3g} x the float64 bound")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rots", [(256, (0, 0, 0)), (256, (1, 2, 3)), (16384, (3, 3, 3))], ids=["chunk256-rot000", "chunk256-rot123", "chunk16384-rot333"])
def test_sgd_tab_bit_for_bit(chunk, rots):
    """mt_sgd's rule with a per-tensor momentum: Nesterov and plain, a first step over a NaN-filled buffer, clipped, then skipped"""
    L, st = y3d.lib(), ops.stream()
    sizes = O.SIZES[chunk]
    rng = np.random.default_rng(chunk + sum(rots))
    tb = O.Tables(sizes, chunk)
    ap, ag, ab = (O.Arena(sizes, r) for r in rots)
    p = O.rand_list(sizes, rng)
    ap.put(p)
    ab.put([np.full(n, np.nan) for n in sizes])
    b = [np.full(n, np.nan, dtype=F) for n in sizes]
    what = f"mt_sgd_tab chunk={chunk} rots={rots}"
    for step, (nesterov, coef) in enumerate(((1, None), (1, 0.37), (0, None), (1, None))):
        mom_h = [0.0 if (t + step) % 5 == 0 else 0.8 + 0.02 * ((t + step) % 7) for t in range(len(sizes))]
        mom = torch.tensor(mom_h, dtype=torch.float32, device=DEV)
        g = O.rand_list(sizes, rng)
        ag.put(g)
        clip = torch.tensor([5.0, coef, 1.0, 0.0, 0.0], device=DEV) if coef is not None else None
        L.mt_sgd_tab(ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), ab.ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                     mom.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, chunk, nesterov, int(step == 0),
                     clip.data_ptr() if clip is not None else None, st)
        torch.cuda.synchronize()
        for a in (ap, ag, ab):
            a.check_gaps(what)
        new = [M.sgd_f32(p[t], g[t], b[t], tb.lr_h[t], tb.wd_h[t], mom_h[t], nesterov, int(step == 0), 1.0 if coef is None else coef)
               for t in range(len(sizes))]
        p, b = [x[0] for x in new], [x[1] for x in new]
        O.same_bits(ap.get(), p, f"{what} step {step} p")
        O.same_bits(ab.get(), b, f"{what} step {step} momentum buffer")
    clip = torch.tensor([float("nan"), float("nan"), 0.0, 3.0, 1.0], device=DEV)
    L.mt_sgd_tab(ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), ab.ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                 mom.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, chunk, 1, 0, clip.data_ptr(), st)
    torch.cuda.synchronize()
    O.same_bits(ap.get(), p, f"{what} skipped step p")
    O.same_bits(ab.get(), b, f"{what} skipped step momentum buffer")


@pytest.mark.gpu
def test_new_entry_points_reject_bad_arguments():
    L, st = y3d.lib(), ops.stream()
    sizes = [300, 5]
    tb = O.Tables(sizes, 256)
    a = [O.Arena(sizes, i).put([np.ones(n) for n in sizes]) for i in range(4)]
    mom = torch.zeros(2, device=DEV)
    sbuf, scal = O.guarded_out(M.NSCAL)
    clip = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.0], device=DEV)

    def update(kind, n, chunk, mom_p, scal_p):
        L.mt_update(kind, a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), a[2].ptrs.data_ptr(), a[3].ptrs.data_ptr(), tb.sizes.data_ptr(),
                    tb.lr.data_ptr(), tb.wd.data_ptr(), mom_p, tb.ct.data_ptr(), tb.co.data_ptr(), n, chunk, 0.9, 0.999, 1e-8, scal_p, None, st)

    for n, chunk in ((0, 256), (tb.n, 255), (-1, 256)):
        with pytest.raises(Y3DError):
            update(M.ADAM, n, chunk, None, scal.data_ptr())
        with pytest.raises(Y3DError):
            L.mt_sgd_tab(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), a[2].ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                         mom.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), n, chunk, 1, 0, None, st)
    for kind in (-1, 5):
        with pytest.raises(Y3DError):
            update(kind, tb.n, 256, mom.data_ptr(), scal.data_ptr())
    with pytest.raises(Y3DError):
        update(M.NADAM, tb.n, 256, None, None)  # the Adam family needs the step scalars
    with pytest.raises(Y3DError):
        update(M.RMSPROP, tb.n, 256, None, scal.data_ptr())  # RMSprop needs the momentum table
    with pytest.raises(Y3DError):
        L.mt_sgd_tab(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), a[2].ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                     None, tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, 256, 1, 0, None, st)
    for b1, b2, c, s in ((1.0, 0.999, clip.data_ptr(), scal.data_ptr()), (0.9, -0.1, clip.data_ptr(), scal.data_ptr()),
                         (0.9, 0.999, None, scal.data_ptr()), (0.9, 0.999, clip.data_ptr(), None)):
        with pytest.raises(Y3DError):
            L.mt_step_scalars(c, b1, b2, 4e-3, s, st)
    torch.cuda.synchronize()
    for x in a:
        O.same_bits(x.get(), [np.ones(n) for n in sizes], "a rejected call changed a tensor")
    assert bool(R.untouched(sbuf[M.NSCAL:]).all()) and not bool(scal.any())


# ---- y3d_mt_step_scalars ----------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.937, 0.99)], ids=["b0.9-0.999", "b0.937-0.99"])
def test_step_scalars_one_rounding_from_float64(betas):
    """t = 1..8 with a skipped step after t = 3: every value is the float64 restatement (fed the device's own fp32 mu_product of the
    step before) rounded to fp32, or one fp32 ulp from it; across the skipped step the whole array, mu_product included, keeps its bits"""
    L, st = y3d.lib(), ops.stream()
    b1, b2 = betas
    sbuf = R.sentinel((M.NSCAL + 64,), torch.float32, DEV)
    scal = sbuf[:M.NSCAL]
    used = list(range(14))
    off, total, mp = 0, 0, 1.0
    for t in range(1, 9):
        clip = torch.tensor([3.0, 1.0, 1.0, float(t), 0.0], device=DEV)
        L.mt_step_scalars(clip.data_ptr(), b1, b2, 4e-3, scal.data_ptr(), st)
        torch.cuda.synchronize()
        got = scal.cpu().numpy()
        want = M.step_scalars_f32(b1, b2, t, mp)
        mp = float(got[M.MU_PROD])
        for i in used:
            lo, hi = np.nextafter(want[i], F(-np.inf)), np.nextafter(want[i], F(np.inf))
            assert got[i] in (want[i], lo, hi), f"step scalar {i} at t={t}: {got[i]!r}, float64 rounded {want[i]!r}"
            off += int(got[i] != want[i])
            total += 1
        assert got[M.RECT_ON] == want[M.RECT_ON] and got[M.T] == t
        assert bool(R.untouched(sbuf[14:]).all()), "entries 14, 15 and everything behind the array stay unwritten"
        if t == 3:
            before = scal.clone()
            skipped = torch.tensor([float("inf"), float("nan"), 0.0, 3.0, 1.0], device=DEV)
            L.mt_step_scalars(skipped.data_ptr(), b1, b2, 4e-3, scal.data_ptr(), st)
            torch.cuda.synchronize()
            assert_bits(scal, before, "step scalars across a skipped step")
    print(f"mt_step_scalars betas={betas}: {off} of {total} values one ulp from the float64 restatement")


# ---- the optimizer classes --------------------------------------------------------------------------------------------------------------

CLASSES = ["SGD-table", "Adam", "Adamax", "NAdam", "RAdam", "RMSprop"]


def _params(seed, idle=True):
    """test_hip_optim's parameters, plus one that never carries a gradient"""
    ps = O._params(seed)
    if idle:
        ps.append(torch.ones(9, device=DEV).requires_grad_(True))
    return ps


def _make(kind, ps):
    from yolov10_3d_amd import optim as P
    groups = [{"params": ps[:2], "weight_decay": 5e-4}, {"params": ps[2:], "weight_decay": 0.0, "lr": 0.02}]
    if kind == "SGD-table":
        groups[1]["momentum"] = 0.8
        return P.FusedSGD(groups, lr=0.01, momentum=0.937, nesterov=True, device_momentum=True)
    if kind == "SGD":
        return P.FusedSGD(groups, lr=0.01, momentum=0.937, nesterov=True)
    if kind == "AdamW":
        return P.FusedAdamW(groups, lr=0.002, betas=(0.9, 0.999), weight_decay=0.0)
    if kind == "RMSprop":
        groups[0]["momentum"] = 0.0
        return P.FusedRMSprop(groups, lr=0.002, momentum=0.9)
    cls = {"Adam": P.FusedAdam, "Adamax": P.FusedAdamax, "NAdam": P.FusedNAdam, "RAdam": P.FusedRAdam}[kind]
    return cls(groups, lr=0.002, betas=(0.9, 0.999), weight_decay=0.0)


def _set_grads(ps, seed, nan=False):
    O._set_grads(ps[:5], seed, nan)
    for p in ps[5:]:
        p.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CLASSES)
def test_nonfinite_gradients_skip_the_step_on_the_device(kind):
    """parameters, both state buffers, the step scalars and the applied-step counter keep their bits; the skipped counter goes up by one"""
    ps = _params(2)
    opt = _make(kind, ps)
    assert opt.NSTATE == (1 if kind == "SGD-table" else 2)
    for s in range(2):
        _set_grads(ps, 40 + s)
        opt.step(max_norm=5.0)
    torch.cuda.synchronize()
    p0 = [p.detach().clone() for p in ps]
    flat0, nc0 = opt.state.flat.clone(), opt.state.norm_clip.clone()
    assert nc0.numel() == 5 + opt.NSCAL and nc0[3:5].tolist() == [2.0, 0.0] and bool(flat0.any())
    if opt.NSCAL:
        assert float(nc0[5 + M.T]) == 2.0 and float(nc0[5 + M.BC1]) > 0
    _set_grads(ps, 50, nan=True)
    opt.step(max_norm=5.0)
    torch.cuda.synchronize()
    nc1 = opt.state.norm_clip
    assert nc1[2:5].tolist() == [0.0, 2.0, 1.0] and opt.last_norm.numel() == 5
    if opt.NSCAL:
        assert_bits(nc1[5:], nc0[5:], f"{kind}: step scalars across a skipped step")
    assert_bits(opt.state.flat, flat0, f"{kind}: state across a skipped step")
    for t, (p, q) in enumerate(zip(ps, p0)):
        assert_bits(p.detach(), q, f"{kind}: parameter {t} across a skipped step")


@pytest.mark.gpu
def test_fused_sgd_device_momentum_follows_set_hyper_bit_for_bit():
    """four eager steps, lr and both groups' momenta rewritten through set_hyper() before each, against sgd_f32 with the same values;
    without clipping the coefficient is exactly 1"""
    ps = _params(3, idle=False)
    opt = _make("SGD-table", ps)
    assert [g["momentum"] for g in opt.param_groups] == [0.937, 0.8]
    p = [x.detach().cpu().numpy().reshape(-1) for x in ps]
    b = [np.zeros_like(x) for x in p]
    for s in range(4):
        if s:
            opt.param_groups[0]["momentum"] = float(np.interp(s, [0, 3], [0.8, 0.937]))
            opt.param_groups[1]["momentum"] = 0.0 if s == 2 else 0.5 + 0.1 * s
            opt.param_groups[1]["lr"] = 0.02 / s
            opt.set_hyper()
        O._set_grads(ps, 60 + s)
        g = [x.grad.cpu().numpy().reshape(-1) for x in ps]
        opt.step(max_norm=None)
        torch.cuda.synchronize()
        for t in range(len(ps)):
            grp = opt.param_groups[0 if t < 2 else 1]
            p[t], b[t] = M.sgd_f32(p[t], g[t], b[t], grp["lr"], grp["weight_decay"], grp["momentum"], 1, 0)
        O.same_bits([x.detach().cpu().numpy().reshape(-1) for x in ps], p, f"device momentum step {s} p")
        O.same_bits([x[0].cpu().numpy() for x in opt.state.bufs], b, f"device momentum step {s} buffer")


@pytest.mark.gpu
def test_default_optimizers_make_the_parent_commits_library_calls(monkeypatch):
    """FusedSGD / FusedAdamW constructed as before (device_momentum off) launch mt_sqnorm, mt_clip_coef and mt_sgd / mt_adamw with the
    argument lists they had - none of the new entry points; their groups carry no "momentum" key and norm_clip keeps five floats"""
    L = y3d.lib()
    calls = []
    for name in L.protos:
        short = name[4:]
        if short.startswith("mt_"):
            fn = getattr(L, short)
            monkeypatch.setattr(L, short, lambda *a, _f=fn, _n=short: (calls.append((_n, len(a))), _f(*a))[1])
    for kind, last in (("SGD", ("mt_sgd", 15)), ("AdamW", ("mt_adamw", 18))):
        ps = _params(4)
        opt = _make(kind, ps)
        assert not opt.device_momentum and all(sorted(k for k in g if k != "params") == ["lr", "weight_decay"] for g in opt.param_groups)
        del calls[:]
        _set_grads(ps, 70)
        opt.step(max_norm=10.0)
        torch.cuda.synchronize()
        assert calls == [("mt_sqnorm", 8), ("mt_clip_coef", 5), last], calls
        assert opt.state.norm_clip.numel() == 5 and opt.last_norm is opt.state.norm_clip and opt.table.mom is None
        assert sorted(opt.state_dict()) == ["flat", "norm_clip", "steps"]
    ps = _params(4)
    opt = _make("SGD-table", ps)
    del calls[:]
    _set_grads(ps, 70)
    opt.step(max_norm=10.0)
    assert [c[0] for c in calls] == ["mt_sqnorm", "mt_clip_coef", "mt_sgd_tab"]
    # the other kinds, ModelEMA and GradAccumulator: the sequence and the argument counts they had before the launch tables moved to
    # mt.py, written out.  A step over the same gradient tensors makes the same calls and uploads no gradient pointers; one replaced
    # gradient tensor costs exactly one upload
    from yolov10_3d_amd import optim as P
    adam = [("mt_sqnorm", 8), ("mt_clip_coef", 5), ("mt_step_scalars", 6), ("mt_update", 19)]
    for kind in CLASSES[1:]:
        want = [("mt_sqnorm", 8), ("mt_clip_coef", 5), ("mt_update", 19)] if kind == "RMSprop" else adam
        ps = _params(4)
        opt = _make(kind, ps)
        _set_grads(ps, 70)
        for s in range(3):
            if s == 2:
                ps[1].grad = ps[1].grad.clone()
            del calls[:]
            opt.step(max_norm=10.0)
            assert calls == want, (kind, s, calls)
            col = opt.table.col["grads"]
            if s == 0:
                col0, key0 = col, col.key
            assert col is col0 and col.uploads == (1 if s < 2 else 2) and (col.key is key0) == (s < 2), (kind, s, col.uploads)
    torch.cuda.synchronize()
    net = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.BatchNorm1d(3)).to(DEV)
    ema = P.ModelEMA(net)
    for s in range(2):
        del calls[:]
        ema.update(net)
        assert calls == [("mt_ema", 12)], calls
        assert [c.uploads for c in ema._tab.col.values()] == [1, 1]
    ps = _params(4, idle=False)
    acc = P.GradAccumulator(ps)
    _set_grads(ps, 71)
    grads = [p.grad for p in ps]
    for s in range(3):
        for p, g in zip(ps, grads):
            p.grad = g.clone() if (s == 2 and p is ps[1]) else g
        del calls[:]
        acc.add()
        assert calls == [("mt_grad_acc", 8)], calls
        assert [tb.col["grads"].uploads for tb in acc._tabs.values()] == [1 if s < 2 else 2]
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["SGD", "AdamW"] + CLASSES)
def test_state_moves_through_the_torch_format_bit_for_bit(kind):
    """3 steps (the second skipped), state_dict(torch_format=True) -> a fresh optimizer over cloned parameters, loaded before its first
    step and after it; the next step leaves parameters and state bit-identical to the original's.  The dict has torch's keys, entries
    only for parameters that have carried a gradient, and its hyper-parameters are taken over"""
    from yolov10_3d_amd import optim as P
    ps = _params(1)
    opt = _make(kind, ps)
    for s in range(3):
        _set_grads(ps, 10 + s, nan=(s == 1))
        opt.step(max_norm=5.0)
    opt.param_groups[1]["lr"] = 0.013  # a scheduler moved it: the loaded optimizer must follow
    if opt.device_momentum:
        opt.param_groups[1]["momentum"] = 0.85
    opt.set_hyper()
    torch.cuda.synchronize()
    sd = opt.state_dict(torch_format=True)
    keys, _, has_step = P.TORCH_STATE[opt.TORCH_NAME]
    assert sorted(sd["state"]) == [0, 1, 2, 3, 4] and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3, 4, 5]]
    for i, e in sd["state"].items():
        assert sorted(e) == sorted(keys + (("step",) if has_step else ()) + (("mu_product",) if kind == "NAdam" else ()))
        assert all(e[k].shape == ps[i].shape for k in keys) and (not has_step or float(e["step"]) == 2.0)
    assert sd["param_groups"][1]["lr"] == 0.013 and sd["param_groups"][0]["weight_decay"] == 5e-4
    assert ("betas" in sd["param_groups"][0]) == (kind not in ("SGD", "SGD-table", "RMSprop")) and ("momentum" in sd["param_groups"][0]) == (
        kind in ("SGD", "SGD-table", "RMSprop"))
    clones = []
    for after_first_step in (False, True):
        qs = [p.detach().clone().requires_grad_(True) for p in ps]
        o2 = _make(kind, qs)
        if after_first_step:
            _set_grads(qs, 99)
            o2.step(max_norm=5.0)
            with torch.no_grad():
                for q, p in zip(qs, ps):
                    q.copy_(p)
        o2.load_state_dict(sd)
        assert o2.param_groups[1]["lr"] == 0.013
        clones.append((qs, o2))
    for params, o in [(ps, opt)] + clones:
        _set_grads(params, 20)
        o.step(max_norm=5.0)
    torch.cuda.synchronize()
    for i, (qs, o2) in enumerate(clones):
        tag = f"{kind} resumed {'after' if i else 'before'} the first step"
        for t, (q, p) in enumerate(zip(qs, ps)):
            assert_bits(q.detach(), p.detach(), f"{tag}: parameter {t}")
        assert_bits(o2.state.flat, opt.state.flat, f"{tag}: flat state")
        if has_step:
            assert float(o2.state.norm_clip[3]) == 3.0
            if opt.NSCAL:
                # torch's dict carries mu_product for NAdam alone: for the other kinds the entries derived from it are not state
                keep = [i for i in range(M.NSCAL) if kind == "NAdam" or i not in (M.MU_PROD, M.MU_PROD_NEXT, M.NADAM_G, M.NADAM_M)]
                assert_bits(o2.state.norm_clip[5:][keep], opt.state.norm_clip[5:][keep], f"{tag}: step scalars")
    # refusals reach the caller through load_state_dict, naming the parameter
    bad = opt.state_dict(torch_format=True)
    bad["state"][3][keys[0]] = torch.zeros(7, device=DEV)
    with pytest.raises(Y3DError, match="parameter 3"):
        clones[0][1].load_state_dict(bad)
    if has_step:
        bad = opt.state_dict(torch_format=True)
        bad["state"][4]["step"] = torch.tensor(9.0)
        with pytest.raises(Y3DError, match="parameter 4: step 9"):
            clones[0][1].load_state_dict(bad)
    other = _make("Adam" if kind in ("SGD", "SGD-table", "RMSprop") else "SGD", [p.detach().clone().requires_grad_(True) for p in ps])
    with pytest.raises(Y3DError, match="parameter 0 has keys"):
        other.load_state_dict(sd)
    assert other._pending_load is None and other.param_groups[1]["lr"] == 0.02, "a refused dict must leave the optimizer as it was"


# ---- build_optimizer and captured steps on the tiny 3D model --------------------------------------------------------------------------


def _model(seed=3):
    torch.manual_seed(seed)
    return y3d.YOLOv10_3DDetectionModel("yolov10n_3D.yaml").to(DEV).train()


@pytest.mark.gpu
def test_build_optimizer_every_name_and_auto():
    """every name build_optimizer takes, on the tiny 3D model, with the reference's three groups; "auto" on both sides of 10 000
    iterations.  "RMSProp" is not among them (tests/test_host_logic.py pins that it raises): FusedRMSprop over reference_groups() is
    the reference's line, checked at the end"""
    from yolov10_3d_amd import optim as P
    model = _model()
    n_bias = sum(1 for m in model.modules() for n, _ in m.named_parameters(recurse=False) if n == "bias")
    want = {"SGD": P.FusedSGD, "AdamW": P.FusedAdamW, "Adam": P.FusedAdam, "Adamax": P.FusedAdamax, "NAdam": P.FusedNAdam, "RAdam": P.FusedRAdam}
    ref = P.build_optimizer(model, lr=0.01, momentum=0.9, decay=5e-4, name="SGD")
    for name, cls in want.items():
        opt = P.build_optimizer(model, lr=0.01, momentum=0.9, decay=5e-4, name=name)
        assert type(opt) is cls and len(opt.param_groups) == 3 and opt.auto is None
        assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 5e-4, 0.0] and len(opt.param_groups[0]["params"]) == n_bias > 0
        assert [[id(p) for p in g["params"]] for g in opt.param_groups] == [[id(p) for p in g["params"]] for g in ref.param_groups]
    nc = getattr(model, "nc", 10)
    long = P.build_optimizer(model, name="auto", iterations=10001)
    assert type(long) is P.FusedSGD and long.auto == {"name": "SGD", "lr": 0.01, "momentum": 0.9, "warmup_bias_lr": 0.0}
    short = P.build_optimizer(model, name="auto", iterations=10000)
    lr_fit = round(0.002 * 5 / (4 + nc), 6)
    assert type(short) is P.FusedAdamW and short.auto == {"name": "AdamW", "lr": lr_fit, "momentum": 0.9, "warmup_bias_lr": 0.0}
    assert short.betas == (0.9, 0.999) and all(g["lr"] == lr_fit for g in short.param_groups)
    with pytest.raises(NotImplementedError, match="Optimizer 'Lion' not found in list of available optimizers"):
        P.build_optimizer(model, name="Lion")
    rms = P.FusedRMSprop(P.reference_groups(model, 5e-4), lr=0.01, momentum=0.9)
    assert [[id(p) for p in g["params"]] for g in rms.param_groups] == [[id(p) for p in g["params"]] for g in ref.param_groups]
    assert [g["weight_decay"] for g in rms.param_groups] == [0.0, 5e-4, 0.0] and all(g["momentum"] == 0.9 for g in rms.param_groups)


def _run(name, mode, batches, hyper=None, device_momentum=False):
    """len(batches) steps, eager or replayed from one hipGraph; `hyper(opt, j)` moves the groups before step j > 0"""
    from yolov10_3d_amd.graph import GraphedTrainStep
    from yolov10_3d_amd.optim import FusedRMSprop, build_optimizer, reference_groups
    y3d.set_compute_dtype(torch.bfloat16)
    model = _model()
    if name == "RMSprop":  # (not among build_optimizer's names: the reference's line over the same three groups)
        opt = FusedRMSprop(reference_groups(model), lr=0.002, momentum=0.9)
    else:
        opt = build_optimizer(model, lr=0.002 if name not in ("SGD",) else 0.01, momentum=0.9, name=name, device_momentum=device_momentum)
    model.model[-1].restack()
    step = GraphedTrainStep(model, opt, batches[0]) if mode == "graph" else None
    for j, b in enumerate(batches):
        if hyper is not None and j:
            hyper(opt, j)
            opt.set_hyper()
        if step is not None:
            step(b)
        else:
            loss, _ = model(b)
            loss.backward()
            opt.step(max_norm=10.0)
            opt.zero_grad()
            del loss
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in model.state_dict().items()}, opt.state.flat.clone(), opt.state.norm_clip.clone())


def _same_run(a, b, what):
    for k, v in a[0].items():
        assert torch.equal(v, b[0][k]), f"{what}: state {k} differs"
    assert_bits(b[1], a[1], f"{what}: optimizer state")
    assert_bits(b[2][3:], a[2][3:], f"{what}: step counters and step scalars")


@pytest.fixture(scope="module")
def batches():
    from bench import synth_batch
    return [synth_batch(2, 256, 256, 20 + j, DEV) for j in range(4)]


@pytest.mark.gpu
def test_graphed_step_follows_momentum_and_lr_between_replays(batches):
    """FusedSGD(device_momentum=True): four replays with momentum and lr rewritten in place between them end where four eager steps end"""
    def hyper(opt, j):
        for g in opt.param_groups:
            g["momentum"] = float(np.interp(j, [0, 3], [0.8, 0.937]))
            g["lr"] = 0.01 * (1 + j) / 4
    res = {mode: _run("SGD", mode, batches, hyper, device_momentum=True) for mode in ("eager", "graph")}
    _same_run(res["eager"], res["graph"], "SGD with device momentum")
    assert bool(res["eager"][1].any())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["Adam", "Adamax", "NAdam", "RAdam", "RMSprop"])
def test_graphed_step_replays_each_new_optimizer(name, batches):
    """one capture, two replays (constructing the step must leave the step scalars, NAdam's mu_product among them, where they were)"""
    res = {mode: _run(name, mode, batches[:2]) for mode in ("eager", "graph")}
    _same_run(res["eager"], res["graph"], name)
    assert float(res["graph"][2][3]) == 2.0 and bool(res["eager"][1].any())
