"""Fused optimizer step: gradient clipping + SGD(Nesterov) or AdamW over all parameters in three HIP launches, + ModelEMA in one.

Reference recipe (engine/trainer.py:567-575): unscale -> clip_grad_norm_(max_norm=10) -> optimizer.step -> zero_grad -> ema.update,
with the three parameter groups of build_optimizer (:734-790: weights with decay, norm weights without, biases without; SGD with
nesterov for long schedules, AdamW(betas=(momentum, 0.999)) for short ones).  Semantics are torch.optim.SGD's (dampening 0),
torch.optim.AdamW's (amsgrad off), torch.nn.utils.clip_grad_norm_'s and utils/torch_utils.py:416-443's ModelEMA.

The rest of the reference's list (:776-781 Adam, Adamax, NAdam, RAdam, RMSProp - the last as a class, not yet by name -; :755-764 `auto`) runs on two more launches: the step
scalars (bias corrections, NAdam's mu terms, RAdam's rectification: everything that depends only on the device's count of applied
steps) and one update kernel per kind, in torch's single-tensor arithmetic.  FusedSGD(device_momentum=True) / FusedRMSprop read
momentum from a device table, so the reference's momentum warm-up (:392-393) reaches a captured step through set_hyper(); Schedule
restates that warm-up and the LambdaLR schedule on the host; state_dict(torch_format=True) / load_state_dict speak torch.optim's
checkpoint layout (the reference resumes from `ckpt["optimizer"]`).
"""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from . import mt, ops
from ._lib import Y3DError, lib
from .mt import CHUNK, PtrUploader, chunk_map  # noqa: F401  (their home is mt.py; tests and tools import them from here)

# indices into the step-scalar array (include/y3d.h, y3d_mt_step_scalars) and y3d_mt_update's kinds
S_BC1, S_BC2, S_BC1_SQRT, S_BC2_SQRT, S_MU, S_MU_NEXT, S_MU_PROD, S_MU_PROD_NEXT, S_RHO, S_RECT_ON, S_RECT, S_T, S_NADAM_G, S_NADAM_M = range(14)
OPT_ADAM, OPT_ADAMAX, OPT_NADAM, OPT_RADAM, OPT_RMSPROP = range(5)


# ---- torch-format optimizer state <-> the flat state buffers: pure functions, no device needed --------------------------------------------
# per kind: (keys of the flat state rows in order, keys that torch may leave out or set to None, whether torch keeps a `step`)
TORCH_STATE = {
    "SGD": (("momentum_buffer",), ("momentum_buffer",), False),
    "AdamW": (("exp_avg", "exp_avg_sq"), (), True),
    "Adam": (("exp_avg", "exp_avg_sq"), (), True),
    "NAdam": (("exp_avg", "exp_avg_sq"), (), True),
    "RAdam": (("exp_avg", "exp_avg_sq"), (), True),
    "Adamax": (("exp_avg", "exp_inf"), (), True),
    "RMSprop": (("square_avg", "momentum_buffer"), ("momentum_buffer",), True),
}


def is_torch_format(sd):
    return isinstance(sd, dict) and "state" in sd and "param_groups" in sd


def flat_to_torch_state(kind, flat, shapes, indices, step=None, mu_product=None):
    """flat (NSTATE, sum of numel) -> torch's `state`: {i: {key: tensor of shapes[i]}} for i in `indices`, with `step` (and NAdam's
    `mu_product`) as the 0-dim float32 tensors torch keeps"""
    keys, _, has_step = TORCH_STATE[kind]
    offs = np.concatenate([[0], np.cumsum([int(np.prod(sh)) for sh in shapes])]).astype(np.int64)
    out = {}
    for i in indices:
        e = {}
        if has_step:
            e["step"] = torch.tensor(float(step or 0), dtype=torch.float32)
        for r, k in enumerate(keys):
            e[k] = flat[r, int(offs[i]):int(offs[i + 1])].detach().clone().reshape(tuple(shapes[i]))
        if kind == "NAdam":
            e["mu_product"] = torch.tensor(1.0 if mu_product is None else float(mu_product), dtype=torch.float32)
        out[i] = e
    return out


def torch_state_to_flat(kind, state, shapes, dtype=torch.float32):
    """torch's `state` -> (flat (NSTATE, sum of numel) on the CPU, step | None, mu_product | None, indices present).  Parameters without
    an entry load as zeros.  Y3DError: per-parameter `step` (or `mu_product`) values that differ - there is ONE device counter -, a
    tensor whose size is not its parameter's, the state keys of another optimizer kind; each names the parameter index."""
    keys, optional, has_step = TORCH_STATE[kind]
    sizes = [int(np.prod(sh)) for sh in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = torch.zeros(len(keys), int(offs[-1]), dtype=dtype)
    step = mu = None
    present = []
    for i in sorted(state):
        e = state[i]
        if not 0 <= i < len(shapes):
            raise Y3DError(f"optimizer state for parameter {i}: this optimizer has {len(shapes)} parameters")
        extra = set(e) - {"step", "mu_product"} - set(keys)
        missing = [k for k in keys if k not in e and k not in optional]
        if extra or missing:
            raise Y3DError(f"optimizer state for parameter {i} has keys {sorted(e)}: not the state of {kind} ({', '.join(keys)})")
        for r, k in enumerate(keys):
            v = e.get(k)
            if v is None:
                continue
            if v.numel() != sizes[i]:
                raise Y3DError(f"optimizer state for parameter {i}: {k} has {v.numel()} elements, the parameter {sizes[i]}")
            flat[r, int(offs[i]):int(offs[i + 1])] = v.detach().reshape(-1).to(device="cpu", dtype=dtype)
        if has_step and "step" in e:
            t = float(e["step"])
            if step is not None and t != step:
                raise Y3DError(f"optimizer state for parameter {i}: step {t:g}, earlier parameters {step:g} - the fused step keeps one "
                               "device-side step count for all parameters")
            step = t
        if kind == "NAdam" and "mu_product" in e:
            m = float(e["mu_product"])
            if mu is not None and m != mu:
                raise Y3DError(f"optimizer state for parameter {i}: mu_product {m!r}, earlier parameters {mu!r} - one device-side value")
            mu = m
        present.append(i)
    return flat, step, mu, present


# ---- the optimizers: DESIGN.md §3.29 for the two lifetimes of their device state and the capture contract ----------------------------------
class OptState:
    """What lives as long as the optimizer, created on its first step in one allocation each: `flat` (NSTATE, sum of numel) zero-
    initialised state rows, `bufs[i]` the (NSTATE, numel) view of parameter i, `norm_clip` the device counters [norm, clip coefficient,
    finite flag, steps applied, steps skipped] followed by the NSCAL step scalars, of which `scal` is the view (None for NSCAL = 0)"""

    def __init__(self, sizes, nstate, nscal, dev):
        self.flat = torch.zeros(nstate, sum(sizes), dtype=torch.float32, device=dev)
        self.bufs, off = [], 0
        for n in sizes:
            self.bufs.append(self.flat[:, off:off + n])
            off += n
        self.norm_clip = torch.zeros(5 + nscal, dtype=torch.float32, device=dev)
        self.scal = self.norm_clip[5:] if nscal else None


class OptTable(mt.Table):
    """The launch table over the `active` parameters (those that carry a gradient), valid while that list and the group layout `hkey`
    stay: mt.Table's chunk map, the fixed columns ptr["state0"] / ["state1"] into OptState.flat, the refreshable columns col["params"]
    (plain upload) and col["grads"] (pinned), the per-tensor `lr` / `wd` / `mom` (None unless the momentum is a device table) that
    set_hyper() rewrites in place, and `partials` of the norm launch"""

    def __init__(self, state, active, sizes, hkey, hyper):
        dev = state.flat.device
        super().__init__(sizes, dev, **{f"state{r}": [state.bufs[i][r].data_ptr() for i in active] for r in range(state.flat.shape[0])})
        self.active, self.hkey = list(active), hkey
        self.partials = torch.empty(self.nchunks, dtype=torch.float32, device=dev)
        self.lr, self.wd, self.mom = (None if v is None else torch.tensor(v, dtype=torch.float32, device=dev) for v in hyper)
        self.column("params", pinned=False)
        self.column("grads")


class FusedOptimizer:
    """What the fused optimizers share: parameter groups, OptState and OptTable, the clipping launches, step(), zero_grad(), set_hyper(),
    both checkpoint layouts.  A kind sets NSTATE / NSCAL / TORCH_NAME and has its own constructor arguments, `_update(L, tb, clip, s)` (its
    launches), `_torch_group_hyper()` (what torch keeps per group beside lr / weight_decay) and `_take_group_hyper(groups)` (the same,
    taken from a torch dict's groups).  `device_momentum` (class or instance): the groups carry a "momentum" key and a per-
    tensor device column holds it next to lr / weight_decay - read in one place, `_hyper`."""
    NSTATE = 1  # flat zero-initialised state buffers per parameter
    NSCAL = 0   # floats behind the five counters of `norm_clip`: the step scalars of y3d_mt_step_scalars
    TORCH_NAME = None
    ALWAYS_CLIP = False  # the update reads the device's count of applied steps, which the clipping launch keeps
    device_momentum = False
    momentum = None

    def __init__(self, param_groups, lr, weight_decay):
        if isinstance(param_groups, (list, tuple)) and param_groups and not isinstance(param_groups[0], dict):
            param_groups = [{"params": list(param_groups)}]
        self.param_groups, self.params = [], []
        for g in param_groups:
            self._append_group(g, lr, weight_decay)
        if not self.params:
            raise ValueError("FusedSGD: no parameters")
        self.state = self.table = None
        self._steps = 0
        self.last_norm = None
        self._pending_load = None
        self._seen = set()  # parameters that have carried a gradient (or loaded state): the ones torch would hold state for
        self.auto = None    # build_optimizer(name="auto"): what was chosen

    @property
    def _hyper(self):
        """(group key, OptTable attribute) of the per-tensor hyper-parameter columns"""
        return (("lr", "lr"), ("weight_decay", "wd"), ("momentum", "mom"))[:3 if self.device_momentum else 2]

    def _append_group(self, g, lr, weight_decay):
        g = dict(g)
        for (key, _), v in zip(self._hyper, (lr, weight_decay, self.momentum)):
            g.setdefault(key, v)
        g["params"] = [p for p in g["params"] if p.requires_grad]
        self.param_groups.append(g)
        self.params = [p for gg in self.param_groups for p in gg["params"]]

    def add_param_group(self, g):
        self._append_group(g, self.param_groups[0]["lr"], 0.0)
        self.state = self.table = None

    def _hkey(self):
        return [tuple(g[key] for key, _ in self._hyper) + (len(g["params"]),) for g in self.param_groups]

    def _per_tensor(self, key, active):
        row = [g[key] for g in self.param_groups for _ in g["params"]]
        return [row[i] for i in active]

    def _build(self, active):
        """the table over the parameters that carry a gradient (torch.optim.SGD and clip_grad_norm_ skip the others, e.g. the neck
        blocks behind a detect level that `num_scales: 2` leaves unused); on the first call the state: its buffers are zero-
        initialised, so the first update `buf = momentum*0 + g` equals torch's `buf = clone(g)` exactly."""
        dev = self.params[0].device
        if dev.type != "cuda":
            raise Y3DError("FusedSGD needs parameters on a HIP device")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise Y3DError("FusedSGD: parameters must be contiguous fp32 tensors")
        fresh = self.state is None
        if fresh:
            self.state = OptState([p.numel() for p in self.params], self.NSTATE, self.NSCAL, dev)
        hyper = ([self._per_tensor(key, active) for key, _ in self._hyper] + [None])[:3]
        self.table = OptTable(self.state, active, [self.params[i].numel() for i in active], self._hkey(), hyper)
        self._seen.update(active)
        if fresh and self._pending_load is not None:  # load_state_dict() before the first step
            sd, self._pending_load = self._pending_load, None
            if "torch" in sd:
                self._apply_torch(*sd["torch"])
            else:
                self.load_state_dict(sd)
        return self.table

    def _take_group_momentum(self, groups):
        """momentum is one launch constant unless device_momentum keeps it per group"""
        moms = {float(g["momentum"]) for g in groups if "momentum" in g}
        if self.device_momentum:
            for g, src in zip(self.param_groups, groups):
                if "momentum" in src:
                    g["momentum"] = float(src["momentum"])
        elif len(moms) > 1:
            raise Y3DError(f"optimizer state with per-group momenta {sorted(moms)}: construct the optimizer with device_momentum=True")
        if len(moms) == 1:
            self.momentum = moms.pop()

    def _held(self):
        """(flat, norm_clip) as they are now: the state's, or those of a native dict loaded before the first step, or None"""
        if self.state is not None:
            return self.state.flat, self.state.norm_clip
        pl = self._pending_load
        if pl is not None and pl.get("flat") is not None and pl.get("norm_clip") is not None:
            return pl["flat"], pl["norm_clip"]
        return None

    def state_dict(self, torch_format=False, native=False):
        """optimizer state for checkpoint / resume (the reference saves `optimizer.state_dict()`, engine/trainer.py:470-486): the flat
        state buffers in parameter order (SGD: momentum; AdamW: exp_avg, exp_avg_sq) and the device-side counters [norm, clip
        coefficient, finite flag, steps APPLIED, steps skipped] - `steps applied` is AdamW's bias-correction step count.

        torch_format: torch.optim's layout instead, as the reference's checkpoints hold it - `state[i]` with torch's keys for this
        optimizer (TORCH_STATE) for every parameter that has been active, `param_groups` with lr, weight_decay, momentum / betas,
        initial_lr when set and `params` indices in group order.  native (with torch_format): a third entry "native" = {"steps",
        "norm_clip" on the CPU or None} - the counters torch's layout has no place for (steps skipped, the step scalars), which
        load_state_dict takes back; train.Trainer's checkpoints hold it"""
        held = self._held()
        if not torch_format:
            st = self.state
            return {"steps": self._steps, "flat": None if st is None else st.flat.detach().clone(),
                    "norm_clip": None if st is None else st.norm_clip.detach().clone()}
        groups, k = [], 0
        for g in self.param_groups:
            d = {"lr": g["lr"], "weight_decay": g["weight_decay"]}
            d.update(self._torch_group_hyper())
            for key in ("momentum", "initial_lr"):
                if key in g:
                    d[key] = g[key]
            d["params"] = list(range(k, k + len(g["params"])))
            k += len(g["params"])
            groups.append(d)
        shapes = [tuple(p.shape) for p in self.params]
        state = {}
        if held is not None:
            nc = held[1].detach().cpu()
            mu = float(nc[5 + S_MU_PROD]) if self.TORCH_NAME == "NAdam" and float(nc[3]) > 0 else None
            state = flat_to_torch_state(self.TORCH_NAME, held[0], shapes, sorted(self._seen), step=float(nc[3]), mu_product=mu)
        elif self._pending_load is not None and "torch" in self._pending_load:  # loaded, not stepped yet
            flat, step, mu, present = self._pending_load["torch"]
            state = flat_to_torch_state(self.TORCH_NAME, flat, shapes, present, step=step, mu_product=mu)
        sd = {"state": state, "param_groups": groups}
        if native:
            sd["native"] = {"steps": self._steps, "norm_clip": None if held is None else held[1].detach().cpu().clone()}
        return sd

    def _convert_torch(self, sd):
        """a torch.optim state dict -> (flat, step, mu_product, indices present), validated against these parameters; nothing is changed"""
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != [len(g["params"]) for g in self.param_groups]:
            raise Y3DError(f"optimizer state with parameter groups of {[len(g['params']) for g in groups]} parameters does not fit "
                           f"these groups {[len(g['params']) for g in self.param_groups]}")
        order = [i for g in groups for i in g["params"]]  # torch's ids in group order -> our parameter index
        pos = {pid: k for k, pid in enumerate(order)}
        unknown = [pid for pid in sd["state"] if pid not in pos]
        if unknown:
            raise Y3DError(f"optimizer state for parameter {unknown[0]}, which no parameter group lists")
        state = {pos[pid]: e for pid, e in sd["state"].items()}
        return torch_state_to_flat(self.TORCH_NAME, state, [tuple(p.shape) for p in self.params])

    def _apply_torch(self, flat, step, mu, present):
        st = self.state
        st.flat.copy_(flat)
        self._seen.update(present)
        if step is not None:  # (torch's SGD keeps no step count: the device counters stay)
            self._steps = int(step)
            nc = st.norm_clip.detach().cpu()
            nc[3] = step
            if mu is not None:
                nc[5 + S_MU_PROD] = mu
            st.norm_clip.copy_(nc)

    def load_state_dict(self, sd):
        """inverse of state_dict(), either format; before the first step the state is kept and applied when the state is created.
        A torch-format dict with a "native" entry (state_dict(native=True)) restores the counters behind torch's layout exactly as
        they were (steps applied / skipped, NAdam's mu_product) - but only into an optimizer that has not stepped yet: one whose
        state exists takes the torch entries alone."""
        if is_torch_format(sd):  # torch.optim's layout (a reference checkpoint's `ckpt["optimizer"]`)
            conv = self._convert_torch(sd)  # raises before anything is taken over
            for g, src in zip(self.param_groups, sd["param_groups"]):
                for key in ("lr", "weight_decay", "initial_lr"):
                    if key in src:
                        g[key] = float(src[key])
            self._take_group_hyper(sd["param_groups"])
            if self.state is not None:
                self._apply_torch(*conv)
                return self.set_hyper()
            self._pending_load = {"torch": conv}
            native = sd.get("native")
            if native is not None and native["norm_clip"] is not None:
                self._seen.update(conv[3])
                self.load_state_dict({"steps": native["steps"], "flat": conv[0], "norm_clip": native["norm_clip"]})
            return
        self._steps = int(sd["steps"])
        if self.state is None:
            self._pending_load = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
            return
        st = self.state
        if sd.get("flat") is not None:
            if sd["flat"].shape != st.flat.shape:
                raise Y3DError(f"optimizer state of shape {tuple(sd['flat'].shape)} does not fit these parameters {tuple(st.flat.shape)}")
            st.flat.copy_(sd["flat"])
            st.norm_clip.copy_(sd["norm_clip"])

    def set_hyper(self):
        """write the groups' current lr / weight_decay (and momentum, with device_momentum) into the EXISTING device columns (in place: a
        captured hipGraph of the step keeps reading them, graph.GraphedTrainStep) - what a scheduler's `param_group["lr"] = ...` needs
        before the next replay"""
        tb = self.table
        if tb is None:
            return
        for key, attr in self._hyper:
            getattr(tb, attr).copy_(torch.tensor(self._per_tensor(key, tb.active), dtype=torch.float32), non_blocking=False)
        tb.hkey = self._hkey()

    def _tables(self):
        active = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not active:
            raise Y3DError("FusedSGD.step: no parameter has a gradient")
        tb = self.table
        hkey = self._hkey()
        if tb is not None and tb.active == active and tb.hkey != hkey and [h[-1] for h in tb.hkey] == [h[-1] for h in hkey]:
            self.set_hyper()  # only the values moved (a scheduler): same tables, new contents
        if tb is None or tb.active != active or tb.hkey != hkey:
            tb = self._build(active)
        ps = [self.params[i] for i in active]
        tb.col["params"].refresh([p.data_ptr() for p in ps])  # parameters re-pointed (e.g. sibling-branch stacking, .to()): refresh
        grads = tb.fp32_contiguous([p.grad for p in ps])
        for p, g in zip(ps, grads):
            if g is not p.grad:
                p.grad = g
        tb.col["grads"].refresh([g.data_ptr() for g in grads])
        return tb

    @torch.no_grad()
    def step(self, max_norm: float | None = 10.0):
        """clip (when max_norm is given) + update; self.last_norm holds the device tensor [total_norm, clip_coef, finite flag, steps
        applied, steps skipped].  A step whose gradient norm is inf / NaN is skipped ON THE DEVICE (no host synchronisation): parameters,
        momentum / Adam state and AdamW's bias-correction step count stay - torch.cuda.amp.GradScaler.step's rule, engine/trainer.py:
        567-572.  Under ddp.FlatGradReducer the norm is that of the all-reduced buffer, so every rank takes the same decision.

        The Adam family (ALWAYS_CLIP) runs the clipping launch without a `max_norm` too (with an infinite bound: coefficient 1), because
        the bias corrections read the number of APPLIED steps from its device-side counter - ONE source for the step count, whether or
        not the step is clipped, eager or replayed from a hipGraph, fresh or resumed.  Side effect: a step with a non-finite gradient
        norm is skipped in that case too."""
        if max_norm is None and self.ALWAYS_CLIP:
            max_norm = float("inf")
        tb = self._tables()
        L, s = lib(), ops.stream()
        clip = None
        if max_norm is not None:
            nc = self.state.norm_clip
            L.mt_sqnorm(tb.col["grads"].dev.data_ptr(), tb.sizes.data_ptr(), *tb.chunks, tb.partials.data_ptr(), s)
            L.mt_clip_coef(tb.partials.data_ptr(), tb.nchunks, float(max_norm), nc.data_ptr(), s)
            clip = nc.data_ptr()
            self.last_norm = nc[:5] if self.NSCAL else nc
        self._steps += 1
        self._update(L, tb, clip, s)
        ops.bump_weight_epoch()  # the parameters changed behind torch's version counters

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    # ---- what graph.GraphedTrainStep needs: undoing its warm-up steps, and a capture of step() ------------------------------------------
    def snapshot(self):
        """-> (host step count, clones of flat and norm_clip, or None when there is no state yet) for restore()"""
        st = self.state
        return self._steps, None if st is None else (st.flat.clone(), st.norm_clip.clone())

    def restore(self, snap):
        """put a snapshot() back IN PLACE (every address stays); state that did not exist at the snapshot is zeroed"""
        self._steps, held = snap
        st = self.state
        if st is not None and held is None:
            st.flat.zero_()
            st.norm_clip.zero_()
        elif st is not None:
            st.flat.copy_(held[0])
            st.norm_clip.copy_(held[1])

    def begin_capture(self):
        """before step() is recorded into a hipGraph: the gradient column gets an uploader of its own, of depth 1, and no key (the
        recorded step uploads).  The optimizer's rotating pinned buffers would be overwritten a few eager steps later, and the replays
        would read those pointers."""
        self.table.column("grads", depth=1, now=True)
        self._steps_at_capture = self._steps

    def end_capture(self):
        """after the capture -> what the graph must keep alive: the table as captured (chunk maps, state / parameter / gradient pointer
        columns, the depth-1 uploader whose pinned buffer the graph's copy node reads, lr / wd / mom).  The optimizer keeps the SAME
        table, so set_hyper() reaches the replays, with a fresh gradient column: its next eager step builds an uploader and uploads.
        The step the recorded Python counted has not run: the host step count is put back."""
        held = self.table.held()
        self.table.column("grads")
        self._steps = self._steps_at_capture
        return held


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD (dampening 0) with Nesterov momentum"""
    TORCH_NAME = "SGD"

    def __init__(self, param_groups, lr=0.01, momentum=0.937, nesterov=True, weight_decay=0.0, device_momentum=False):
        """device_momentum: the groups carry a "momentum" key (as torch's do: the reference's warm-up finds it, engine/trainer.py:392),
        a per-tensor device table holds it next to lr / wd, set_hyper() rewrites it in place and the table-reading kernel
        (y3d_mt_sgd_tab) is launched - so a captured step follows a momentum schedule.  False: momentum is a launch constant."""
        self.device_momentum = bool(device_momentum)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        super().__init__(param_groups, lr, weight_decay)

    def _torch_group_hyper(self):
        return {"momentum": self.momentum, "nesterov": self.nesterov}

    _take_group_hyper = FusedOptimizer._take_group_momentum

    def _update(self, L, tb, clip, s):
        head = (tb.col["params"].dev.data_ptr(), tb.col["grads"].dev.data_ptr(), tb.ptr["state0"].data_ptr(), tb.sizes.data_ptr(),
                tb.lr.data_ptr(), tb.wd.data_ptr())
        if self.device_momentum:
            L.mt_sgd_tab(*head, tb.mom.data_ptr(), *tb.chunks, int(self.nesterov), 0, clip, s)
        else:
            L.mt_sgd(*head, *tb.chunks, self.momentum, int(self.nesterov), 0, clip, s)


class _Betas(FusedOptimizer):
    """the Adam family: betas and eps as launch constants, two state rows, the clipping launch always"""
    NSTATE = 2  # exp_avg, exp_avg_sq (Adamax: exp_inf)
    ALWAYS_CLIP = True

    def __init__(self, param_groups, lr, betas, eps, weight_decay):
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        super().__init__(param_groups, lr, weight_decay)

    def _torch_group_hyper(self):
        return {"betas": self.betas, "eps": self.eps}

    def _take_group_hyper(self, groups):
        """the betas are launch constants (the reference's warm-up never touches them): one pair for all groups"""
        betas = {(float(g["betas"][0]), float(g["betas"][1])) for g in groups if "betas" in g}
        if len(betas) > 1:
            raise Y3DError(f"optimizer state with per-group betas {sorted(betas)}: the fused step takes one pair")
        if betas:
            self.betas = betas.pop()
        eps = {float(g["eps"]) for g in groups if "eps" in g}
        if len(eps) == 1:
            self.eps = eps.pop()

    def _pointers(self, tb):
        return (tb.col["params"].dev.data_ptr(), tb.col["grads"].dev.data_ptr(), tb.ptr["state0"].data_ptr(), tb.ptr["state1"].data_ptr(),
                tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr())


class FusedAdamW(_Betas):
    """torch.optim.AdamW(betas, eps, weight_decay per group), amsgrad off"""
    TORCH_NAME = "AdamW"

    def __init__(self, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(param_groups, lr, betas, eps, weight_decay)

    def _update(self, L, tb, clip, s):
        # bias_corr1 / bias_corr2_sqrt: the launcher wants them positive; the kernel recomputes both from the device's count of applied
        # steps whenever norm_clip is given, which ALWAYS_CLIP makes every step of this class
        L.mt_adamw(*self._pointers(tb), *tb.chunks, *self.betas, self.eps, 1.0, 1.0, clip, s)


class FusedAdam(_Betas):
    """torch.optim.Adam: coupled L2 decay `g += wd*p` (amsgrad off).  Two launches after the clipping pair: y3d_mt_step_scalars turns
    the device's count of APPLIED steps into the bias corrections (and NAdam's / RAdam's scalars), y3d_mt_update applies them - one
    device-side source for everything that depends on the step, eager or replayed, as FusedAdamW's bias corrections"""
    NSCAL = 16
    KIND = OPT_ADAM
    TORCH_NAME = "Adam"
    MOMENTUM_DECAY = 4e-3  # torch.optim.NAdam's default (read by y3d_mt_step_scalars for every kind; used by NAdam)

    def __init__(self, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr, betas, eps, weight_decay)

    def _update(self, L, tb, clip, s):
        scal = self.state.scal.data_ptr()
        L.mt_step_scalars(clip, *self.betas, self.MOMENTUM_DECAY, scal, s)
        L.mt_update(self.KIND, *self._pointers(tb), None, *tb.chunks, *self.betas, self.eps, scal, clip, s)


class FusedAdamax(FusedAdam):
    """torch.optim.Adamax: exp_inf = max(beta2*exp_inf, |g| + eps); p -= lr/(1-beta1^t) * exp_avg / exp_inf"""
    KIND, TORCH_NAME = OPT_ADAMAX, "Adamax"

    def __init__(self, param_groups, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr, betas, eps, weight_decay)


class FusedNAdam(FusedAdam):
    """torch.optim.NAdam (momentum_decay 4e-3, coupled decay); mu_product is the one piece of state among the step scalars"""
    KIND, TORCH_NAME = OPT_NADAM, "NAdam"

    def __init__(self, param_groups, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr, betas, eps, weight_decay)


class FusedRAdam(FusedAdam):
    """torch.optim.RAdam (coupled decay): the unrectified arm while rho_t <= 5, the rectified one after"""
    KIND, TORCH_NAME = OPT_RADAM, "RAdam"


class FusedRMSprop(FusedOptimizer):
    """torch.optim.RMSprop(alpha, eps, momentum), not centered; the momentum always comes from the per-tensor device table"""
    NSTATE = 2  # square_avg, momentum_buffer
    TORCH_NAME = "RMSprop"
    device_momentum = True

    def __init__(self, param_groups, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0):
        self.momentum, self.alpha, self.eps = float(momentum), float(alpha), float(eps)
        super().__init__(param_groups, lr, weight_decay)

    def _torch_group_hyper(self):
        return {"alpha": self.alpha, "eps": self.eps}

    def _take_group_hyper(self, groups):
        self._take_group_momentum(groups)
        for key in ("alpha", "eps"):
            vals = {float(g[key]) for g in groups if key in g}
            if len(vals) == 1:
                setattr(self, key, vals.pop())

    def _update(self, L, tb, clip, s):
        L.mt_update(OPT_RMSPROP, tb.col["params"].dev.data_ptr(), tb.col["grads"].dev.data_ptr(), tb.ptr["state0"].data_ptr(),
                    tb.ptr["state1"].data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(), tb.mom.data_ptr(), *tb.chunks,
                    0.0, self.alpha, self.eps, None, clip, s)


class Schedule:
    """The reference's learning-rate and momentum schedule (engine/trainer.py:217-223, 332, 384-393, 468-470), host only: `LambdaLR` with
    the linear or cosine factor per epoch, and over the first `nw` iterations the interpolation of lr (group 0, the biases, from
    `warmup_bias_lr`, the other groups from 0) and momentum (from `warmup_momentum`) towards their scheduled values.  Every change is
    written into the optimizer's groups and, through set_hyper(), into its device tables in place - a captured step follows it.
    Momentum moves only where a group has a "momentum" key (FusedSGD(device_momentum=True), FusedRMSprop), as in the reference.
    No loop, no validation, no checkpoints: `for epoch: for i: sched.iteration(i + nb*epoch, epoch); step(...)`, then epoch_end()."""

    def __init__(self, opt, epochs, nb, lrf=0.01, cos_lr=False, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, nbs=64, batch=16):
        self.opt, self.epochs, self.nb = opt, int(epochs), int(nb)
        if cos_lr:  # utils/torch_utils.py:390-392 one_cycle(1, lrf, epochs)
            self.lf = lambda x: max((1 - math.cos(x * math.pi / self.epochs)) / 2, 0) * (lrf - 1) + 1
        else:
            self.lf = lambda x: max(1 - x / self.epochs, 0) * (1.0 - lrf) + lrf
        self.nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1
        self.warmup_momentum, self.warmup_bias_lr = float(warmup_momentum), float(warmup_bias_lr)
        self.nbs, self.batch = nbs, batch
        self.last_epoch = 0
        for g in opt.param_groups:  # LambdaLR.__init__: initial_lr, then the factor of epoch 0
            g.setdefault("initial_lr", g["lr"])
        self.momentum = [g.get("momentum") for g in opt.param_groups]  # the scheduled value the warm-up rises to
        self._apply_epoch()

    def _apply_epoch(self):
        for g in self.opt.param_groups:
            g["lr"] = g["initial_lr"] * self.lf(self.last_epoch)
        self.opt.set_hyper()

    def iteration(self, ni, epoch):
        """before the step of iteration ni = i + nb*epoch"""
        if ni > self.nw:
            return
        xi = [0, self.nw]
        for j, g in enumerate(self.opt.param_groups):
            g["lr"] = float(np.interp(ni, xi, [self.warmup_bias_lr if j == 0 else 0.0, g["initial_lr"] * self.lf(epoch)]))
            if "momentum" in g:
                g["momentum"] = float(np.interp(ni, xi, [self.warmup_momentum, self.momentum[j]]))
        self.opt.set_hyper()

    def epoch_end(self, epoch=None):
        """`scheduler.last_epoch = epoch; scheduler.step()`: the factor of the next epoch"""
        self.last_epoch = (self.last_epoch if epoch is None else int(epoch)) + 1
        self._apply_epoch()

    def accumulate(self, ni):
        """the reference's number of batches per optimizer step at iteration ni (only the number: nothing here accumulates)"""
        if self.nw <= 0:
            return max(round(self.nbs / self.batch), 1)
        return max(1, int(np.interp(min(ni, self.nw), [0, self.nw], [1, self.nbs / self.batch]).round()))


class ModelEMA:
    """utils/torch_utils.py:416-443: exponential moving average of every floating-point state_dict tensor (parameters AND
    BatchNorm running statistics), decay ramp `decay * (1 - exp(-updates / tau))`, one multi-tensor launch per update.

    The reference walks the EMA model's state_dict KEYS; the one-to-one head branches are registered under two names each
    (`o2o_heads.*` and `cls/o2d/...`, nn/modules/head.py:627-629), so those tensors receive the update twice per call.  The table
    keeps that multiplicity (`reps`), because matching the reference's EMA weights bit for bit needs it."""

    def __init__(self, model, decay=0.9999, tau=2000, updates=0):
        self.ema = copy.deepcopy(model).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / tau))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.enabled = True
        self._tab = None

    def _tables(self, model):
        esd = self.ema.state_dict(keep_vars=True)   # keep_vars: the live tensors, so that re-pointed storage is noticed
        msd = model.state_dict(keep_vars=True)
        pairs, index = [], {}
        for k, v in esd.items():
            if not v.dtype.is_floating_point:
                continue
            m = msd[k]
            if v.dtype != torch.float32 or m.dtype != torch.float32 or not (v.is_contiguous() and m.is_contiguous()):
                raise Y3DError(f"ModelEMA: {k} must be a contiguous fp32 tensor on both models")
            if v.shape != m.shape:
                raise Y3DError(f"ModelEMA: {k} has shape {tuple(v.shape)} in the EMA model and {tuple(m.shape)} in the model")
            j = index.get(v.data_ptr())
            if j is None:
                index[v.data_ptr()] = len(pairs)
                pairs.append([v, m, 1])
            else:
                pairs[j][2] += 1
        dev = pairs[0][0].device
        if dev.type != "cuda":
            raise Y3DError("ModelEMA needs the models on a HIP device")
        tb = self._tab = mt.Table([v.numel() for v, _, _ in pairs], dev)
        tb.column("ema", pinned=False)  # plain uploads: the addresses move when storage is re-pointed, not from step to step
        tb.column("model", pinned=False)
        self._pairs, self._model = pairs, model
        self._reps = torch.tensor([r for _, _, r in pairs], dtype=torch.int32, device=dev)
        return tb

    @torch.no_grad()
    def update(self, model, guard=None):
        """guard: FusedSGD / FusedAdamW `.last_norm` of the optimizer step this update follows - the update is then skipped on the
        device when that step was (the reference's line runs unconditionally, engine/trainer.py:574-575, and re-applies the decay to
        an unchanged model; guard=None keeps that arithmetic)"""
        if not self.enabled:
            return
        self.updates += 1
        d = self.decay(self.updates)
        tb = self._tab
        if tb is None or self._model is not model:
            tb = self._tables(model)
        ekey = [v.data_ptr() for v, _, _ in self._pairs]
        if len(set(ekey)) != len(ekey):  # storage re-pointed so that entries merged or split: rebuild the multiplicities
            tb = self._tables(model)
            ekey = [v.data_ptr() for v, _, _ in self._pairs]
        eptr = tb.col["ema"].refresh(ekey)
        mptr = tb.col["model"].refresh([m.data_ptr() for _, m, _ in self._pairs])
        ops.bump_param_epoch()
        lib().mt_ema(eptr.data_ptr(), mptr.data_ptr(), tb.sizes.data_ptr(), self._reps.data_ptr(), *tb.chunks, float(d), float(1 - d),
                     guard.data_ptr() if guard is not None else None, ops.stream())

    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        """utils/torch_utils.py:445-448 / copy_attr :342-349"""
        if self.enabled:
            for k, v in model.__dict__.items():
                if (len(include) and k not in include) or k.startswith("_") or k in exclude:
                    continue
                setattr(self.ema, k, v)


ACC_ALIGN = 4  # elements: every arena view starts on a 16-byte boundary, so the accumulate launch takes its 16-byte path


def accum_layout(sizes, chunk=CHUNK, align=ACC_ALIGN):
    """Host only: the arena of GradAccumulator for tensors of `sizes` elements.  -> (offsets, total): tensor t owns arena elements
    [offsets[t], offsets[t] + sizes[t]), every offset a multiple of `align`, `total` the arena's length"""
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += (int(n) + align - 1) // align * align
    return offs, pos


class GradAccumulator:
    """The gradient sum of the `accumulate` micro-batches of one optimizer step (engine/trainer.py:384-386, 411-413) in a flat fp32
    arena, one `y3d_mt_grad_acc` launch per micro-batch instead of autograd's one add per parameter tensor:

        loss.backward(); acc.add()      # every micro-batch: arena += p.grad for every parameter, p.grad = None
        acc.bind(); opt.step(); acc.reset()

    The arena of zeros is allocated on first use; parameter i owns the view `views[i]` at a multiple of 4 elements.  The first add()
    after a reset() fixes the window's active set (the parameters that carry a gradient); a later add() with another set raises before
    anything is launched - autograd would tolerate it, the tables do not.  bind() hands the arena views to the optimizer as `p.grad`:
    fixed addresses, so its gradient pointer table is uploaded once.  reset() zeroes the arena, takes the views off the parameters and
    forgets the set.  `count`: adds since the last reset."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("GradAccumulator: no parameters")
        self.sizes = [p.numel() for p in self.params]
        self.offsets, self.total = accum_layout(self.sizes)
        self.arena = self.views = None
        self.count = 0
        self._active = None
        self._tabs = {}
        self._bound = False

    def _ensure(self):
        if self.arena is None:
            dev = self.params[0].device
            if dev.type != "cuda":
                raise Y3DError("GradAccumulator needs parameters on a HIP device")
            self.arena = torch.zeros(self.total, dtype=torch.float32, device=dev)
            self.views = [self.arena[o:o + n].view_as(p) for o, n, p in zip(self.offsets, self.sizes, self.params)]
        return self.arena

    def _table(self, active):
        key = tuple(active)
        tb = self._tabs.get(key)
        if tb is None:
            dev = self._ensure().device
            tb = self._tabs[key] = mt.Table([self.sizes[i] for i in active], dev, arena=[self.views[i].data_ptr() for i in active])
            tb.column("grads")
        return tb

    @torch.no_grad()
    def add(self, uploader=None):
        """arena += p.grad over every parameter that has one, then p.grad = None.  uploader: a PtrUploader of the caller's (a hipGraph
        capture keeps one of depth 1 alive for its replays); by default the accumulator's own rotating one, written only when the
        gradient addresses changed"""
        active = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not active:
            raise Y3DError("GradAccumulator.add: no parameter has a gradient")
        if self._bound:
            raise Y3DError("GradAccumulator.add: the arena is bound as the parameters' gradients (bind()): reset() first")
        if self._active is not None and active != self._active:
            raise Y3DError(f"GradAccumulator.add: {len(active)} parameters carry a gradient, the window began with {len(self._active)} "
                           "(the active set may not change between reset() calls)")
        tb = self._table(active)
        grads = tb.fp32_contiguous([self.params[i].grad for i in active])
        if len(tb.host_sizes) != len(grads):
            raise Y3DError(f"GradAccumulator.add: a table of {len(tb.host_sizes)} tensors for {len(grads)} gradients")
        for i, g, n in zip(active, grads, tb.host_sizes):
            if not (n == self.params[i].numel() == g.numel()):
                raise Y3DError(f"GradAccumulator.add: parameter {i} has {self.params[i].numel()} elements, its gradient {g.numel()}, "
                               f"the table {n}")
        gkey = [g.data_ptr() for g in grads]
        if uploader is not None:
            if uploader.n != len(gkey):
                raise Y3DError(f"GradAccumulator.add: the uploader holds {uploader.n} pointers, {len(gkey)} gradients")
            gptr = uploader.upload(gkey)
        else:
            gptr = tb.col["grads"].refresh(gkey)
        lib().mt_grad_acc(tb.ptr["arena"].data_ptr(), gptr.data_ptr(), tb.sizes.data_ptr(), *tb.chunks, ops.stream())
        for i in active:
            self.params[i].grad = None
        self._active = active
        self.count += 1

    def bind(self):
        """p.grad = the arena view, for the window's active set"""
        if self._active is None:
            raise Y3DError("GradAccumulator.bind: nothing was added since the last reset()")
        for i in self._active:
            self.params[i].grad = self.views[i]
        self._bound = True

    def reset(self):
        if self.arena is not None:
            self.arena.zero_()
        if self._bound:
            for i in self._active:
                if self.params[i].grad is self.views[i]:
                    self.params[i].grad = None
        self._active, self._bound, self.count = None, False, 0


OPTIMIZERS = ("Adam", "Adamax", "AdamW", "NAdam", "RAdam", "SGD", "auto")


def reference_groups(model, decay=5e-4):
    """the reference's three parameter groups (engine/trainer.py:766-790): biases, weights (decay), normalisation weights"""
    g = [], [], []
    bn = tuple(v for k, v in torch.nn.__dict__.items() if "Norm" in k)
    seen = set()
    for mod in model.modules():
        for pn, p in mod.named_parameters(recurse=False):
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            if pn == "bias":
                g[2].append(p)
            elif isinstance(mod, bn):
                g[1].append(p)
            else:
                g[0].append(p)
    return [{"params": g[2], "weight_decay": 0.0}, {"params": g[0], "weight_decay": decay}, {"params": g[1], "weight_decay": 0.0}]


def build_optimizer(model, lr=0.01, momentum=0.937, decay=5e-4, name="SGD", iterations=1e5, device_momentum=False):
    """reference_groups(model, decay) under "SGD" (nesterov), "Adam" / "Adamax" / "AdamW" / "NAdam" / "RAdam" (betas = (momentum, 0.999);
    engine/trainer.py:776-781), or "auto" (:755-764): SGD(0.01, 0.9) for more than 10 000 iterations, else
    AdamW(round(0.002 * 5 / (4 + nc), 6), 0.9) - `lr` and `momentum` are then ignored and the reference sets warmup_bias_lr = 0;
    the choice is exposed as `opt.auto` = {"name", "lr", "momentum", "warmup_bias_lr"} (None for every other name).
    device_momentum: FusedSGD's switch.
    The one name of the reference's list that is NOT taken here is "RMSProp": it raises NotImplementedError as every unknown name does,
    which tests/test_host_logic.py pins; the optimizer itself exists - `FusedRMSprop(reference_groups(model, decay), lr=lr,
    momentum=momentum)` is what the reference's :779 builds"""
    auto = None
    if name == "auto":
        nc = getattr(model, "nc", 10)
        lr_fit = round(0.002 * 5 / (4 + nc), 6)
        name, lr, momentum = ("SGD", 0.01, 0.9) if iterations > 10000 else ("AdamW", lr_fit, 0.9)
        auto = {"name": name, "lr": lr, "momentum": momentum, "warmup_bias_lr": 0.0}
    if name == "RMSProp":
        raise NotImplementedError("Optimizer 'RMSProp' is not built by name: construct optim.FusedRMSprop(optim.reference_groups(model, decay), "
                                  "lr=lr, momentum=momentum)")
    if name not in OPTIMIZERS[:-1]:
        raise NotImplementedError(f"Optimizer '{name}' not found in list of available optimizers [{', '.join(OPTIMIZERS)}].")
    groups = reference_groups(model, decay)
    if name == "SGD":
        opt = FusedSGD(groups, lr=lr, momentum=momentum, nesterov=True, device_momentum=device_momentum)
    else:
        cls = {"Adam": FusedAdam, "Adamax": FusedAdamax, "AdamW": FusedAdamW, "NAdam": FusedNAdam, "RAdam": FusedRAdam}[name]
        opt = cls(groups, lr=lr, betas=(momentum, 0.999), weight_decay=0.0)
    opt.auto = auto
    return opt
