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

from . import ops
from ._lib import Y3DError, lib

CHUNK = 16384
# indices into the step-scalar array (include/y3d.h, y3d_mt_step_scalars) and y3d_mt_update's kinds
S_BC1, S_BC2, S_BC1_SQRT, S_BC2_SQRT, S_MU, S_MU_NEXT, S_MU_PROD, S_MU_PROD_NEXT, S_RHO, S_RECT_ON, S_RECT, S_T, S_NADAM_G, S_NADAM_M = range(14)
OPT_ADAM, OPT_ADAMAX, OPT_NADAM, OPT_RADAM, OPT_RMSPROP = range(5)


class PtrUploader:
    """Pointer tables that change every step (the step's gradient tensors) go to the device through rotating PINNED host buffers
    with a non-blocking copy: `torch.tensor(list, device=...)` stages through pageable memory and holds the host until the stream
    has drained, which leaves the GPU idle while the rest of the optimizer's host code runs (measured ~1 ms per step)."""

    def __init__(self, n, device, depth=4):
        import numpy as np
        self.host = [torch.empty(n, dtype=torch.int64).pin_memory() for _ in range(depth)]
        self.np = [h.numpy() for h in self.host]
        self.dev = [torch.empty(n, dtype=torch.int64, device=device) for _ in range(depth)]
        self.i, self.n = 0, n
        self._np = np

    def upload(self, ptrs):
        assert len(ptrs) == self.n
        k = self.i
        self.i = (self.i + 1) % len(self.host)
        self.np[k][:] = self._np.asarray(ptrs, dtype=self._np.int64)
        self.dev[k].copy_(self.host[k], non_blocking=True)
        return self.dev[k]


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


class FusedSGD:
    NSTATE = 1  # flat zero-initialised state buffers per parameter (SGD: momentum)
    NSCAL = 0   # floats behind the five counters of `norm_clip`: the step scalars of y3d_mt_step_scalars (none for SGD / AdamW)
    TORCH_NAME = "SGD"

    def __init__(self, param_groups, lr=0.01, momentum=0.937, nesterov=True, weight_decay=0.0, device_momentum=False):
        """device_momentum: the groups carry a "momentum" key (as torch's do: the reference's warm-up finds it, engine/trainer.py:392),
        a per-tensor device table holds it next to lr / wd, set_hyper() rewrites it in place and the table-reading kernel
        (y3d_mt_sgd_tab) is launched - so a captured step follows a momentum schedule.  False: momentum is a launch constant."""
        self.device_momentum = bool(device_momentum)
        if isinstance(param_groups, (list, tuple)) and param_groups and not isinstance(param_groups[0], dict):
            param_groups = [{"params": list(param_groups)}]
        self.param_groups = []
        for g in param_groups:
            g = dict(g)
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            if self.device_momentum:
                g.setdefault("momentum", float(momentum))
            g["params"] = [p for p in g["params"] if p.requires_grad]
            self.param_groups.append(g)
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.params = [p for g in self.param_groups for p in g["params"]]
        if not self.params:
            raise ValueError("FusedSGD: no parameters")
        self._state = None
        self._steps = 0
        self.last_norm = None
        self._pending_load = None
        self._seen = set()  # parameters that have carried a gradient (or loaded state): the ones torch would hold state for
        self.auto = None    # build_optimizer(name="auto"): what was chosen

    def add_param_group(self, g):
        g = dict(g)
        g.setdefault("lr", self.param_groups[0]["lr"])
        g.setdefault("weight_decay", 0.0)
        if self.device_momentum:
            g.setdefault("momentum", self.momentum)
        g["params"] = [p for p in g["params"] if p.requires_grad]
        self.param_groups.append(g)
        self.params = [p for gg in self.param_groups for p in gg["params"]]
        self._state = None

    def _build(self, active):
        """tables over the parameters that carry a gradient (torch.optim.SGD and clip_grad_norm_ skip the others, e.g. the neck
        blocks behind a detect level that `num_scales: 2` leaves unused); momentum buffers are zero-initialised, so the first
        update `buf = momentum*0 + g` equals torch's `buf = clone(g)` exactly."""
        dev = self.params[0].device
        if dev.type != "cuda":
            raise Y3DError("FusedSGD needs parameters on a HIP device")
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise Y3DError("FusedSGD: parameters must be contiguous fp32 tensors")
        old = self._state
        if old is None:
            sizes_all = [p.numel() for p in self.params]
            flat = torch.zeros(self.NSTATE, sum(sizes_all), dtype=torch.float32, device=dev)  # state buffers, one allocation
            bufs, off = [], 0
            for n in sizes_all:
                bufs.append(flat[:, off:off + n])
                off += n
        else:
            flat, bufs = old["flat"], old["bufs"]
        sizes = [self.params[i].numel() for i in active]
        ct, co = [], []
        for t, n in enumerate(sizes):
            for c in range((n + CHUNK - 1) // CHUNK):
                ct.append(t)
                co.append(c)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        lr_all = [g["lr"] for g in self.param_groups for _ in g["params"]]
        wd_all = [g["weight_decay"] for g in self.param_groups for _ in g["params"]]
        st = {
            "dev": dev, "flat": flat, "bufs": bufs, "nchunks": len(ct), "active": list(active),
            "sizes": i64(sizes), "ctensor": torch.tensor(ct, dtype=torch.int32, device=dev), "coff": torch.tensor(co, dtype=torch.int32, device=dev),
            "bptr": i64([bufs[i][0].data_ptr() for i in active]),
            "bptr2": i64([bufs[i][1].data_ptr() for i in active]) if self.NSTATE > 1 else None, "partials": torch.empty(len(ct), dtype=torch.float32, device=dev),
            "norm_clip": old["norm_clip"] if old is not None else torch.zeros(5 + self.NSCAL, dtype=torch.float32, device=dev), "pkey": None, "gkey": None,
            "lr": torch.tensor([lr_all[i] for i in active], dtype=torch.float32, device=dev),
            "wd": torch.tensor([wd_all[i] for i in active], dtype=torch.float32, device=dev),
            "hkey": self._hkey(),
        }
        if self.device_momentum:
            mom_all = [g["momentum"] for g in self.param_groups for _ in g["params"]]
            st["mom"] = torch.tensor([mom_all[i] for i in active], dtype=torch.float32, device=dev)
        if self.NSCAL:
            st["scal"] = st["norm_clip"][5:]  # one allocation with the counters: checkpointed and restored with them
        self._seen.update(active)
        self._state = st
        if self._pending_load is not None:  # load_state_dict() before the first step
            sd, self._pending_load = self._pending_load, None
            if "torch" in sd:
                self._apply_torch(*sd["torch"])
            else:
                self.load_state_dict(sd)
        return st

    def _hkey(self):
        if self.device_momentum:
            return [(g["lr"], g["weight_decay"], len(g["params"]), g["momentum"]) for g in self.param_groups]
        return [(g["lr"], g["weight_decay"], len(g["params"])) for g in self.param_groups]

    def _torch_group_hyper(self):
        """the hyper-parameters torch keeps per group, beside lr / weight_decay"""
        return {"momentum": self.momentum, "nesterov": self.nesterov}

    def _take_group_hyper(self, groups):
        """load_state_dict(torch dict): momentum is one launch constant unless device_momentum keeps it per group"""
        moms = {float(g["momentum"]) for g in groups if "momentum" in g}
        if self.device_momentum:
            for g, src in zip(self.param_groups, groups):
                if "momentum" in src:
                    g["momentum"] = float(src["momentum"])
        elif len(moms) > 1:
            raise Y3DError(f"optimizer state with per-group momenta {sorted(moms)}: construct the optimizer with device_momentum=True")
        if len(moms) == 1:
            self.momentum = moms.pop()

    def state_dict(self, torch_format=False):
        """optimizer state for checkpoint / resume (the reference saves `optimizer.state_dict()`, engine/trainer.py:470-486): the flat
        state buffers in parameter order (SGD: momentum; AdamW: exp_avg, exp_avg_sq) and the device-side counters [norm, clip
        coefficient, finite flag, steps APPLIED, steps skipped] - `steps applied` is AdamW's bias-correction step count.

        torch_format: torch.optim's layout instead, as the reference's checkpoints hold it - `state[i]` with torch's keys for this
        optimizer (TORCH_STATE) for every parameter that has been active, `param_groups` with lr, weight_decay, momentum / betas,
        initial_lr when set and `params` indices in group order"""
        st = self._state
        if not torch_format:
            return {"steps": self._steps, "flat": None if st is None else st["flat"].detach().clone(),
                    "norm_clip": None if st is None else st["norm_clip"].detach().clone()}
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
        if st is not None:
            nc = st["norm_clip"].detach().cpu()
            mu = float(nc[5 + S_MU_PROD]) if self.TORCH_NAME == "NAdam" and float(nc[3]) > 0 else None
            state = flat_to_torch_state(self.TORCH_NAME, st["flat"], shapes, sorted(self._seen), step=float(nc[3]), mu_product=mu)
        elif self._pending_load is not None and "torch" in self._pending_load:  # loaded, not stepped yet
            flat, step, mu, present = self._pending_load["torch"]
            state = flat_to_torch_state(self.TORCH_NAME, flat, shapes, present, step=step, mu_product=mu)
        return {"state": state, "param_groups": groups}

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
        st = self._state
        st["flat"].copy_(flat)
        self._seen.update(present)
        if step is not None:  # (torch's SGD keeps no step count: the device counters stay)
            self._steps = int(step)
            nc = st["norm_clip"].detach().cpu()
            nc[3] = step
            if mu is not None:
                nc[5 + S_MU_PROD] = mu
            st["norm_clip"].copy_(nc)

    def load_state_dict(self, sd):
        """inverse of state_dict(), either format; before the first step the state is kept and applied when the tables are built"""
        if is_torch_format(sd):  # torch.optim's layout (a reference checkpoint's `ckpt["optimizer"]`)
            conv = self._convert_torch(sd)  # raises before anything is taken over
            for g, src in zip(self.param_groups, sd["param_groups"]):
                for key in ("lr", "weight_decay", "initial_lr"):
                    if key in src:
                        g[key] = float(src[key])
            self._take_group_hyper(sd["param_groups"])
            if self._state is None:
                self._pending_load = {"torch": conv}
                return
            self._apply_torch(*conv)
            return self.set_hyper()
        if self._state is None:
            self._pending_load = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
            self._steps = int(sd["steps"])
            return
        st = self._state
        self._steps = int(sd["steps"])
        if sd.get("flat") is not None:
            if sd["flat"].shape != st["flat"].shape:
                raise Y3DError(f"optimizer state of shape {tuple(sd['flat'].shape)} does not fit these parameters {tuple(st['flat'].shape)}")
            st["flat"].copy_(sd["flat"])
            st["norm_clip"].copy_(sd["norm_clip"])

    def set_hyper(self):
        """write the groups' current lr / weight_decay (and momentum, with device_momentum) into the EXISTING device tables (in place: a captured hipGraph of the step keeps
        reading them, graph.GraphedTrainStep) - what a scheduler's `param_group["lr"] = ...` needs before the next replay"""
        st = self._state
        if st is None:
            return
        lr_all = [g["lr"] for g in self.param_groups for _ in g["params"]]
        wd_all = [g["weight_decay"] for g in self.param_groups for _ in g["params"]]
        st["lr"].copy_(torch.tensor([lr_all[i] for i in st["active"]], dtype=torch.float32), non_blocking=False)
        st["wd"].copy_(torch.tensor([wd_all[i] for i in st["active"]], dtype=torch.float32), non_blocking=False)
        if self.device_momentum:
            mom_all = [g["momentum"] for g in self.param_groups for _ in g["params"]]
            st["mom"].copy_(torch.tensor([mom_all[i] for i in st["active"]], dtype=torch.float32), non_blocking=False)
        st["hkey"] = self._hkey()

    def _tables(self):
        active = [i for i, p in enumerate(self.params) if p.grad is not None]
        if not active:
            raise Y3DError("FusedSGD.step: no parameter has a gradient")
        st = self._state
        hkey = self._hkey()
        if st is not None and st["active"] == active and st["hkey"] != hkey and [h[2] for h in st["hkey"]] == [h[2] for h in hkey]:
            self.set_hyper()  # only the values moved (a scheduler): same tables, new contents
        if st is None or st["active"] != active or st["hkey"] != hkey:
            st = self._build(active)
        pkey = [self.params[i].data_ptr() for i in active]
        if pkey != st["pkey"]:  # parameters re-pointed (e.g. sibling-branch stacking, .to()): refresh
            st["pptr"] = torch.tensor(pkey, dtype=torch.int64, device=st["dev"])
            st["pkey"] = pkey
        gkey = []
        for i in active:
            p = self.params[i]
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = p.grad = g.float().contiguous()
            gkey.append(g.data_ptr())
        if gkey != st["gkey"]:
            if st.get("gup") is None or st["gup"].n != len(gkey):
                st["gup"] = PtrUploader(len(gkey), st["dev"])
            st["gptr"] = st["gup"].upload(gkey)
            st["gkey"] = gkey
        return st

    @torch.no_grad()
    def step(self, max_norm: float | None = 10.0):
        """clip (when max_norm is given) + update; self.last_norm holds the device tensor [total_norm, clip_coef, finite flag, steps
        applied, steps skipped].  A step whose gradient norm is inf / NaN is skipped ON THE DEVICE (no host synchronisation): parameters,
        momentum / Adam state and AdamW's bias-correction step count stay - torch.cuda.amp.GradScaler.step's rule, engine/trainer.py:
        567-572.  Under ddp.FlatGradReducer the norm is that of the all-reduced buffer, so every rank takes the same decision."""
        st = self._tables()
        L, s = lib(), ops.stream()
        clip = None
        if max_norm is not None:
            L.mt_sqnorm(st["gptr"].data_ptr(), st["sizes"].data_ptr(), st["ctensor"].data_ptr(), st["coff"].data_ptr(), st["nchunks"], CHUNK,
                        st["partials"].data_ptr(), s)
            L.mt_clip_coef(st["partials"].data_ptr(), st["nchunks"], float(max_norm), st["norm_clip"].data_ptr(), s)
            clip = st["norm_clip"].data_ptr()
            self.last_norm = st["norm_clip"][:5] if self.NSCAL else st["norm_clip"]
        self._steps += 1
        self._update(L, st, clip, s)
        ops.bump_weight_epoch()  # the parameters changed behind torch's version counters

    def _update(self, L, st, clip, s):
        if self.device_momentum:
            L.mt_sgd_tab(st["pptr"].data_ptr(), st["gptr"].data_ptr(), st["bptr"].data_ptr(), st["sizes"].data_ptr(), st["lr"].data_ptr(),
                         st["wd"].data_ptr(), st["mom"].data_ptr(), st["ctensor"].data_ptr(), st["coff"].data_ptr(), st["nchunks"], CHUNK,
                         int(self.nesterov), 0, clip, s)
            return
        L.mt_sgd(st["pptr"].data_ptr(), st["gptr"].data_ptr(), st["bptr"].data_ptr(), st["sizes"].data_ptr(), st["lr"].data_ptr(),
                 st["wd"].data_ptr(), st["ctensor"].data_ptr(), st["coff"].data_ptr(), st["nchunks"], CHUNK, self.momentum, int(self.nesterov),
                 0, clip, s)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()


class FusedAdamW(FusedSGD):
    """torch.optim.AdamW(betas, eps, weight_decay per group), amsgrad off; same tables and clipping as FusedSGD"""
    NSTATE = 2  # exp_avg, exp_avg_sq
    TORCH_NAME = "AdamW"

    def __init__(self, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(param_groups, lr=lr, momentum=betas[0], nesterov=False, weight_decay=weight_decay)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

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

    def step(self, max_norm: float | None = 10.0):
        """as FusedSGD.step; without a `max_norm` the clipping launch still runs (with an infinite bound: coefficient 1), because the
        bias corrections read the number of APPLIED steps from its device-side counter - ONE source for the step count, whether or not
        the step is clipped, eager or replayed from a hipGraph, fresh or resumed (round-3 advisor finding).  Side effect: a step with a
        non-finite gradient norm is skipped in that case too."""
        return super().step(max_norm=float("inf") if max_norm is None else max_norm)

    def _update(self, L, st, clip, s):
        b1, b2 = self.betas
        bc1 = 1.0 - b1 ** max(self._steps, 1)  # (placeholders: the kernel recomputes both from the device-side step count)
        bc2s = math.sqrt(1.0 - b2 ** max(self._steps, 1))
        L.mt_adamw(st["pptr"].data_ptr(), st["gptr"].data_ptr(), st["bptr"].data_ptr(), st["bptr2"].data_ptr(), st["sizes"].data_ptr(),
                   st["lr"].data_ptr(), st["wd"].data_ptr(), st["ctensor"].data_ptr(), st["coff"].data_ptr(), st["nchunks"], CHUNK, b1, b2,
                   self.eps, bc1, bc2s, clip, s)


class FusedAdam(FusedAdamW):
    """torch.optim.Adam: coupled L2 decay `g += wd*p` (amsgrad off).  Two launches after the clipping pair: y3d_mt_step_scalars turns
    the device's count of APPLIED steps into the bias corrections (and NAdam's / RAdam's scalars), y3d_mt_update applies them - one
    device-side source for everything that depends on the step, eager or replayed, as FusedAdamW's bias corrections"""
    NSCAL = 16
    KIND = OPT_ADAM
    TORCH_NAME = "Adam"
    MOMENTUM_DECAY = 4e-3  # torch.optim.NAdam's default (read by y3d_mt_step_scalars for every kind; used by NAdam)

    def __init__(self, param_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)

    def _update(self, L, st, clip, s):
        b1, b2 = self.betas
        scal = st["scal"].data_ptr()
        L.mt_step_scalars(clip, b1, b2, self.MOMENTUM_DECAY, scal, s)
        L.mt_update(self.KIND, st["pptr"].data_ptr(), st["gptr"].data_ptr(), st["bptr"].data_ptr(), st["bptr2"].data_ptr(), st["sizes"].data_ptr(),
                    st["lr"].data_ptr(), st["wd"].data_ptr(), None, st["ctensor"].data_ptr(), st["coff"].data_ptr(), st["nchunks"], CHUNK, b1, b2,
                    self.eps, scal, clip, s)


class FusedAdamax(FusedAdam):
    """torch.optim.Adamax: exp_inf = max(beta2*exp_inf, |g| + eps); p -= lr/(1-beta1^t) * exp_avg / exp_inf"""
    KIND = OPT_ADAMAX
    TORCH_NAME = "Adamax"

    def __init__(self, param_groups, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class FusedNAdam(FusedAdam):
    """torch.optim.NAdam (momentum_decay 4e-3, coupled decay); mu_product is the one piece of state among the step scalars"""
    KIND = OPT_NADAM
    TORCH_NAME = "NAdam"

    def __init__(self, param_groups, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(param_groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)


class FusedRAdam(FusedAdam):
    """torch.optim.RAdam (coupled decay): the unrectified arm while rho_t <= 5, the rectified one after"""
    KIND = OPT_RADAM
    TORCH_NAME = "RAdam"


class FusedRMSprop(FusedSGD):
    """torch.optim.RMSprop(alpha, eps, momentum), not centered; the momentum always comes from the per-tensor device table"""
    NSTATE = 2  # square_avg, momentum_buffer
    TORCH_NAME = "RMSprop"

    def __init__(self, param_groups, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0):
        super().__init__(param_groups, lr=lr, momentum=momentum, nesterov=False, weight_decay=weight_decay, device_momentum=True)
        self.alpha, self.eps = float(alpha), float(eps)

    def _torch_group_hyper(self):
        return {"alpha": self.alpha, "eps": self.eps}

    def _take_group_hyper(self, groups):
        super()._take_group_hyper(groups)
        for key in ("alpha", "eps"):
            vals = {float(g[key]) for g in groups if key in g}
            if len(vals) == 1:
                setattr(self, key, vals.pop())

    def _update(self, L, st, clip, s):
        L.mt_update(OPT_RMSPROP, st["pptr"].data_ptr(), st["gptr"].data_ptr(), st["bptr"].data_ptr(), st["bptr2"].data_ptr(),
                    st["sizes"].data_ptr(), st["lr"].data_ptr(), st["wd"].data_ptr(), st["mom"].data_ptr(), st["ctensor"].data_ptr(),
                    st["coff"].data_ptr(), st["nchunks"], CHUNK, 0.0, self.alpha, self.eps, None, clip, s)


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
        ct, co = [], []
        for t, (v, _, _) in enumerate(pairs):
            for c in range((v.numel() + CHUNK - 1) // CHUNK):
                ct.append(t)
                co.append(c)
        i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
        self._tab = {"pairs": pairs, "n": len(ct), "sizes": i64([v.numel() for v, _, _ in pairs]), "reps": i32([r for _, _, r in pairs]),
                     "ct": i32(ct), "co": i32(co), "ekey": None, "mkey": None, "model": model}
        return self._tab

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
        if tb is None or tb["model"] is not model:
            tb = self._tables(model)
        ekey = [v.data_ptr() for v, _, _ in tb["pairs"]]
        mkey = [m.data_ptr() for _, m, _ in tb["pairs"]]
        if len(set(ekey)) != len(ekey):  # storage re-pointed so that entries merged or split: rebuild the multiplicities
            tb = self._tables(model)
            ekey = [v.data_ptr() for v, _, _ in tb["pairs"]]
            mkey = [m.data_ptr() for _, m, _ in tb["pairs"]]
        dev = tb["sizes"].device
        if ekey != tb["ekey"]:
            tb["eptr"], tb["ekey"] = torch.tensor(ekey, dtype=torch.int64, device=dev), ekey
        if mkey != tb["mkey"]:
            tb["mptr"], tb["mkey"] = torch.tensor(mkey, dtype=torch.int64, device=dev), mkey
        ops.bump_param_epoch()
        lib().mt_ema(tb["eptr"].data_ptr(), tb["mptr"].data_ptr(), tb["sizes"].data_ptr(), tb["reps"].data_ptr(), tb["ct"].data_ptr(),
                     tb["co"].data_ptr(), tb["n"], CHUNK, float(d), float(1 - d), guard.data_ptr() if guard is not None else None, ops.stream())

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


def chunk_map(sizes, chunk=CHUNK):
    """Host only: the (chunk_tensor, chunk_off) tables of the multi-tensor launches: workgroup c handles elements
    [chunk_off[c] * chunk, + chunk) of tensor chunk_tensor[c]"""
    ct, co = [], []
    for t, n in enumerate(sizes):
        for c in range((int(n) + chunk - 1) // chunk):
            ct.append(t)
            co.append(c)
    return ct, co


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
            sizes = [self.sizes[i] for i in active]
            ct, co = chunk_map(sizes)
            tb = {"n": len(ct), "host_sizes": sizes, "sizes": torch.tensor(sizes, dtype=torch.int64, device=dev),
                  "ct": torch.tensor(ct, dtype=torch.int32, device=dev), "co": torch.tensor(co, dtype=torch.int32, device=dev),
                  "aptr": torch.tensor([self.views[i].data_ptr() for i in active], dtype=torch.int64, device=dev), "up": None, "gkey": None,
                  "gptr": None}
            self._tabs[key] = tb
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
        grads = []
        for i in active:
            p = self.params[i]
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = p.grad = g.float().contiguous()
            grads.append(g)
        if len(tb["host_sizes"]) != len(grads):
            raise Y3DError(f"GradAccumulator.add: a table of {len(tb['host_sizes'])} tensors for {len(grads)} gradients")
        for i, g, n in zip(active, grads, tb["host_sizes"]):
            if not (n == self.params[i].numel() == g.numel()):
                raise Y3DError(f"GradAccumulator.add: parameter {i} has {self.params[i].numel()} elements, its gradient {g.numel()}, "
                               f"the table {n}")
        gkey = [g.data_ptr() for g in grads]
        if uploader is not None:
            if uploader.n != len(gkey):
                raise Y3DError(f"GradAccumulator.add: the uploader holds {uploader.n} pointers, {len(gkey)} gradients")
            gptr = uploader.upload(gkey)
        else:
            if gkey != tb["gkey"]:
                if tb["up"] is None:
                    tb["up"] = PtrUploader(len(gkey), self.arena.device)
                tb["gptr"], tb["gkey"] = tb["up"].upload(gkey), gkey
            gptr = tb["gptr"]
        lib().mt_grad_acc(tb["aptr"].data_ptr(), gptr.data_ptr(), tb["sizes"].data_ptr(), tb["ct"].data_ptr(), tb["co"].data_ptr(), tb["n"],
                          CHUNK, ops.stream())
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
