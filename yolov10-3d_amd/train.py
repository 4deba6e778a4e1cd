"""The training loop: the reference's `_setup_train` / `_do_train` (engine/trainer.py:307-322, 331-474) over the parts this package
already has - a resident split's `epoch()`, the dual-assignment losses, `build_optimizer`, `optim.Schedule`, `optim.ModelEMA`, the
one-call validators - with the `accumulate` micro-batches of an optimizer step summed by `optim.GradAccumulator` (one launch per
micro-batch).  Micro-batches are launched eagerly; `graph.GraphedTrainStep` cannot express "backward without a step".

    trainer = y3d.train.Trainer(model, kitti.DeviceSplit(root), lambda m: val.Validator3d(m, val_split, batch=64, plots=False),
                                epochs=100, batch=32, save_dir="runs/s3d")
    trainer.fit()

What is restated, line by line (engine/trainer.py):
  :307      accumulate = max(round(nbs / batch), 1)                                    plan()
  :308      weight_decay * batch * accumulate / nbs                                    scaled_weight_decay()
  :309      iterations = ceil(n / max(batch, nbs)) * epochs -> build_optimizer         optimizer_iterations()
  :320      EarlyStopping(patience) (utils/torch_utils.py:553-595)                     EarlyStopping
  :331-332  nb, nw                                                                     plan()
  :365-371  close_mosaic / close_mixup: args.mosaic / args.mixup = 0 from epochs - close_* on
  :377      optimizer.zero_grad() at the epoch start (drops a leftover micro-batch)    accum.reset()
  :384-393  warm-up of accumulate, lr and momentum                                     plan(), Schedule.iteration
  :403-405  tloss running mean (on the device; read back once per epoch)
  :411-413  ni - last_opt_step >= accumulate -> optimizer_step                         plan()
  :442      ema.update_attr
  :445-449  when to validate, save_metrics (results.csv), the stopper
  :454-455, :514-541  last.pt / best.pt / epoch{n}.pt
  :470      scheduler.step()                                                           Schedule.epoch_end
  :567-575  clip, step, zero_grad, ema.update                                          accum.bind / opt.step / accum.reset / ema.update
  :588-591  best_fitness
  :695-720  resume

Where this loop differs, on purpose: a checkpoint holds state_dicts (the reference pickles the model objects and halves the EMA), the
EMA stays fp32; a resumed run continues exactly where the straight run would be - the learning-rate factor of the epoch it starts, the
accumulation window (`last_opt_step` comes from plan(), which always counts from epoch 0) and the random streams are restored, where the
reference restarts its window counter and keeps the previous epoch's factor for one epoch; a step with a non-finite gradient norm is
skipped on the device and the EMA update with it (optim.FusedSGD.step); there is no GradScaler (bf16 needs none), no callbacks but one
`on_epoch_end` hook, no
plots of training samples, no time limit, no AutoBatch, no multi-GPU.

Frozen layers (`freeze`, engine/trainer.py:247-267): `freeze_layer_names` / `apply_freeze` restate the rule; the autograd functions of
ops.py read `needs_input_grad` per parameter, so a frozen layer launches no weight gradient and a frozen prefix no backward at all.

Hierarchical task learning (`htl`, engine/trainer.py:349-358, 398-400, 498-512 + utils/htl.py): `HtlWeights` keeps the reference's
`Hierarchical_Task_Learning` state on the device and `y3d_htl_update` restates `compute_weight` there; the criterion reads the 12 weights
from that table (loss.DetectLoss3d.set_item_weights -> y3d_loss3d_weighted), so nothing about the weights crosses to the host but the
epoch's one read-back.  Restated with its quirks: the e0 pass runs in train mode under no_grad (BatchNorm statistics move) and divides
by the number of batches; from the second epoch on the weights come from the LAST micro-batch of the epoch before (:398); the loss is
weights @ items without `* batch_size`; stat_epoch_nums = 5 and max_epochs = 200 whatever the run's `epochs`.  Where it differs, on
purpose: a resumed run restores the state (and the last micro-batch's items) from the checkpoint's optional "htl" entry instead of
repeating the e0 pass with a fresh `Hierarchical_Task_Learning`, and continues bit for bit; a non-finite weight raises Y3DError at the
end of its epoch, naming the items (the reference dies with a KeyError inside its diagnostic print, htl.py:48-51), and the optimizer's
device-side skip rule has kept that epoch's steps from being applied."""
from __future__ import annotations

import math
import os
import random
from datetime import datetime

import numpy as np
import torch

from . import loss as _loss
from . import ops
from ._lib import Y3DError
from .optim import GradAccumulator, ModelEMA, Schedule, build_optimizer

CKPT_KEYS = ("epoch", "best_fitness", "model", "ema", "updates", "optimizer", "train_args", "train_metrics", "history", "rng", "stopper", "date")
EMA_ATTRS = ("yaml", "nc", "args", "names", "stride", "class_weights")  # engine/trainer.py:442


def plan(n, batch, epochs, nbs=64, warmup_epochs=3.0):
    """Host only.  One row (epoch, i, ni, accumulate, step) per iteration of a run over n images: `accumulate` as the reference holds
    it at that iteration (engine/trainer.py:307, 384-386) and whether the optimizer steps after it (:411-413)."""
    n, batch, epochs = int(n), int(batch), int(epochs)
    if n < 1 or batch < 1 or epochs < 1:
        raise Y3DError(f"plan: n = {n}, batch = {batch}, epochs = {epochs}")
    nb = math.ceil(n / batch)
    nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1
    accumulate = max(round(nbs / batch), 1)
    last_opt_step = -1
    rows = []
    for ni in range(nb * epochs):
        if ni <= nw:
            accumulate = max(1, int(np.interp(ni, [0, nw], [1, nbs / batch]).round()))
        step = ni - last_opt_step >= accumulate
        if step:
            last_opt_step = ni
        rows.append((ni // nb, ni % nb, ni, accumulate, step))
    return rows


def scaled_weight_decay(weight_decay, batch, nbs=64):
    """engine/trainer.py:307-308"""
    return weight_decay * batch * max(round(nbs / batch), 1) / nbs


def optimizer_iterations(n, batch, epochs, nbs=64):
    """engine/trainer.py:309: what build_optimizer's `auto` decides on"""
    return math.ceil(n / max(batch, nbs)) * epochs


class EarlyStopping:
    """utils/torch_utils.py:553-595: stop when `patience` epochs have passed without a fitness at least as good as the best"""

    def __init__(self, patience=50):
        self.best_fitness, self.best_epoch = 0.0, 0
        self.patience = patience or float("inf")
        self.possible_stop = False

    def __call__(self, epoch, fitness):
        if fitness is None:
            return False
        if fitness >= self.best_fitness:
            self.best_epoch, self.best_fitness = epoch, fitness
        delta = epoch - self.best_epoch
        self.possible_stop = delta >= self.patience - 1
        return delta >= self.patience

    def state_dict(self):
        return {"best_fitness": self.best_fitness, "best_epoch": self.best_epoch, "patience": self.patience, "possible_stop": self.possible_stop}

    def load_state_dict(self, sd):
        self.best_fitness, self.best_epoch, self.possible_stop = sd["best_fitness"], sd["best_epoch"], sd["possible_stop"]


def better_fitness(best, fitness):
    """engine/trainer.py:589-590 -> the new best_fitness"""
    return fitness if (not best or best < fitness) else best


def validates(epoch, epochs, val_period, possible_stop=False, stop=False, val=True):
    """engine/trainer.py:445-446"""
    return bool((val and ((epoch + 1) % val_period == 0 or (epochs - epoch) <= 10)) or epoch + 1 == epochs or possible_stop or stop)


def preprocess_batch(batch):
    """the builders' (B, H, W, 3) uint8 image as the (B, 3, H, W) view the stem takes; everything else as it is"""
    img = batch["img"]
    if img.dtype == torch.uint8 and img.dim() == 4 and img.shape[-1] == 3 and img.is_contiguous():
        batch = dict(batch)
        batch["img"] = img.permute(0, 3, 1, 2)
    return batch


ALWAYS_FROZEN = (".dfl",)  # engine/trainer.py:255


def _freeze_indices(freeze):
    """the layer indices of a `freeze` setting: None -> none, an int n -> 0..n-1, a list / tuple / range of ints -> themselves"""
    if freeze is None:
        return []
    if isinstance(freeze, bool):
        raise Y3DError(f"freeze = {freeze}: a bool is not a layer count; pass None, an int n (layers 0..n-1) or a list of layer indices")
    if isinstance(freeze, int):
        if freeze < 0:
            raise Y3DError(f"freeze = {freeze}: a layer count cannot be negative")
        return list(range(freeze))
    if isinstance(freeze, (list, tuple, range)):
        idx = list(freeze)
        bad = [i for i in idx if isinstance(i, bool) or not isinstance(i, int) or i < 0]
        if bad:
            raise Y3DError(f"freeze = {freeze!r}: layer indices are non-negative ints (got {bad})")
        return idx
    raise Y3DError(f"freeze = {freeze!r}: pass None, an int n (layers 0..n-1) or a list of layer indices")


def freeze_layer_names(freeze):
    """Host only.  engine/trainer.py:248-256: the substrings that freeze a parameter: "model.{i}." per layer index, then the always
    frozen ".dfl".  A bool is refused (the reference reads True as range(1))."""
    return [f"model.{i}." for i in _freeze_indices(freeze)] + list(ALWAYS_FROZEN)


def normalize_freeze(freeze):
    """the form a checkpoint keeps: None, an int, or a list of ints"""
    _freeze_indices(freeze)
    return freeze if freeze is None or isinstance(freeze, int) else [int(i) for i in freeze]


def apply_freeze(model, freeze):
    """engine/trainer.py:257-267 -> the names of the frozen parameters.  A parameter whose name holds one of `freeze_layer_names(freeze)`
    gets requires_grad = False; a floating-point parameter that matches none and arrives frozen is set back to True.  Where this
    differs, on purpose: a layer index past the model's last layer raises (the reference trains everything, silently); a bool raises; a
    freeze that leaves nothing to train raises; `DepthPredictor.depth_bin_values` - a constant table created with requires_grad =
    False that nothing differentiable reads - stays as it is.  Only the flags change: BatchNorm layers of frozen modules stay in
    training mode, as in the reference.  The flags survive the head's restack (it re-points `.data`, the Parameter objects stay)."""
    idx = _freeze_indices(freeze)
    layers = getattr(model, "model", None)
    nl = len(layers) if hasattr(layers, "__len__") else 0
    bad = sorted({i for i in idx if i >= nl})
    if bad:
        raise Y3DError(f"freeze: layer {', '.join(map(str, bad))} does not exist (the model has layers 0..{nl - 1})")
    names = freeze_layer_names(freeze)
    named = list(model.named_parameters())
    frozen = [k for k, _ in named if any(x in k for x in names)]
    hit = set(frozen)
    if not any(k not in hit and v.dtype.is_floating_point and not k.endswith("depth_bin_values") for k, v in named):
        raise Y3DError(f"freeze = {freeze!r} leaves no trainable parameter")
    for k, v in named:
        if k in hit:
            v.requires_grad = False
        elif not v.requires_grad and v.dtype.is_floating_point and not k.endswith("depth_bin_values"):
            v.requires_grad = True
    model.freeze_layers = sorted(set(idx))  # graph.GraphedTrainStep reads it
    return frozen


HTL_STAT_EPOCHS, HTL_MAX_EPOCHS = 5, 200  # utils/htl.py:4, never overridden by engine/trainer.py:351


def htl_time_value(epoch, max_epochs=HTL_MAX_EPOCHS):
    """utils/htl.py:41, with its literal 5"""
    return min((epoch - 5) / (max_epochs - 5), 1.0)


class HtlWeights:
    """utils/htl.py `Hierarchical_Task_Learning` as device state: the list of past losses (a ring of stat_epochs x 12 floats, oldest first,
    and its fill count), `init_diff` and whether it exists, the 12 weights, and a status word whose bit 0 is set once a weight or their sum
    was not finite.  `table` (12 floats) keeps its address for the life of the object: hand it to `criterion.set_item_weights` once.
    `update(items, epoch)` is `compute_weight(items, epoch)`: one launch, nothing read back."""
    PARTS = (("weights", 0, 12), ("init_diff", 12, 12), ("ring", 24, 96))  # floats of `buf`; int words: 120 count, 121 have_init, 122 status

    def __init__(self, device, stat_epochs=HTL_STAT_EPOCHS, max_epochs=HTL_MAX_EPOCHS):
        device = torch.device(device)
        if device.type != "cuda":
            raise NotImplementedError("HtlWeights (htl): the weight table lives on a HIP device; there is no host path")
        if not 3 <= int(stat_epochs) <= 8:
            raise Y3DError(f"HtlWeights: stat_epochs = {stat_epochs}, 3..8")
        self.stat_epochs, self.max_epochs = int(stat_epochs), int(max_epochs)
        self.buf = torch.zeros(124, dtype=torch.float32, device=device)
        self.table, self.init_diff, self.ring = (self.buf[o:o + n] for _, o, n in self.PARTS)
        self.ints = self.buf[120:124].view(torch.int32)
        self.status = self.ints[2:3]

    def update(self, items, epoch):
        if not (torch.is_tensor(items) and items.is_cuda and items.dtype == torch.float32 and items.numel() == 12 and items.is_contiguous()):
            raise Y3DError("HtlWeights.update: the 12 loss items as contiguous fp32 on the HIP device")
        i = self.ints
        _loss.lib().htl_update(items.data_ptr(), float(htl_time_value(epoch, self.max_epochs)), self.stat_epochs, self.ring.data_ptr(),
                               i[0:].data_ptr(), self.init_diff.data_ptr(), i[1:].data_ptr(), self.table.data_ptr(), i[2:].data_ptr(), ops.stream())
        return self.table

    def state_dict(self):
        sd = {k: self.buf[o:o + n].cpu().clone() for k, o, n in self.PARTS}
        ints = self.ints.cpu()
        return {**sd, "count": int(ints[0]), "have_init": int(ints[1]), "status": int(ints[2]), "stat_epochs": self.stat_epochs,
                "max_epochs": self.max_epochs}

    def load_state_dict(self, sd):
        if sd["stat_epochs"] != self.stat_epochs or sd["max_epochs"] != self.max_epochs:
            raise Y3DError(f"HtlWeights: the state was kept for stat_epochs = {sd['stat_epochs']}, max_epochs = {sd['max_epochs']}")
        for k, o, n in self.PARTS:
            self.buf[o:o + n].copy_(sd[k])
        self.ints.copy_(torch.tensor([sd["count"], sd["have_init"], sd["status"], 0], dtype=torch.int32))


class Trainer:
    """`Trainer(model, train_split, validator).fit()`; see the module docstring.  Defaults: the reference's cfg/default.yaml.

    train_split: anything with `__len__` and `epoch(batch, args, shuffle=, seed=)` that yields batch dicts on the model's device (the
    four resident splits).  validator: `model -> callable -> results dict with "fitness"`, called once with the EMA model.
    fit() seeds numpy, torch and random with `seed` (a resumed run restores their states instead); epoch e is drawn with seed + e.
    htl: hierarchical task learning (module docstring); None follows `model.args.htl`.  3D models only, not with distillation.
    freeze: None, an int n (layers 0..n-1) or a list of layer indices (`apply_freeze`); kept in `train_args`, so a resumed run re-freezes
    the same names.  Frozen layers keep BatchNorm in training mode (batch statistics; their running statistics and the EMA move on).
    After fit(): `history` (one dict per epoch: epoch, the loss items by name, htl/<name> weights when htl is on, lr/pg*, the validation
    results, fitness),
    `best_fitness`, `ema`, `opt`."""

    def __init__(self, model, train_split, validator=None, epochs=400, batch=32, nbs=64, optimizer="auto", lr0=0.001, lrf=0.01, momentum=0.937,
                 weight_decay=0.0005, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, cos_lr=False, close_mixup=0, close_mosaic=0,
                 val_period=1, patience=150, save_dir=None, save_period=-1, seed=0, data_args=None, max_norm=10.0, resume=None, htl=None,
                 freeze=None):
        if htl is None:
            htl = getattr(getattr(model, "args", None), "htl", False)
        margs = getattr(model, "args", None)
        if htl and getattr(margs, "fgdm_loss", False):
            raise NotImplementedError("Trainer: htl with fgdm_loss: 12 weights for 13 items, as with distillation; set one of them off")
        head = model.model[-1] if hasattr(model, "model") else None
        if getattr(head, "fgdm_pred", False) and not getattr(margs, "fgdm_loss", False):
            raise Y3DError("Trainer: the head was built with fgdm_predictor but fgdm_loss is off: the depth predictor's parameters would "
                           "never get a gradient; set fgdm_loss: True (and load_depth_maps: True in the data args) or build the head without it")
        if htl:
            if next(model.parameters()).device.type != "cuda":
                raise NotImplementedError("Trainer: htl (hierarchical task learning) keeps its weight table on the device and weights the "
                                          "items in the loss kernels: the model must live on a HIP device (no host path)")
            from .tasks import YOLOv10_3DDetectionModel
            if not isinstance(model, YOLOv10_3DDetectionModel):
                raise NotImplementedError("Trainer: htl weights the 12 items of the 3D loss; a 2D model's reference items carry no graph")
            if getattr(model.args, "distillation", False):
                raise NotImplementedError("Trainer: htl with distillation: the reference multiplies 12 weights into 14 items")
        if int(batch) < 1 or int(epochs) < 1:
            raise Y3DError(f"Trainer: batch = {batch}, epochs = {epochs}")
        import torch.distributed as dist
        if isinstance(model, torch.nn.parallel.DistributedDataParallel) or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            raise Y3DError("Trainer: single GPU only (ddp.FlatGradReducer and its no_sync stay the caller's)")
        self.ckpt = None
        if resume is not None:
            self.ckpt = torch.load(resume, map_location="cpu", weights_only=False)
            missing = [k for k in CKPT_KEYS if k not in self.ckpt]
            if missing:
                raise Y3DError(f"Trainer: {resume} is not a checkpoint of this trainer (no {', '.join(missing)})")
            if self.ckpt["epoch"] + 1 >= int(epochs) or self.ckpt["epoch"] < 0:
                raise Y3DError(f"{resume} training to {int(epochs)} epochs is finished, nothing to resume.\n"
                               "Start a new training without resuming, i.e. Trainer(...) without resume")
            # the freeze is the checkpoint's (checkpoints from before `freeze` froze nothing); an explicit one has to agree with it
            kept = self.ckpt["train_args"].get("freeze")
            if freeze is not None and normalize_freeze(freeze) != kept:
                raise Y3DError(f"Trainer: freeze = {freeze!r} disagrees with the checkpoint's freeze = {kept!r}: a resumed run keeps the "
                               "frozen set it was started with (its optimizer state is laid out over the trainable parameters)")
            freeze = kept
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise Y3DError(f"Trainer: the model must live on a HIP device, not {dev} (no host fallback)")
        n = len(train_split)
        if n < 1:
            raise Y3DError("Trainer: the training split is empty")
        self.model, self.split, self.make_validator, self.device = model, train_split, validator, dev
        self.epochs, self.batch, self.nbs = int(epochs), int(batch), int(nbs)
        self.train_args = dict(epochs=self.epochs, batch=self.batch, nbs=self.nbs, optimizer=optimizer, lr0=lr0, lrf=lrf, momentum=momentum,
                               weight_decay=weight_decay, warmup_epochs=warmup_epochs, warmup_momentum=warmup_momentum,
                               warmup_bias_lr=warmup_bias_lr, cos_lr=bool(cos_lr), close_mixup=close_mixup, close_mosaic=close_mosaic,
                               val_period=val_period, patience=patience, save_period=save_period, seed=seed, max_norm=max_norm,
                               freeze=normalize_freeze(freeze))
        self.val_period, self.save_period, self.seed, self.max_norm = int(val_period), int(save_period), int(seed), max_norm
        self.close_mixup, self.close_mosaic = int(close_mixup), int(close_mosaic)
        self.save_dir = save_dir
        if data_args is None:
            from . import kitti
            data_args = kitti.data_args()
        self.data_args = data_args
        self.nb = math.ceil(n / self.batch)
        self.plan = plan(n, self.batch, self.epochs, self.nbs, warmup_epochs)
        # engine/trainer.py:247-267, before the optimizer, the EMA and the accumulator size their tables from the flags
        self.frozen = apply_freeze(model, freeze)
        # engine/trainer.py:307-317
        self.opt = build_optimizer(model, name=optimizer, lr=lr0, momentum=momentum, decay=scaled_weight_decay(weight_decay, self.batch, self.nbs),
                                   iterations=optimizer_iterations(n, self.batch, self.epochs, self.nbs), device_momentum=True)
        if self.opt.auto is not None:
            warmup_bias_lr = self.opt.auto["warmup_bias_lr"]  # :763
        for m in model.modules():  # the fused head's stacked storage, before the EMA copies the model
            if hasattr(m, "restack"):
                m.restack()
        self.ema = ModelEMA(model)
        # ... and the copy's own, before its first update: a restack REPLACES the BatchNorm buffer objects of the head, ModelEMA's table
        # holds the objects it found at its first update, and the validator's forward would otherwise restack the copy behind its back
        # (the updates after the first validation would then go to the orphaned buffers)
        for m in self.ema.ema.modules():
            if hasattr(m, "restack"):
                m.restack()
        self.sched = Schedule(self.opt, self.epochs, self.nb, lrf=lrf, cos_lr=cos_lr, warmup_epochs=warmup_epochs, warmup_momentum=warmup_momentum,
                              warmup_bias_lr=warmup_bias_lr, nbs=self.nbs, batch=self.batch)
        self.stopper, self.stop = EarlyStopping(patience), False
        # no arena when no window of the run holds more than one micro-batch
        self.accum = GradAccumulator(model.parameters()) if max(r[3] for r in self.plan) > 1 else None
        self.names = _loss.loss_names(getattr(model, "args", None))
        self.history, self.best_fitness, self.fitness, self.metrics = [], None, None, {}
        self.start_epoch = 0
        self.validator = None
        self.on_epoch_end = None  # callable(history row): tools/train.py prints its line from it
        self.htl, self._ei = None, None  # the weight state; the loss items the next update takes (engine/trainer.py:350, 398)
        if htl:
            self.htl = HtlWeights(dev)
            if not hasattr(model, "criterion"):
                model.criterion = model.init_criterion()
            model.criterion.set_item_weights(self.htl.table)
        if self.ckpt is not None:
            self._resume(self.ckpt)

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------------
    def _resume(self, ck):
        """engine/trainer.py:695-720, and everything else the run holds"""
        self.model.load_state_dict(ck["model"])
        self.ema.ema.load_state_dict(ck["ema"])
        self.ema.updates = ck["updates"]
        self.opt.load_state_dict(ck["optimizer"])  # torch's layout, then the native counters behind it
        self.best_fitness, self.history = ck["best_fitness"], list(ck["history"])
        self.stopper.load_state_dict(ck["stopper"])
        self.start_epoch = ck["epoch"] + 1
        self.sched.epoch_end(ck["epoch"])  # the factor of the epoch the run continues with
        if self.htl is not None:
            if "htl" not in ck:
                raise Y3DError("Trainer: htl is on and the checkpoint holds no htl state (it was written by a run without htl)")
            self.htl.load_state_dict(ck["htl"]["state"])
            self._ei = ck["htl"]["items"].to(self.device).float().contiguous()
        ops.bump_weight_epoch()

    def checkpoint(self, epoch):
        opt_sd = self.opt.state_dict(torch_format=True, native=True)
        cpu = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
        # numpy's state with its key array as a tensor: the file then holds tensors and plain Python values only, so that
        # BaseModel.load_pretrained_body can read it with weights_only=True
        kind, keys, *rest = np.random.get_state()
        rng = {"numpy": (kind, torch.from_numpy(keys.astype(np.int64)), *rest), "torch": torch.get_rng_state(), "torch_cuda": torch.cuda.get_rng_state(self.device),
               "random": random.getstate()}
        ck = {"epoch": epoch, "best_fitness": self.best_fitness, "model": cpu(self.model.state_dict()),
              "ema": {k: (v.float() if v.is_floating_point() else v) for k, v in cpu(self.ema.ema.state_dict()).items()},
              "updates": self.ema.updates, "optimizer": opt_sd, "train_args": dict(self.train_args),
              "train_metrics": {**self.metrics, "fitness": self.fitness}, "history": list(self.history), "rng": rng,
              "stopper": self.stopper.state_dict(), "date": datetime.now().isoformat()}
        if self.htl is not None:  # optional: CKPT_KEYS is what every checkpoint holds
            ck["htl"] = {"state": self.htl.state_dict(), "items": self._ei.detach().cpu().clone()}
        return ck

    def _e0_loss(self):
        """engine/trainer.py:498-512 compute_e0_loss: one pass over the training data in train mode under no_grad (BatchNorm running
        statistics move), the 12 items summed and divided by the number of batches (a short last batch counts like any other)"""
        self.model.train()
        total, n = None, 0
        with torch.no_grad():
            # an order of its own, seed - 1 (epoch e draws seed + e); modulo 2^32: the splits seed a RandomState, which takes no -1
            for batch in self.split.epoch(self.batch, self.data_args, shuffle=True, seed=(self.seed - 1) % (1 << 32)):
                _, items = self.model(preprocess_batch(batch))
                items = items.detach().float()
                total = items.clone() if total is None else total + items
                n += 1
        return (total / n).contiguous()

    def _save(self, epoch):
        """engine/trainer.py:536-541"""
        wdir = os.path.join(self.save_dir, "weights")
        os.makedirs(wdir, exist_ok=True)
        ck = self.checkpoint(epoch)
        torch.save(ck, os.path.join(wdir, "last.pt"))
        if self.best_fitness == self.fitness:
            torch.save(ck, os.path.join(wdir, "best.pt"))
        if self.save_period > 0 and epoch > 0 and epoch % self.save_period == 0:
            torch.save(ck, os.path.join(wdir, f"epoch{epoch}.pt"))

    def _save_metrics(self, epoch, row):
        """engine/trainer.py:639-645"""
        os.makedirs(self.save_dir, exist_ok=True)
        path = os.path.join(self.save_dir, "results.csv")
        keys, vals = list(row), list(row.values())
        n = len(row) + 1
        head = "" if os.path.exists(path) else (("%23s," * n % tuple(["epoch"] + keys)).rstrip(",") + "\n")
        with open(path, "a") as f:
            f.write(head + ("%23.5g," * n % tuple([epoch + 1] + vals)).rstrip(",") + "\n")

    # ---- one micro-batch -----------------------------------------------------------------------------------------------------------
    def _micro(self, batch):
        """forward + loss + backward (+ accumulate) of one micro-batch -> loss items"""
        loss, items = self.model(preprocess_batch(batch))
        loss.backward()
        del loss
        if self.accum is not None:
            self.accum.add()
        return items

    def _optimizer_step(self):
        """engine/trainer.py:567-575"""
        if self.accum is not None:
            self.accum.bind()
        self.opt.step(max_norm=self.max_norm)
        if self.accum is not None:
            self.accum.reset()
        else:
            self.opt.zero_grad(set_to_none=True)
        self.ema.update(self.model, guard=self.opt.last_norm)

    # ---- the loop ------------------------------------------------------------------------------------------------------------------
    def fit(self):
        if self.ckpt is None:
            random.seed(self.seed)
            np.random.seed(self.seed)
            torch.manual_seed(self.seed)
        else:
            rng = self.ckpt["rng"]
            random.setstate(rng["random"])
            kind, keys, *rest = rng["numpy"]  # (older checkpoints keep the key array as numpy's)
            np.random.set_state((kind, np.asarray(keys.numpy() if torch.is_tensor(keys) else keys, dtype=np.uint32), *rest))
            torch.set_rng_state(rng["torch"])
            torch.cuda.set_rng_state(rng["torch_cuda"], self.device)
            self.ckpt = None
        if self.make_validator is not None and self.validator is None:
            self.validator = self.make_validator(self.ema.ema)
        model, args = self.model, self.data_args
        if self.htl is not None and self._ei is None:
            self._ei = self._e0_loss()  # :349-350
        for epoch in range(self.start_epoch, self.epochs):
            self.epoch = epoch
            if self.htl is not None:
                self.htl.update(self._ei, epoch)  # :357-358
            model.train()
            if self.close_mosaic > 0 and epoch >= self.epochs - self.close_mosaic and hasattr(args, "mosaic"):
                args.mosaic = 0.0
            if self.close_mixup > 0 and epoch >= self.epochs - self.close_mixup and hasattr(args, "mixup"):
                args.mixup = 0.0
            # :377 zero_grad: a micro-batch left over from the last epoch's final window is dropped
            if self.accum is not None:
                self.accum.reset()
            self.opt.zero_grad(set_to_none=True)
            tloss = None
            for i, batch in enumerate(self.split.epoch(self.batch, args, shuffle=True, seed=self.seed + epoch)):
                _, _, ni, _, step = self.plan[epoch * self.nb + i]
                self.sched.iteration(ni, epoch)
                items = self._micro(batch).detach().float()
                tloss = items.clone() if tloss is None else (tloss * i + items) / (i + 1)
                if self.htl is not None:
                    self._ei = items.contiguous()  # :398 the last micro-batch's items, not the epoch mean, feed the next update
                if step:
                    self._optimizer_step()
            lr = {f"lr/pg{j}": g["lr"] for j, g in enumerate(self.opt.param_groups)}
            self.ema.update_attr(model, include=EMA_ATTRS)
            final = epoch + 1 == self.epochs
            if self.validator is not None and validates(epoch, self.epochs, self.val_period, self.stopper.possible_stop, self.stop):
                self.metrics = {k: float(v) for k, v in self.validator().items()}
                self.fitness = self.metrics.pop("fitness", None)
                self.best_fitness = better_fitness(self.best_fitness, self.fitness)
            hw = {}
            if self.htl is not None:  # the weights and the status word ride on the same read-back
                tloss = torch.cat((tloss, self.htl.table, self.htl.status.float())).cpu()
                tloss, w, status = tloss[:-13], tloss[-13:-1], int(tloss[-1])
                hw = {f"htl/{k}": float(v) for k, v in zip(self.names, w)}
                if status & 1:
                    bad = [k for k, v in zip(self.names, w) if not math.isfinite(float(v))]
                    raise Y3DError(f"Trainer: htl weights not finite in epoch {epoch}: {', '.join(bad) or 'their sum'} "
                                   f"(weights {[float(v) for v in w]}); the optimizer skipped the steps that saw them")
            else:
                tloss = tloss.cpu()  # the epoch's one read-back of the loss items
            names = self.names if len(self.names) == tloss.numel() else [f"loss_{j}" for j in range(tloss.numel())]  # (2D models)
            losses = dict(zip(names, (float(v) for v in tloss)))
            row = {**{f"train/{k}": v for k, v in losses.items()}, **hw, **self.metrics, **lr}
            self.history.append({"epoch": epoch, **losses, **hw, **lr, **self.metrics, "fitness": self.fitness})
            self.stop |= self.stopper(epoch + 1, self.fitness) or final
            if self.save_dir is not None:
                self._save_metrics(epoch, row)
                self._save(epoch)
            self.sched.epoch_end(epoch)
            if self.on_epoch_end is not None:
                self.on_epoch_end(self.history[-1])
            if self.stop:
                break
        return self.history
