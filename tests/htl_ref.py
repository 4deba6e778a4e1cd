"""TEST INFRASTRUCTURE - NumPy restatement of the reference's hierarchical task learning weights (utils/htl.py:23-56
`Hierarchical_Task_Learning.compute_weight`) in float32 and in float64, the loss sequences of tests/golden/htl.npz, and the loader of that
fixture.  Plain NumPy: imports neither torch nor the HIP library.

`Weightor(dtype)` keeps the reference's state (the list of past losses, `init_diff`) and `compute_weight(current_loss, epoch)` returns the 12
weights.  In float32 every operation is rounded where the reference's torch code rounds it:

  htl.py:36  mean_diff = (past[:-2] - past[2:]).mean(0)     the differences summed in order, then divided by their count
  htl.py:39  c = 1 - relu(mean_diff / init_diff)            relu keeps NaN
  htl.py:41  time_value = min((epoch - 5) / (T - 5), 1.0)   a Python float (double); torch.pow rounds it to the exponent's dtype
  htl.py:44-47  control = 1.0; control *= c[p] for p in predecessors; w = time_value ** (1 - control)
  htl.py:56  w / w.sum() * 6.0

In float64 the same formulae run on the float32 INPUTS widened to double, and time_value stays the double it is.

Two steps of the float32 restatement are NOT the reference's bits, and `F32_BOUND` is what they can cost: torch sums the 12 weights in its
own vectorised order (here: in index order; any two orders of 12 non-negative terms are within 2 x 11 x 2^-24 of each other, relative), and
its vectorised powf is within 1 ulp of the correctly rounded value this file takes (the double result rounded once; 2 x 2^-24 each way plus
the final division and product, 2^-23).  A weight is at most 6: F32_BOUND = 6 x (11 + 2 + 1) x 2^-23 = 1.0e-5, absolute.  Rows whose
weights are small-integer ratios (every call before epoch 6; 0 ** 0 = 1) involve no rounding before the last division and are bit-exact.

The sequences (`SEQUENCES`: name -> (epochs, losses (len(epochs), 12) float32)); each runs through one fresh weightor, call by call:
  decay      losses that fall at a shrinking rate, epochs 0..8, then 150 and 250 (time_value below and clamped at 1)
  rising     the box items fall, then rise again: mean_diff / init_diff < 0, the relu clips it to 0, c = 1 and the exponent is 0
  restart_inf  epochs 0..5 and then 5 AGAIN (a run whose epoch counter repeats, as after a manual restart), 6..8 and 200.  Both
             predecessors of depth (box, 3D size) of the one-to-many set drop sharply between calls 4 and 5: at the repeated epoch 5 their
             ratios to the first mean difference are above 2, both c below -1, their product above 1, depth's exponent negative, and
             time_value is 0: 0 ** negative = inf, the sum is inf, depth's weight inf / inf = NaN and every other weight 0.  At epochs 6..8
             the negative exponent on a small time_value gives depth nearly all of the 6.
  restart_one  the same epochs; box of the one-to-one set jumps up at call 5 and keeps rising: c = 1, exponent 0 for the three items that
             hang on box alone, and at the repeated epoch 5 their weight is 0 ** 0 = 1 (6 / 7 after the normalisation).
  constant   a box item that stays constant: init_diff = 0, 0 / 0 = NaN at epoch 5, where the reference raises (a KeyError inside its
             diagnostic print, htl.py:48-51).  Recorded for epochs 0..4 (`RECORDED`); the restatement runs the sixth call too and shows the NaN.
"""
import os

import numpy as np

NAMES = ("box_om", "cls_om", "dep_om", "o3d_om", "s3d_om", "hd_om", "box_oo", "cls_oo", "dep_oo", "o3d_oo", "s3d_oo", "hd_oo")
PRE = ((), (), (0, 4), (0,), (0,), (0,), (), (), (6, 10), (6,), (6,), (6,))  # utils/htl.py:8-21
STAT_EPOCHS, MAX_EPOCHS = 5, 200
F32_BOUND = 6 * (11 + 2 + 1) * 2.0 ** -23  # see the module docstring
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "htl.npz")


def time_value(epoch, max_epochs=MAX_EPOCHS):
    return min((epoch - 5) / (max_epochs - 5), 1.0)


class Weightor:
    def __init__(self, dtype=np.float32, stat_epochs=STAT_EPOCHS, max_epochs=MAX_EPOCHS):
        self.dt, self.S, self.T = np.dtype(dtype).type, stat_epochs, max_epochs
        self.past, self.init_diff = [], None
        self.last = {}  # the intermediate values of the last call that had a full list: ratio, c, exponent (for the edge checks)

    def compute_weight(self, current_loss, epoch):
        dt = self.dt
        cur = np.asarray(current_loss, np.float32).astype(dt)
        w = np.array([0.0 if p else 1.0 for p in PRE], dt)
        with np.errstate(all="ignore"):
            if len(self.past) == self.S:
                past = np.stack(self.past)
                diff = past[:-2] - past[2:]
                s = np.zeros(12, dt)
                for d in diff:
                    s = (s + d).astype(dt)
                mean_diff = (s / dt(len(diff))).astype(dt)
                if self.init_diff is None:
                    self.init_diff = mean_diff
                ratio = (mean_diff / self.init_diff).astype(dt)
                relu = np.where(ratio > 0, ratio, np.where(np.isnan(ratio), ratio, dt(0))).astype(dt)
                c = (dt(1) - relu).astype(dt)
                tv = dt(time_value(epoch, self.T))
                expo = np.zeros(12, dt)
                for i, pre in enumerate(PRE):
                    if pre:
                        control = dt(1.0)
                        for p in pre:
                            control = dt(control * c[p])
                        expo[i] = dt(dt(1) - control)
                        w[i] = dt(np.power(np.float64(tv), np.float64(expo[i])))  # the double result rounded once: see POW_ULP
                self.last = {"ratio": ratio, "c": c, "expo": expo, "tv": tv}
                self.past.pop(0)
            self.past.append(cur)
            total = dt(0)
            for v in w:
                total = dt(total + v)
            return ((w / total).astype(dt) * dt(6.0)).astype(dt)


def run(epochs, losses, dtype=np.float32):
    """one fresh weightor over a sequence -> (weights (n, 12) of `dtype`, [the intermediate values per call])"""
    wt = Weightor(dtype)
    out, mids = [], []
    for e, l in zip(epochs, losses):
        wt.last = {}
        out.append(wt.compute_weight(l, int(e)))
        mids.append(wt.last)
    return np.stack(out), mids


def _seq_decay():
    epochs = list(range(9)) + [150, 250]
    base = np.array([2.0, 3.0, 4.0, 1.5, 1.2, 2.5, 2.2, 3.1, 4.4, 1.4, 1.1, 2.7])
    k = np.arange(len(epochs))[:, None]
    rate = np.array([0.30, 0.10, 0.05, 0.12, 0.22, 0.08, 0.26, 0.11, 0.04, 0.13, 0.2, 0.07])
    return epochs, (base * (0.35 + 0.65 * np.exp(-rate * k * (1 + 0.07 * k)))).astype(np.float32)


def _seq_rising():
    epochs = list(range(9)) + [200]
    k = np.arange(len(epochs))[:, None]
    base = np.array([2.0, 3.0, 4.0, 1.5, 1.2, 2.5, 2.2, 3.1, 4.4, 1.4, 1.1, 2.7])
    los = base * np.exp(-0.1 * k)
    los[:, 0] = 2.0 - 0.2 * k[:, 0] + 0.045 * k[:, 0] ** 2   # falls to k = 2.2, then rises past its start
    los[:, 6] = 2.2 - 0.25 * k[:, 0] + 0.05 * k[:, 0] ** 2
    return epochs, los.astype(np.float32)


RESTART_EPOCHS = [0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 200]
BASE = np.array([2.0, 3.0, 4.0, 1.5, 1.2, 2.5, 2.2, 3.1, 4.4, 1.4, 1.1, 2.7])


def _drop(start, slope, drop, k):
    """falls by `slope` per call, and by `drop` between calls 4 and 5"""
    return start - slope * k - (drop - slope) * (k >= 5)


def _seq_restart_inf():
    k = np.arange(len(RESTART_EPOCHS))
    los = BASE * np.exp(-0.05 * k[:, None])
    # box_om and s3d_om drop between calls 4 and 5: at call 6 their mean differences are 2.5 and 3.3 times the first ones, both c below -1,
    # their product above 1: depth's exponent is negative, the exponent of the items that hang on box alone is above 1
    los[:, 0] = _drop(5.0, 0.05, 0.5, k)
    los[:, 4] = _drop(4.0, 0.04, 0.6, k)
    return RESTART_EPOCHS, los.astype(np.float32)


def _seq_restart_one():
    k = np.arange(len(RESTART_EPOCHS))
    los = BASE * np.exp(-0.05 * k[:, None])
    # box_oo falls over the first five calls, jumps up by 1.5 and rises from then on: clipped ratio, c = 1, exponent 0
    los[:, 6] = 2.2 - 0.2 * np.minimum(k, 4) + 1.5 * (k >= 5) + 0.5 * np.maximum(k - 5, 0)
    return RESTART_EPOCHS, los.astype(np.float32)


def _seq_constant():
    epochs = list(range(6))
    k = np.arange(len(epochs))[:, None]
    base = np.array([2.0, 3.0, 4.0, 1.5, 1.2, 2.5, 2.2, 3.1, 4.4, 1.4, 1.1, 2.7])
    los = base * np.exp(-0.1 * k)
    los[:, 0] = 1.25  # box_om never moves: init_diff[0] = 0
    return epochs, los.astype(np.float32)


SEQUENCES = {"decay": _seq_decay(), "rising": _seq_rising(), "restart_inf": _seq_restart_inf(), "restart_one": _seq_restart_one(),
             "constant": _seq_constant()}
RECORDED = {"decay": 11, "rising": 10, "restart_inf": 11, "restart_one": 11, "constant": 5}  # calls the fixture holds: `constant` stops before the reference raises


def d_ref(golden):
    """the largest distance between the fixture (the reference in float32) and the float64 restatement over the entries finite in both; the
    non-finite entries must be the same ones"""
    worst = 0.0
    for name, (epochs, losses) in SEQUENCES.items():
        n = RECORDED[name]
        w64, _ = run(epochs[:n], losses[:n], np.float64)
        gw = golden[name]["weights"].astype(np.float64)
        both = np.isfinite(gw) & np.isfinite(w64)
        assert np.array_equal(np.isnan(gw), np.isnan(w64)) and np.array_equal(np.isinf(gw), np.isinf(w64)), name
        worst = max(worst, float(np.abs(gw - w64)[both].max()))
    return worst


def exact_rows(name):
    """calls whose weights are ratios of small integers: every call before epoch 6, and the repeated epoch 5 of `restart_one` (0 ** 0 = 1)"""
    return [i for i in range(RECORDED[name]) if i < 6 or (name == "restart_one" and i == 6)]


def load_golden():
    """-> {name: dict(epochs, losses, weights)}: the reference's own outputs (tools/make_golden_htl.py)"""
    z = np.load(GOLDEN)
    return {n: {k: z[f"{n}/{k}"] for k in ("epochs", "losses", "weights")} for n in SEQUENCES}
