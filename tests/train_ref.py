"""The reference's iteration bookkeeping restated as the loop it is (engine/trainer.py:331-332, 384-386, 411-413) and its EarlyStopping
(utils/torch_utils.py:553-595), for tests/test_train_host.py and tests/test_hip_train.py.  Nothing here imports the package."""
import math

import numpy as np


def do_train_rows(n, batch, epochs, nbs, warmup_epochs):
    """-> [(epoch, i, ni, accumulate, stepped)] in the order `_do_train` visits its batches; `len(train_loader)` is ceil(n / batch)"""
    accumulate = max(round(nbs / batch), 1)                                    # :307
    nb = math.ceil(n / batch)                                                  # :331
    nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1      # :332
    last_opt_step = -1
    rows = []
    epoch = 0
    while True:
        for i in range(nb):
            ni = i + nb * epoch
            if ni <= nw:                                                       # :384
                xi = [0, nw]
                accumulate = max(1, int(np.interp(ni, xi, [1, nbs / batch]).round()))  # :386
            stepped = False
            if ni - last_opt_step >= accumulate:                               # :411
                stepped = True
                last_opt_step = ni                                             # :413
            rows.append((epoch, i, ni, accumulate, stepped))
        epoch += 1
        if epoch == epochs:
            return rows


def windows(rows):
    """-> the micro-batch counts of the optimizer steps, and the (epoch, i) of micro-batches that no step consumed because the epoch
    ended first (the `zero_grad` at the next epoch's start drops them)"""
    sizes, dropped, open_ = [], [], []
    for k, (epoch, i, ni, acc, stepped) in enumerate(rows):
        if open_ and open_[0][0] != epoch:
            dropped += open_
            open_ = []
        open_.append((epoch, i))
        if stepped:
            sizes.append(len(open_))
            open_ = []
    return sizes, dropped + open_


class Stopper:
    def __init__(self, patience=50):
        self.best_fitness = 0.0
        self.best_epoch = 0
        self.patience = patience or float("inf")
        self.possible_stop = False

    def __call__(self, epoch, fitness):
        if fitness is None:
            return False
        if fitness >= self.best_fitness:
            self.best_epoch = epoch
            self.best_fitness = fitness
        delta = epoch - self.best_epoch
        self.possible_stop = delta >= (self.patience - 1)
        return delta >= self.patience


def best_fitness_rule(best, fitness):
    """engine/trainer.py:589-590"""
    if not best or best < fitness:
        best = fitness
    return best
