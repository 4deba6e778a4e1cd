"""The device tables of the multi-tensor launches (csrc/optim.hip, y3d_mt_pack_weights): one home for the chunk map, the pinned pointer
upload and the table a launch reads - used by the optimizers, ModelEMA, GradAccumulator (optim.py), FlatGradReducer (ddp.py) and the
weight packs (ops.py).  Imports neither `ops` nor `optim`: both import this.  DESIGN.md §3.29.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

CHUNK = 16384  # elements per workgroup of every multi-tensor launch


def chunk_map(sizes, chunk=CHUNK):
    """Host only: the (chunk_tensor, chunk_off) tables of the multi-tensor launches: workgroup c handles elements
    [chunk_off[c] * chunk, + chunk) of tensor chunk_tensor[c]; a tensor of 0 elements gets no workgroup"""
    ct, co = [], []
    for t, n in enumerate(sizes):
        for c in range((int(n) + chunk - 1) // chunk):
            ct.append(t)
            co.append(c)
    return ct, co


class PtrUploader:
    """Pointer tables that change every step (the step's gradient tensors) go to the device through rotating PINNED host buffers
    with a non-blocking copy: `torch.tensor(list, device=...)` stages through pageable memory and holds the host until the stream
    has drained, which leaves the GPU idle while the rest of the optimizer's host code runs (measured ~1 ms per step)."""

    def __init__(self, n, device, depth=4):
        self.host = [torch.empty(n, dtype=torch.int64).pin_memory() for _ in range(depth)]
        self.np = [h.numpy() for h in self.host]
        self.dev = [torch.empty(n, dtype=torch.int64, device=device) for _ in range(depth)]
        self.i, self.n = 0, n

    def upload(self, ptrs):
        assert len(ptrs) == self.n
        k = self.i
        self.i = (self.i + 1) % len(self.host)
        self.np[k][:] = np.asarray(ptrs, dtype=np.int64)
        self.dev[k].copy_(self.host[k], non_blocking=True)
        return self.dev[k]


class PtrColumn:
    """One refreshable pointer column of a Table: `key` is the host list of addresses last uploaded, `dev` the device tensor that
    holds them, `uploads` how often that happened.  pinned: through a rotating PtrUploader of `depth` buffers, made on first use - or
    now, for `n` pointers: pinned memory cannot be allocated while a hipGraph is being captured; otherwise a plain `torch.tensor`
    upload (a new device tensor each time: for columns that almost never change)."""

    def __init__(self, device, pinned=True, depth=4, n=None):
        self.device, self.pinned, self.depth = device, pinned, depth
        self.key = self.dev = None
        self.up = None if n is None else PtrUploader(n, device, depth)
        self.uploads = 0

    def refresh(self, ptrs, force=False):
        """-> the device tensor holding `ptrs`; nothing is uploaded when they equal the key, unless `force` (a launch recorded into a
        hipGraph, or on a stream of its own, needs its copy whatever the host remembers)"""
        if force or ptrs != self.key:
            if self.pinned:
                if self.up is None or self.up.n != len(ptrs):
                    self.up = PtrUploader(len(ptrs), self.device, self.depth)
                self.dev = self.up.upload(ptrs)
            else:
                self.dev = torch.tensor(ptrs, dtype=torch.int64, device=self.device)
            self.key = ptrs
            self.uploads += 1
        return self.dev


class Table:
    """What a multi-tensor launch reads for ONE fixed list of tensors of `sizes` elements: the device tensors `sizes` (int64),
    `chunk_tensor` / `chunk_off` (int32, chunk_map) and `nchunks`; `ptr[name]`: pointer columns fixed for the table's life, given
    as keyword lists of addresses (state buffers, arena views, reducer slots); `col[name]`: PtrColumns added with column().
    `host_sizes` is the list the table was built from.  `chunks` = (chunk_tensor, chunk_off addresses, nchunks, chunk): the four
    arguments every y3d_mt_* entry point takes in that order."""

    def __init__(self, sizes, device, chunk=CHUNK, **fixed):
        self.host_sizes = [int(n) for n in sizes]
        self.device, self.chunk = device, chunk
        ct, co = chunk_map(self.host_sizes, chunk)
        self.nchunks = len(ct)
        self.sizes = torch.tensor(self.host_sizes, dtype=torch.int64, device=device)
        self.chunk_tensor = torch.tensor(ct, dtype=torch.int32, device=device)
        self.chunk_off = torch.tensor(co, dtype=torch.int32, device=device)
        self.chunks = (self.chunk_tensor.data_ptr(), self.chunk_off.data_ptr(), self.nchunks, chunk)
        self.ptr = {k: torch.tensor(v, dtype=torch.int64, device=device) for k, v in fixed.items()}
        self.col = {}

    def column(self, name, pinned=True, depth=4, now=False):
        """add (or replace) a refreshable column; now: with its uploader made here, not on first use"""
        self.col[name] = PtrColumn(self.device, pinned, depth, len(self.host_sizes) if now else None)
        return self.col[name]

    def held(self):
        """a copy for a captured hipGraph to keep alive: the same device tensors and uploaders as the table has NOW, whatever the
        owner's columns are refreshed to, or replaced by, afterwards"""
        t = copy.copy(self)
        t.col = {k: copy.copy(c) for k, c in self.col.items()}
        return t

    @staticmethod
    def fp32_contiguous(grads):
        """the gradients as the kernels read them: a tensor that is not contiguous fp32 is replaced by a converted copy"""
        return [g if g.dtype == torch.float32 and g.is_contiguous() else g.float().contiguous() for g in grads]
