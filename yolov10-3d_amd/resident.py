"""What the splits held on the device share (`kitti.DeviceSplit`, `yolo2d.DeviceSplit`, `yolo2d.DeviceRectSplit`, `json3d.DeviceSplit`),
and nothing that knows a dataset: the index lists of an epoch, the layout of the frame arena and its byte budget, the span table of
the label rows, the decode of every frame into the arena, the ring of pinned draw tables, the checks of a plan kernel's tables, and
`ResidentSplit`, the base class that holds the arena with its frame tables.  A split may keep the frames that its device budget cannot
hold in a second tier, one pinned host arena (`tier_layout`, `fill_pinned`, `load_pinned`, `stage_layout`, `stage_frames`, `ResidentSplit._layout_tiers`
/ `_fill_tiers` / `_stage`); `json3d.DeviceSplit` is the one that does.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import Y3DError

ALIGN = 16  # every frame starts on a multiple of 16 bytes of the arena (the image kernels read their sources byte by byte)


def upload(a, device, dtype=None):
    """a host array -> a contiguous tensor on `device` (one copy)"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def epoch_indices(n, batch, shuffle=True, seed=0, drop_last=False):
    """The batches of one epoch over n dataset positions: a list of index lists that covers every position once (drop_last: without the
    short last batch).  shuffle: a permutation from a generator of its own seeded with `seed`, so np.random's global state — the stream
    `sample_augment` replays — is not touched."""
    n, batch = int(n), int(batch)
    if batch < 1 or n < 0:
        raise Y3DError(f"epoch_indices: batch = {batch}, n = {n}")
    order = np.random.RandomState(int(seed)).permutation(n) if shuffle else np.arange(n)
    out = [[int(i) for i in order[s:s + batch]] for s in range(0, n, batch)]
    if drop_last and out and len(out[-1]) < batch:
        out.pop()
    return out


def arena_layout(hw, max_bytes, device, who):
    """Per-frame (h, w) sizes -> (offsets (N) int64, padded (N) int64, nbytes) of an arena of (h, w, 3) uint8 frames that each start on a
    multiple of 16 bytes.  Raises when the arena needs more than `max_bytes` (None: half of the free memory of `device`); nothing has
    been decoded or allocated by then.  who: the class name the refusal starts with."""
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    padded = (hw[:, 0] * hw[:, 1] * 3 + ALIGN - 1) // ALIGN * ALIGN
    offsets = np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64)
    nbytes = int(padded.sum())
    allowed = int(max_bytes) if max_bytes is not None else torch.cuda.mem_get_info(device)[0] // 2
    if nbytes > allowed:
        raise Y3DError(f"{who}: the {len(hw)} decoded frames need {nbytes} bytes, {allowed} bytes are allowed (max_bytes)")
    return offsets, padded, nbytes


def tier_layout(hw, max_bytes, host_bytes, device, who):
    """`arena_layout` over two tiers.  Frames in dataset order go into the device arena while their padded bytes fit `max_bytes` (None:
    half of the free memory of `device`); every frame from the first one that does not fit goes into one pinned host arena, a smaller
    later one too, so the tiers meet at a single boundary.  -> (n_dev, offsets (N) int64, padded (N) int64, nbytes, host_offsets (N)
    int64, host_nbytes): positions [0, n_dev) lie at `offsets` in the device arena of `nbytes` bytes, positions [n_dev, N) at
    `host_offsets` in the host arena of `host_nbytes` bytes; the other tier's entry is -1; every offset is a multiple of 16.  Raises
    when the host tier needs more than `host_bytes` (with host_bytes = 0: `arena_layout`'s refusal, and its layout when all fits);
    nothing has been decoded or allocated by then."""
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    N = len(hw)
    padded = (hw[:, 0] * hw[:, 1] * 3 + ALIGN - 1) // ALIGN * ALIGN
    ends = np.cumsum(padded)
    allowed = int(max_bytes) if max_bytes is not None else torch.cuda.mem_get_info(device)[0] // 2
    host_bytes = int(host_bytes)
    n_dev = int(np.searchsorted(ends, allowed, side="right"))  # the first frame whose end lies behind the budget
    if n_dev < N and host_bytes == 0:
        raise Y3DError(f"{who}: the {N} decoded frames need {int(ends[-1])} bytes, {allowed} bytes are allowed (max_bytes)")
    nbytes = int(ends[n_dev - 1]) if n_dev else 0
    host_nbytes = int(ends[-1]) - nbytes if N else 0
    if host_nbytes > host_bytes:
        raise Y3DError(f"{who}: the {N - n_dev} decoded frames behind the {n_dev} that fit the device ({allowed} bytes, max_bytes) need "
                       f"{host_nbytes} bytes of pinned host memory, {host_bytes} bytes are allowed (host_bytes)")
    starts = np.concatenate(([0], ends[:-1])).astype(np.int64)
    host = np.arange(N) >= n_dev
    return n_dev, np.where(host, -1, starts), padded, nbytes, np.where(host, starts - nbytes, -1), host_nbytes


def stage_layout(positions, n_dev, padded):
    """The staging buffer of one batch: the distinct host-tier positions (>= n_dev) among `positions` (primaries and partners; negative:
    none) in the order of their first use, each once, at padded offsets.  -> ({position: byte offset}, nbytes)"""
    at, nbytes = {}, 0
    for p in positions:
        p = int(p)
        if p >= n_dev and p not in at:
            at[p] = nbytes
            nbytes += int(padded[p])
    return at, nbytes


def fill_pinned(arena, offsets, positions, decode, pool):
    """Fills a pinned uint8 host arena: the threads of `pool` decode the frames at `positions` (`decode(pos)` -> (H, W, 3) uint8, as
    `fill_arena` takes it) and write each straight to byte offsets[pos] of the arena, with no pageable copy in between."""
    flat = arena.numpy()

    def put(pos):
        px = decode(pos)
        o = int(offsets[pos])
        flat[o:o + px.size] = px.reshape(-1)

    list(pool.map(put, positions))


def stage_frames(arena, offsets, nbytes_of, at, nbytes, device):
    """`stage_layout`'s frames from the pinned host arena into a device buffer of the batch's own, one non-blocking copy per frame on
    the current stream.  The buffer comes from the caching allocator, so whoever gets its memory next is ordered behind the kernels
    that read it by the stream alone.  -> the buffer (nbytes) uint8, or None when the batch uses no host-tier frame"""
    if not at:
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    for pos, o in at.items():
        n, h = int(nbytes_of[pos]), int(offsets[pos])
        buf[o:o + n].copy_(arena[h:h + n], non_blocking=True)
    return buf


def span_table(rows):
    """Label rows per frame -> (N, 2) int32 (first row, rows) of the frames' rows laid end to end"""
    span = np.zeros((len(rows), 2), np.int32)
    span[:, 1] = rows
    span[1:, 0] = np.cumsum(rows)[:-1]
    return span


def fill_arena(arena, offsets, padded, decode, pool, chunk):
    """Fills a uint8 device arena with decoded frames.  `decode(pos)` -> frame pos as an (H, W, 3) uint8 array (it raises for a frame it
    does not accept); the frame lands at byte offsets[pos], where padded[pos] bytes are its own.  Runs of consecutive frames of at most
    `chunk` bytes are decoded by the threads of `pool` into a pinned stage and reach the arena in one copy per run."""
    N = len(offsets)
    runs, first = [], 0
    for pos in range(1, N + 1):
        if pos == N or offsets[pos] + padded[pos] - offsets[first] > chunk:
            runs.append((first, pos))
            first = pos
    stage = torch.zeros(max(int(offsets[b - 1] + padded[b - 1] - offsets[a]) for a, b in runs), dtype=torch.uint8).pin_memory()
    stage_np = stage.numpy()

    def put(pos, base):
        px = decode(pos)
        o = int(offsets[pos]) - base
        stage_np[o:o + px.size] = px.reshape(-1)

    for a, b in runs:
        base, end = int(offsets[a]), int(offsets[b - 1] + padded[b - 1])
        list(pool.map(lambda pos: put(pos, base), range(a, b)))
        arena[base:end].copy_(stage[:end - base])  # from pinned memory; returns when the stage may be refilled


def load_arena(arena, offsets, padded, hw, decode, name, workers, chunk):
    """`fill_arena` through a pool of `min(workers, 16)` threads of its own, refusing a frame that does not decode to the (h, w, 3) its
    header gave.  name(pos): how the refusal calls the frame, its class-name prefix included."""
    from concurrent.futures import ThreadPoolExecutor

    def checked(pos):
        px = decode(pos)
        h, w = int(hw[pos][0]), int(hw[pos][1])
        if px.shape != (h, w, 3):
            raise Y3DError(f"{name(pos)} decodes to {px.shape}, its header said {(h, w, 3)}")
        return px

    with ThreadPoolExecutor(max_workers=min(int(workers), 16)) as pool:
        fill_arena(arena, offsets, padded, checked, pool, chunk)


def load_pinned(arena, offsets, positions, hw, decode, name, workers):
    """`fill_pinned` through a pool of `min(workers, 16)` threads of its own, with `load_arena`'s refusal of a frame that does not decode
    to the (h, w, 3) its header gave."""
    from concurrent.futures import ThreadPoolExecutor

    def checked(pos):
        px = decode(pos)
        h, w = int(hw[pos][0]), int(hw[pos][1])
        if px.shape != (h, w, 3):
            raise Y3DError(f"{name(pos)} decodes to {px.shape}, its header said {(h, w, 3)}")
        return px

    with ThreadPoolExecutor(max_workers=min(int(workers), 16)) as pool:
        fill_pinned(arena, offsets, positions, checked, pool)


class DrawRing:
    """`n` pinned (rows, width) float64 draw tables in flight to `device`: `upload(rows)` writes a table into the next buffer and starts
    a non-blocking copy -> (host view, device tensor).  A buffer is rewritten only after the copy that last read it has run (one event
    per buffer)."""

    def __init__(self, width, device, n):
        self.width, self.device, self.n, self._r = int(width), device, int(n), None

    def upload(self, rows):
        B = len(rows)
        if self._r is None or self._r["host"][0].shape[0] < B:
            cap = max(64, B)
            self._r = {"host": [torch.empty(cap, self.width, dtype=torch.float64).pin_memory() for _ in range(self.n)],
                       "event": [torch.cuda.Event() for _ in range(self.n)], "next": 0}
        r = self._r
        k = r["next"]
        r["next"] = (k + 1) % self.n
        r["event"][k].synchronize()  # (returns at once for an event never recorded)
        host = r["host"][k][:B]
        host.numpy()[:] = rows
        dev = torch.empty(B, self.width, dtype=torch.float64, device=self.device)
        dev.copy_(host, non_blocking=True)
        r["event"][k].record()
        return host, dev


def check_plan(draws, width, device, tables, draws_dev, out):
    """What every `plan_batch` checks before its launch.  draws: the contiguous (B, width) float64 draw table on the host (numpy or
    tensor); draws_dev: its copy on `device`, the split's (uploaded here when None); out: the output tensors named by `tables`, rows of
    (name, dtype, row shape), each with at least B rows (allocated here when None).  -> (host, draws_dev, out)"""
    host = torch.as_tensor(draws)
    if host.dim() != 2 or host.shape[1] != width or host.dtype != torch.float64 or host.is_cuda or not host.is_contiguous():
        raise Y3DError(f"plan_batch: the draws are a contiguous (B, {width}) float64 table on the host, got {tuple(host.shape)} {host.dtype}")
    B = host.shape[0]
    if draws_dev is None:
        draws_dev = host.to(device)
    if draws_dev.shape != host.shape or draws_dev.dtype != torch.float64 or draws_dev.device != device or not draws_dev.is_contiguous():
        raise Y3DError("plan_batch: the device copy of the draws must match the host table and live on the split's device")
    if out is None:
        out = {k: torch.empty(B, *s, dtype=dt, device=device) for k, dt, s in tables}
    for k, dt, s in tables:
        t = out[k]
        if t.dtype != dt or t.device != device or t.dim() != 1 + len(s) or t.shape[0] < B or tuple(t.shape[1:]) != s or not t.is_contiguous():
            raise Y3DError(f"plan_batch: output {k} must be a contiguous ({B}+, {', '.join(map(str, s))}) {dt} tensor on {device}")
    return host, draws_dev, out


class ResidentSplit:
    """The frames of a split decoded once into one uint8 device arena, and the frame tables indexed by dataset position: `device`;
    `offsets` (N) int64 on the host and `nbytes`; `arena`; `img_off` (N) int64; `frame_hw` (N, 2) int32 (h, w); `rec_span` (N, 2) int32
    (first label row, rows).  A subclass supplies `__len__`, `build_batch` and its label rows; it calls `_layout` once the frame sizes
    are known from the file headers and `_fill` once it has read the labels."""

    RING = 4  # pinned draw tables in flight
    CHUNK = 256 << 20  # bytes of decoded frames per upload

    def _accept(self, device, mode, workers, host_bytes=None):
        """The checks a labelled split's constructor makes before it reads anything (host_bytes: only for a split with a host tier);
        sets `mode`.  -> the device with its index"""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise Y3DError(f"DeviceSplit: the split is held on a HIP device, not {dev} (no host fallback)")
        if mode == "test":
            raise Y3DError("DeviceSplit: the test split has no labels")
        if int(workers) < 1 or (host_bytes is not None and int(host_bytes) < 0):
            raise Y3DError(f"DeviceSplit: workers = {workers}" + ("" if host_bytes is None else f", host_bytes = {host_bytes}"))
        self.mode = mode
        return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _sizes(self, files):
        """The split's image files -> `wh`, every frame's (W, H) from the file headers alone; refuses a split without frames.
        -> (h, w) per frame, what `_layout` takes"""
        from PIL import Image
        if len(files) < 1:
            raise Y3DError("DeviceSplit: the split lists no frame")
        self.wh = []
        for f in files:
            with Image.open(f) as im:
                self.wh.append((int(im.size[0]), int(im.size[1])))
        return [(h, w) for w, h in self.wh]

    def _layout(self, device, hw, max_bytes):
        """(h, w) per frame -> `offsets`, `nbytes`: the budget before anything is decoded or allocated, then `device` with its index"""
        self._hw = np.asarray(hw, np.int64).reshape(-1, 2)
        self.offsets, self._padded, self.nbytes = arena_layout(self._hw, max_bytes, device, type(self).__name__)
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _fill(self, span, decode, name, workers, draw_w):
        """Uploads the frame tables, then allocates the arena and decodes every frame into it (`load_arena`: runs of consecutive frames
        into a pinned stage, one copy per run).  span: `span_table` of the label rows; draw_w: the width of the split's draw table."""
        dev = self.device
        self.rec_span, self.img_off = upload(span, dev, torch.int32), upload(self.offsets, dev, torch.int64)
        self.frame_hw = upload(self._hw, dev, torch.int32)
        self.arena = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        load_arena(self.arena, self.offsets, self._padded, self._hw, decode, lambda pos: f"{type(self).__name__}: {name(pos)}", workers,
                   self.CHUNK)
        self._ring = DrawRing(draw_w, dev, self.RING)

    n_dev = host_arena = None  # one tier unless a subclass lays out two (`_layout_tiers`): every frame in the device arena

    def _layout_tiers(self, device, hw, max_bytes, host_bytes):
        """`_layout` over two tiers (`tier_layout`): also `n_dev`, `host_offsets`, `host_nbytes`.  `offsets` holds -1 behind n_dev."""
        self._hw = np.asarray(hw, np.int64).reshape(-1, 2)
        self.n_dev, self.offsets, self._padded, self.nbytes, self.host_offsets, self.host_nbytes = tier_layout(
            self._hw, max_bytes, host_bytes, device, type(self).__name__)
        self._frame_bytes = self._hw[:, 0] * self._hw[:, 1] * 3
        self.device = device if device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _fill_tiers(self, span, decode, name, workers, draw_w):
        """`_fill` over two tiers: the first `n_dev` frames reach the device arena as there, the rest are decoded by the same number of
        threads straight into `host_arena`, which is allocated pinned."""
        dev, n = self.device, self.n_dev
        self.rec_span, self.img_off = upload(span, dev, torch.int32), upload(self.offsets, dev, torch.int64)
        self.frame_hw = upload(self._hw, dev, torch.int32)
        self.arena = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        named = lambda pos: f"{type(self).__name__}: {name(pos)}"
        if n:
            load_arena(self.arena, self.offsets[:n], self._padded[:n], self._hw, decode, named, workers, self.CHUNK)
        self.host_arena = torch.empty(self.host_nbytes, dtype=torch.uint8, pin_memory=self.host_nbytes > 0)
        if n < len(self._hw):
            load_pinned(self.host_arena, self.host_offsets, range(n, len(self._hw)), self._hw, decode, named, workers)
        self._ring = DrawRing(draw_w, dev, self.RING)

    def _stage(self, positions):
        """the distinct host-tier frames among `positions` staged on the device -> ({position: byte offset}, buffer or None)"""
        at, nbytes = stage_layout(positions, self.n_dev, self._padded)
        return at, stage_frames(self.host_arena, self.host_offsets, self._frame_bytes, at, nbytes, self.device)

    def check_device(self, device):
        d = torch.device(device)
        if d.type != "cuda" or (d.index is not None and d.index != self.device.index):
            raise Y3DError(f"build_batch: the split lives on {self.device}, a batch on {d} was asked for")

    def frame(self, pos):
        """the decoded frame at a dataset position: an (h, w, 3) uint8 view of the arena (of the pinned host arena for a position of the
        host tier)"""
        h, w = int(self._hw[pos][0]), int(self._hw[pos][1])
        if self.n_dev is not None and pos >= self.n_dev:
            o = int(self.host_offsets[pos])
            return self.host_arena[o:o + h * w * 3].view(h, w, 3)
        o = int(self.offsets[pos])
        return self.arena[o:o + h * w * 3].view(h, w, 3)

    def epoch(self, batch, args, mode="train", shuffle=True, seed=0, drop_last=False, **kw):
        """One epoch of batches: `build_batch` over `epoch_indices(len(self), batch, shuffle, seed, drop_last)`.  A build only enqueues
        work on the current stream, so building the next batch already overlaps the step that consumes this one."""
        for idx in epoch_indices(len(self), batch, shuffle, seed, drop_last):
            yield self.build_batch(idx, args, mode=mode, **kw)
