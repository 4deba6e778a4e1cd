"""Host references for the eval head tail (csrc/post.hip) and the NHWC glue kernels (csrc/misc.hip), written from the reference
project's semantics as explicit index arithmetic in numpy / torch-CPU; nothing here calls the code under test.

Selections and copies return tensors of the input's storage type (compared bit for bit with `bits`); arithmetic references return
float64.  tests/test_tail_ref_host.py pins every function against an independent statement (oracle/restate.py, torch.nn.functional)."""
import numpy as np
import torch

SENT_I = -7                      # sentinel of integer outputs
_SENT_BITS = {torch.float32: 0x7FC1BEEF, torch.bfloat16: 0x7FC1, torch.uint8: 0xA5, torch.int32: SENT_I, torch.int64: SENT_I}
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.int32: torch.int32,
             torch.int64: torch.int64}


def bits(t):
    """the tensor's storage as integers (bit equality; NaN payloads and the sign of zero count)"""
    return t.contiguous().view(_INT_VIEW[t.dtype])


def sentinel(shape, dtype, device="cpu"):
    """a buffer no kernel produces: a NaN with a payload for floats, -7 for ints, 0xA5 for bytes"""
    shape = shape if isinstance(shape, (tuple, list)) else (shape,)
    return torch.full(shape, _SENT_BITS[dtype], dtype=_INT_VIEW[dtype], device=device).view(dtype)


def untouched(t):
    """True where `t` still holds the sentinel"""
    return bits(t) == bits(sentinel((1,), t.dtype, t.device))


def rnd(t, dtype):
    """an exact float64 value rounded ONCE to the storage type, as float64"""
    return t.to(dtype).double()


# ---------------------------------------------------------------------------------------------------------------- eval head tail
def patch_gather(x, idx, ps):
    """x (B, H, W, C) storage type, idx (B, K) cells (row * W + col) -> (B * K, ps, ps, C): out[b*K+j][py][px] =
    x[b][row - ps//2 + py][col - ps//2 + px], zero outside the map (head.py:663-684 extract_patches)"""
    B, H, W, C = x.shape
    K = idx.shape[1]
    pad = ps // 2
    out = torch.zeros(B * K, ps, ps, C, dtype=x.dtype)
    for b in range(B):
        for j in range(K):
            row, col = divmod(int(idx[b, j]), W)
            for py in range(ps):
                hh = row - pad + py
                if hh < 0 or hh >= H:
                    continue
                lo, hi = max(0, pad - col), min(ps, W + pad - col)  # px with 0 <= col - pad + px < W
                if lo < hi:
                    out[b * K + j, py, lo:hi] = x[b, hh, col - pad + lo:col - pad + hi]
    return out


def head3d_scatter(cls, reg, idx, nc, no):
    """cls (B, HW, nc), reg (B * K, no - nc), idx (B, K) unique cells -> map (B, HW, no): cls | reg of the candidate on the cell,
    +0 elsewhere (head.py:709-713)"""
    B, HW, _ = cls.shape
    K = idx.shape[1]
    m = torch.zeros(B, HW, no, dtype=cls.dtype)
    m[:, :, :nc] = cls
    for b in range(B):
        m[b, idx[b].long(), nc:] = reg[b * K:(b + 1) * K]
    return m


def anchors(shapes):
    """per anchor of the concatenated levels: level, row, column (utils/tal.py:300-312 make_anchors order: level, row, column)"""
    lv, hy, hx = [], [], []
    for l, (H, W) in enumerate(shapes):
        r = np.arange(H * W)
        lv.append(np.full(H * W, l))
        hy.append(r // W)
        hx.append(r % W)
    return np.concatenate(lv), np.concatenate(hy), np.concatenate(hx)


def _flat_levels(maps):
    """[(B, H, W, no)] storage type -> (B, A, no) float64 of the stored values, anchors in make_anchors order"""
    B, no = maps[0].shape[0], maps[0].shape[3]
    return torch.cat([m.double().reshape(B, -1, no) for m in maps], 1)


def head3d_decode(maps, strides, nc):
    """maps [(B, H, W, nc + 35)] -> y (B, nc + 35, A) float64 (head.py:755-797): cls | xyxy px | centre-3d px | the rest copied.
    Also returns `mag` (B, 6, A): the magnitudes the fp32 rounding bound of the six computed channels is built from, per channel
    2 |c| + |s / 2| + |ref| for the box corners (c = (o + anchor) * stride, s = size * stride) and 2 |c| for the centre"""
    v = _flat_levels(maps)
    lv, hy, hx = anchors([m.shape[1:3] for m in maps])
    st = torch.tensor([float(strides[l]) for l in lv], dtype=torch.float64)
    ax, ay = torch.from_numpy(hx + 0.5), torch.from_numpy(hy + 0.5)
    y = v.clone()
    cx, cy = (v[..., nc] + ax) * st, (v[..., nc + 1] + ay) * st
    sx, sy = v[..., nc + 2] * st, v[..., nc + 3] * st
    y[..., nc + 0], y[..., nc + 1], y[..., nc + 2], y[..., nc + 3] = cx - sx / 2, cy - sy / 2, cx + sx / 2, cy + sy / 2
    y[..., nc + 4], y[..., nc + 5] = (v[..., nc + 4] + ax) * st, (v[..., nc + 5] + ay) * st
    mag = torch.stack([2 * cx.abs() + sx.abs() / 2 + y[..., nc + 0].abs(), 2 * cy.abs() + sy.abs() / 2 + y[..., nc + 1].abs(),
                       2 * cx.abs() + sx.abs() / 2 + y[..., nc + 2].abs(), 2 * cy.abs() + sy.abs() / 2 + y[..., nc + 3].abs(),
                       2 * y[..., nc + 4].abs(), 2 * y[..., nc + 5].abs()], 1)
    return y.permute(0, 2, 1).contiguous(), mag


def head2d_decode(maps, strides, nc):
    """maps [(B, H, W, 64 + nc)] with channels [4 x 16 DFL bins | nc logits] -> y (B, 4 + nc, A) float64 (head.py:53-79): softmax
    expectation of each box side, (l, t, r, b) distances -> xywh px, sigmoid scores"""
    v = _flat_levels(maps)
    B, A, _ = v.shape
    lv, hy, hx = anchors([m.shape[1:3] for m in maps])
    st = torch.tensor([float(strides[l]) for l in lv], dtype=torch.float64)
    ax, ay = torch.from_numpy(hx + 0.5), torch.from_numpy(hy + 0.5)
    bins = v[..., :64].reshape(B, A, 4, 16)
    e = torch.exp(bins - bins.max(-1, keepdim=True)[0])
    d = (e * torch.arange(16, dtype=torch.float64)).sum(-1) / e.sum(-1)
    x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
    y = torch.empty(B, A, 4 + nc, dtype=torch.float64)
    y[..., 0], y[..., 1], y[..., 2], y[..., 3] = (x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st
    y[..., 4:] = 1.0 / (1.0 + torch.exp(-v[..., 64:]))
    return y.permute(0, 2, 1).contiguous()


def _top_desc(v, K):
    """indices of the K largest of a 1-D array by (value desc, index asc); -0 counts as +0"""
    v = np.asarray(v, dtype=np.float64) + 0.0
    return np.lexsort((np.arange(v.size), -v))[:K]


def v10_postprocess(y, nc, K, boxes_first):
    """y (B, C, A) fp32 -> reg (B, K, C - nc) fp32, scores (B, K) fp32, labels (B, K) int64 (utils/ops.py:852-880): the K anchors
    with the best max-class score, then the K best of their K * nc scores (flat index j * nc + c); both by (value desc, index asc)"""
    y = y.numpy()
    B, C, A = y.shape
    s0, r0, nr = (C - nc, 0, C - nc) if boxes_first else (0, nc, C - nc)
    reg = np.empty((B, K, nr), np.float32)
    scores = np.empty((B, K), np.float32)
    labels = np.empty((B, K), np.int64)
    for b in range(B):
        sc = y[b, s0:s0 + nc]                         # (nc, A)
        top = _top_desc(sc.max(0), K)                 # anchors
        flat = sc[:, top].T.reshape(-1)               # [j * nc + c]
        top2 = _top_desc(flat, K)
        scores[b] = flat[top2]
        labels[b] = top2 % nc
        reg[b] = y[b, r0:r0 + nr][:, top[top2 // nc]].T
    return torch.from_numpy(reg), torch.from_numpy(scores), torch.from_numpy(labels)


def postprocess_nseg(A, max_det):
    """the segment count of the hi-res path by the wrapper's documented rule: halve from 16 while 16 * max_det * 2 > A"""
    nseg = 16
    while nseg > 1 and nseg * max_det * 2 > A:
        nseg >>= 1
    return nseg


# ---------------------------------------------------------------------------------------------------------------- NHWC glue
def maxpool_fwd(x, k):
    """x (B, H, W, C) storage type -> y (same type), arg (B, H, W, C) uint8: k x k stride-1 pad-k//2 max pool, the window scanned
    row then column from its FIRST IN-MAP tap with a strict `>` (first max wins), a NaN always taken (the last NaN of the window
    wins); arg = tap index r * k + q (ATen max_pool2d: maxidx starts at the window's first in-map element)"""
    B, H, W, C = x.shape
    pad = k // 2
    xv = x.double().numpy()
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    best = np.full((B, H, W, C), -np.inf)
    bi = np.broadcast_to((np.maximum(0, pad - h) * k + np.maximum(0, pad - w))[None, :, :, None], (B, H, W, C)).copy()
    for r in range(k):          # all output pixels at once, tap by tap in scan order
        for q in range(k):
            hh, ww = h - pad + r, w - pad + q
            ok = ((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W))[None, :, :, None]
            v = xv[:, np.clip(hh, 0, H - 1), np.clip(ww, 0, W - 1)]  # (B, H, W, C)
            take = ok & ((v > best) | np.isnan(v))
            best = np.where(take, v, best)
            bi = np.where(take, r * k + q, bi)
    return torch.from_numpy(best).to(x.dtype), torch.from_numpy(bi.astype(np.uint8))


def maxpool_bwd(dy, arg, k):
    """dy (B, H, W, C) float64, arg from maxpool_fwd -> dx float64: every output pixel adds its gradient to the input pixel its
    arg-max tap names"""
    B, H, W, C = dy.shape
    pad = k // 2
    dx = np.zeros((B, H, W, C), np.float64)
    dyv, a = dy.numpy(), arg.numpy().astype(np.int64)
    bb, cc = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for h in range(H):
        for w in range(W):
            hh, ww = h - pad + a[:, h, w] // k, w - pad + a[:, h, w] % k
            assert (hh >= 0).all() and (hh < H).all() and (ww >= 0).all() and (ww < W).all()
            np.add.at(dx, (bb, hh, ww, cc), dyv[:, h, w])
    return torch.from_numpy(dx)


def upsample2x_fwd(x):
    """x (B, H, W, C) -> (B, 2H, 2W, C): y[h][w] = x[h // 2][w // 2]"""
    B, H, W, C = x.shape
    y = torch.empty(B, 2 * H, 2 * W, C, dtype=x.dtype)
    for h in range(2 * H):
        for w in range(2 * W):
            y[:, h, w] = x[:, h // 2, w // 2]
    return y


def upsample2x_bwd(dy):
    """dy (B, 2H, 2W, C) float64 -> dx (B, H, W, C) float64: the sum of the four output pixels of each input pixel"""
    return dy[:, 0::2, 0::2] + dy[:, 0::2, 1::2] + dy[:, 1::2, 0::2] + dy[:, 1::2, 1::2]


def nchw_to_nhwc(x, Cpad, dtype):
    """x (B, C, H, W) fp32 -> (B, H, W, Cpad) storage type, lanes C..Cpad exactly +0"""
    B, C, H, W = x.shape
    y = torch.zeros(B, H, W, Cpad, dtype=dtype)
    for c in range(C):
        y[..., c] = x[:, c].to(dtype)
    return y


def nhwc_to_nchw(x):
    """x (B, H, W, C) storage type -> (B, C, H, W) fp32 of the stored values"""
    B, H, W, C = x.shape
    y = torch.empty(B, C, H, W, dtype=torch.float32)
    for c in range(C):
        y[:, c] = x[..., c].float()
    return y
