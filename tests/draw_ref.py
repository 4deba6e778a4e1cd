"""A plain NumPy float64 restatement of the drawing rules of include/y3d.h (csrc/draw3d.hip, plot.py), and the case lists the GPU tests
use.  NumPy multiplies and adds in separate roundings and in the order written, which is what the library's build (contraction off)
does, so the two agree bit for bit.

  segment a -> b, thickness t, r2 = (t/2)(t/2), pixel p:  d = b - a, e = p - a, len2 = d.x d.x + d.y d.y, dot = e.x d.x + e.y d.y
      dot <= 0: e.x e.x + e.y e.y <= r2;   dot >= len2: the same with p - b;   else c = d.x e.y - d.y e.x, c c <= r2 len2
  quad q0..q3:  E_i = d_i.x (p.y - q_i.y) - d_i.y (p.x - q_i.x), d_i = q_{i+1} - q_i; all four >= 0 or all four <= 0; skipped when
      (q1 - q0) x (q2 - q0) + (q2 - q0) x (q3 - q0) == 0
  a primitive with a non-finite coordinate is skipped; the lower index wins: painted in descending index order."""
import functools

import numpy as np

SEGMENT_ENDS = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7), (0, 5), (1, 4))
ERR = dict(all="ignore")


# ---------------------------------------------------------------------------------------------------------------- coverage
def _grid(H, W, window):
    y0, y1, x0, x1 = (0, H, 0, W) if window is None else window
    x, y = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64))
    return x, y


def segment_mask(H, W, seg, t, window=None):
    """bool (H, W) (or the window (y0, y1, x0, x1) of it): the pixels segment [ax, ay, bx, by] of thickness t covers"""
    x, y = _grid(H, W, window)
    ax, ay, bx, by = (np.float64(v) for v in seg)
    if not np.isfinite([ax, ay, bx, by]).all():
        return np.zeros(x.shape, bool)
    with np.errstate(**ERR):
        h = np.float64(t) / 2
        r2 = h * h
        dx, dy = bx - ax, by - ay
        ex, ey = x - ax, y - ay
        len2 = dx * dx + dy * dy
        dot = ex * dx + ey * dy
        gx, gy = x - bx, y - by
        c = dx * ey - dy * ex
        return np.where(dot <= 0, ex * ex + ey * ey <= r2, np.where(dot >= len2, gx * gx + gy * gy <= r2, c * c <= r2 * len2))


def quad_area2(quad):
    q = np.asarray(quad, np.float64).reshape(4, 2)
    with np.errstate(**ERR):
        u, v, w = q[1] - q[0], q[2] - q[0], q[3] - q[0]
        return (u[0] * v[1] - u[1] * v[0]) + (v[0] * w[1] - v[1] * w[0])


def quad_mask(H, W, quad, window=None):
    x, y = _grid(H, W, window)
    q = np.asarray(quad, np.float64).reshape(4, 2)
    if not np.isfinite(q).all() or quad_area2(q) == 0:
        return np.zeros(x.shape, bool)
    with np.errstate(**ERR):
        E = []
        for i in range(4):
            d = q[(i + 1) % 4] - q[i]
            E.append(d[0] * (y - q[i, 1]) - d[1] * (x - q[i, 0]))
        E = np.stack(E)
        return (E >= 0).all(0) | (E <= 0).all(0)


def _window(H, W, xs, ys, pad):
    """the pixels within `pad` of the bounding box of the points, cut to the canvas (a generous pad: not the kernel's margin)"""
    lo = lambda v, n: int(np.clip(np.floor(np.min(v)) - pad, 0, n))
    hi = lambda v, n: int(np.clip(np.ceil(np.max(v)) + pad + 1, 0, n))
    return lo(ys, H), hi(ys, H), lo(xs, W), hi(xs, W)


def paint_segments(canvas, segs, rgb, t, n=None, windowed=True):
    """canvas (H, W, 3) uint8 -> a painted copy: segments 0 .. n-1 in descending order, so the lowest index is on top"""
    out = canvas.copy()
    H, W = out.shape[:2]
    n = len(segs) if n is None else max(0, min(int(n), len(segs)))
    pad = int(np.ceil(t / 2)) + 3
    for k in range(n - 1, -1, -1):
        s = segs[k]
        if not np.isfinite(s).all():
            continue
        win = _window(H, W, s[[0, 2]], s[[1, 3]], pad) if windowed else (0, H, 0, W)
        if win[0] >= win[1] or win[2] >= win[3]:
            continue
        out[win[0]:win[1], win[2]:win[3]][segment_mask(H, W, s, t, win)] = rgb[k, :3]
    return out


def paint_quads(canvas, quads, rgb, n=None, windowed=True):
    out = canvas.copy()
    H, W = out.shape[:2]
    quads = np.asarray(quads, np.float64).reshape(-1, 4, 2)
    n = len(quads) if n is None else max(0, min(int(n), len(quads)))
    for k in range(n - 1, -1, -1):
        q = quads[k]
        if not np.isfinite(q).all():
            continue
        win = _window(H, W, q[:, 0], q[:, 1], 3) if windowed else (0, H, 0, W)
        if win[0] >= win[1] or win[2] >= win[3]:
            continue
        out[win[0]:win[1], win[2]:win[3]][quad_mask(H, W, q, win)] = rgb[k, :3]
    return out


def paint_batch(paint, canvases, prims, rgb, n=None, **kw):
    return np.stack([paint(canvases[b], prims[b], rgb[b], n=None if n is None else n[b], **kw) for b in range(len(canvases))])


# ---------------------------------------------------------------------------------------------------------------- preparation
def colours(cls, palette):
    """palette[clamp((int)cls, 0, n - 1)], NaN -> entry 0; -> (K, 4) uint8 [r, g, b, 0]"""
    pal = np.asarray(palette, np.uint8).reshape(-1, 3)
    c = np.asarray(cls, np.float64)
    idx = np.clip(np.trunc(np.where(np.isnan(c), 0.0, c)), 0, len(pal) - 1).astype(np.int64)
    return np.concatenate([pal[idx], np.zeros((len(idx), 1), np.uint8)], 1)


def box_segments(corners3d, rows, count, P2, affine, palette, near):
    """one image: corners3d (K, 8, 3), rows (K, 14) or None, P2 (12,), affine (6,) or None -> segs (K * 14, 4), rgb (K * 14, 4),
    `clipped` (K * 14, 2) bool: the endpoints that went through the clip's division"""
    c3 = np.asarray(corners3d, np.float64).reshape(-1, 8, 3)
    K = len(c3)
    P = np.asarray(P2, np.float64).reshape(12)
    near = np.float64(near)
    segs = np.full((K, 14, 4), np.nan)
    rgb = np.zeros((K, 14, 4), np.uint8)
    clipped = np.zeros((K, 14, 2), bool)
    n = max(0, min(int(count), K))
    with np.errstate(**ERR):
        x, y, z = c3[:n, :, 0], c3[:n, :, 1], c3[:n, :, 2]
        U = ((P[0] * x + P[1] * y) + P[2] * z) + P[3]
        V = ((P[4] * x + P[5] * y) + P[6] * z) + P[7]
        Wc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11]
        for j, (a, b) in enumerate(SEGMENT_ENDS):
            Ua, Va, Wa, Ub, Vb, Wb = U[:, a], V[:, a], Wc[:, a], U[:, b], V[:, b], Wc[:, b]
            la, lb = Wa < near, Wb < near
            sa = (near - Wa) / (Wb - Wa)
            sb = (near - Wb) / (Wa - Wb)
            ca, cb = la & ~lb, lb & ~la
            Ua2, Va2, Wa2 = np.where(ca, Ua + sa * (Ub - Ua), Ua), np.where(ca, Va + sa * (Vb - Va), Va), np.where(ca, Wa + sa * (Wb - Wa), Wa)
            Ub2, Vb2, Wb2 = np.where(cb, Ub + sb * (Ua - Ub), Ub), np.where(cb, Vb + sb * (Va - Vb), Vb), np.where(cb, Wb + sb * (Wa - Wb), Wb)
            pts = [Ua2 / Wa2, Va2 / Wa2, Ub2 / Wb2, Vb2 / Wb2]
            if affine is not None:
                A = np.asarray(affine, np.float64).reshape(6)
                pts = [(A[0] * pts[0] + A[1] * pts[1]) + A[2], (A[3] * pts[0] + A[4] * pts[1]) + A[5],
                       (A[0] * pts[2] + A[1] * pts[3]) + A[2], (A[3] * pts[2] + A[4] * pts[3]) + A[5]]
            segs[:n, j] = np.where((la & lb)[:, None], np.nan, np.stack(pts, 1))
            clipped[:n, j, 0], clipped[:n, j, 1] = ca, cb
        cls = np.zeros(n) if rows is None else np.asarray(rows, np.float64).reshape(-1, 14)[:n, 0]
        rgb[:n] = colours(cls, palette)[:, None]
    return segs.reshape(K * 14, 4), rgb.reshape(K * 14, 4), clipped.reshape(K * 14, 2)


def bev_quads(corners3d, rows, count, palette, scale, cx, cy):
    c3 = np.asarray(corners3d, np.float64).reshape(-1, 8, 3)
    K = len(c3)
    n = max(0, min(int(count), K))
    quads = np.full((K, 4, 2), np.nan)
    rgb = np.zeros((K, 4), np.uint8)
    with np.errstate(**ERR):
        quads[:n, :, 0] = np.float64(cx) + np.float64(scale) * c3[:n, :4, 0]
        quads[:n, :, 1] = np.float64(cy) - np.float64(scale) * c3[:n, :4, 2]
    rgb[:n] = colours(np.zeros(n) if rows is None else np.asarray(rows, np.float64).reshape(-1, 14)[:n, 0], palette)
    return quads, rgb


@functools.lru_cache(maxsize=None)
def bev_background(max_dist=60, scale=10):
    """plot.bev_background restated with the masks above: seven rays (thickness 2) and four rings, white on black, (R, 2R, 3)"""
    R = int(max_dist * scale)
    on = np.zeros((R, 2 * R), bool)
    for theta in np.linspace(0, np.pi, 7):
        on |= segment_mask(R, 2 * R, [int(R - R * np.cos(theta)), int(R - R * np.sin(theta)), R, R], 2)
    x, y = _grid(R, 2 * R, None)
    d2 = (x - R) * (x - R) + (y - R) * (y - R)
    for radius in np.linspace(0, R, 5)[1:]:
        rad = np.float64(int(radius))
        on |= ((rad - 1) * (rad - 1) <= d2) & (d2 <= (rad + 1) * (rad + 1))
    out = np.zeros((R, 2 * R, 3), np.uint8)
    out[on] = 255
    return out


def draw_bev(corners3d, rows, counts, palette, gt=None, max_dist=60, scale=10):
    """(B, K, 8, 3), (B, K, 14), (B,), gt = (corners (B, Kg, 8, 3), counts (B,)) or None -> (B, R, 2R, 3) uint8"""
    R = int(max_dist * scale)
    out = []
    for b in range(len(corners3d)):
        img = bev_background(max_dist, scale)
        if gt is not None:
            img = paint_quads(img, *bev_quads(gt[0][b], None, gt[1][b], [(0, 255, 0)], scale, R, R))
        out.append(paint_quads(img, *bev_quads(corners3d[b], rows[b], counts[b], palette, scale, R, R)))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- case lists
SEGMENT_KINDS = ("horizontal", "vertical", "diagonal", "steep", "point", "outside", "crossing", "nonfinite", "half", "general")


@functools.lru_cache(maxsize=None)
def segment_cases(B, H, W, S, stacked=False):
    """-> segs (B, S, 4) float64, rgb (B, S, 4) uint8 (a random fourth byte: it is ignored), kinds (S,) indices into SEGMENT_KINDS.
    stacked: every segment runs over the same pixels (jittered by less than a pixel), every one in its own colour."""
    rng = np.random.default_rng(1000 * B + 100 * H + 10 * W + S + (7 if stacked else 0))
    segs = np.zeros((B, S, 4))
    kinds = np.arange(S) % len(SEGMENT_KINDS)
    bad = (np.nan, np.inf, -np.inf)
    for b in range(B):
        for i in range(S):
            px, py = rng.uniform(-2, W + 1), rng.uniform(-2, H + 1)
            ln = rng.uniform(1, max(2.0, min(H, W) / 2))
            k = SEGMENT_KINDS[kinds[i]]
            if stacked:
                j = rng.uniform(-0.4, 0.4, 4)
                s = [1 + j[0], 1 + j[1], W - 2 + j[2], H - 2 + j[3]]
            elif k == "horizontal":
                s = [px, py, px + ln, py]
            elif k == "vertical":
                s = [px, py, px, py - ln]
            elif k == "diagonal":
                s = [np.floor(px), np.floor(py), np.floor(px) + np.floor(ln), np.floor(py) + np.floor(ln)]
            elif k == "steep":
                s = [px, py, px + ln / 7, py + ln]
            elif k == "point":
                s = [px, py, px, py]
            elif k == "outside":
                s = [W + 10 + px, -20 - py, W + 10 + px + ln, -20 - py + ln]
            elif k == "crossing":
                s = [-1e9, py - 1e9 * (i % 3 - 1) * 0.25, 1e9, py + 1e9 * (i % 3 - 1) * 0.25]
            elif k == "nonfinite":
                s = [px, py, px + ln, py + 1]
                s[(i // len(SEGMENT_KINDS)) % 4] = bad[(i // (4 * len(SEGMENT_KINDS))) % 3]
            elif k == "half":  # pixel centres at exactly t/2 for t = 1 (and t = 5 two rows on): the bound itself
                s = [np.floor(px) + 0.5, np.floor(py) + 0.5, np.floor(px) + 0.5 + np.floor(ln), np.floor(py) + 0.5]
            else:
                s = [px, py, rng.uniform(-2, W + 1), rng.uniform(-2, H + 1)]
            segs[b, i] = s
    rgb = rng.integers(0, 256, (B, S, 4), dtype=np.uint8)
    if stacked:  # all different
        rgb[..., 0], rgb[..., 1] = (np.arange(S) % 256)[None], (np.arange(S) // 256 + 1)[None]
    return segs, rgb, kinds


QUAD_KINDS = ("ccw", "cw", "flat", "edge", "vertex", "huge", "tiny", "nonfinite", "general")


@functools.lru_cache(maxsize=None)
def quad_cases(B, H, W, Q):
    """-> quads (B, Q, 4, 2), rgb (B, Q, 4), kinds (Q,) indices into QUAD_KINDS"""
    rng = np.random.default_rng(77 * B + 5 * H + 3 * W + Q)
    quads = np.zeros((B, Q, 4, 2))
    kinds = np.arange(Q) % len(QUAD_KINDS)
    for b in range(B):
        for i in range(Q):
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            w, h = rng.uniform(1, max(2.0, W / 3)), rng.uniform(1, max(2.0, H / 3))
            a = rng.uniform(0, np.pi)
            rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            box = np.array([[-w, -h], [w, -h], [w, h], [-w, h]]) / 2
            k = QUAD_KINDS[kinds[i]]
            if k == "ccw" or k == "general":
                q = box @ rot.T + [cx, cy]
            elif k == "cw":
                q = (box @ rot.T + [cx, cy])[::-1]
            elif k == "flat":  # all four on one line through pixel centres (exact coordinates): area exactly 0
                x0, y0 = np.floor(cx), np.floor(cy)
                q = np.array([[x0, y0], [x0 + 2, y0 + 1], [x0 + 4, y0 + 2], [x0 + 6, y0 + 3]], np.float64)
            elif k == "edge":  # integer corners: pixel centres lie exactly on the edges
                x0, y0 = np.floor(cx), np.floor(cy)
                q = np.array([[x0, y0], [x0 + np.ceil(w), y0], [x0 + np.ceil(w), y0 + np.ceil(h)], [x0, y0 + np.ceil(h)]])
            elif k == "vertex":  # a diamond with integer vertices: its vertices and edge midpoints are pixel centres
                x0, y0, r = np.floor(cx), np.floor(cy), np.ceil(w / 2)
                q = np.array([[x0 - r, y0], [x0, y0 - r], [x0 + r, y0], [x0, y0 + r]])
            elif k == "huge":
                q = np.array([[-5.0 * W, -5.0 * H], [6.0 * W, -5.0 * H], [6.0 * W, 6.0 * H], [-5.0 * W, 6.0 * H]])
            elif k == "tiny":  # inside one pixel, around its centre or beside it
                x0, y0 = np.floor(cx), np.floor(cy)
                off = 0.0 if (i // len(QUAD_KINDS)) % 2 == 0 else 0.3
                q = np.array([[-0.1, -0.1], [0.1, -0.1], [0.1, 0.1], [-0.1, 0.1]]) + [x0 + off, y0 + off]
            else:
                q = box + [cx, cy]
                q[(i // len(QUAD_KINDS)) % 4, i % 2] = (np.nan, np.inf, -np.inf)[(i // (4 * len(QUAD_KINDS))) % 3]
            quads[b, i] = q
    return quads, rng.integers(0, 256, (B, Q, 4), dtype=np.uint8), kinds


PALETTE4 = ((250, 10, 20), (30, 240, 50), (60, 70, 230), (200, 200, 90))


@functools.lru_cache(maxsize=None)
def box_cases(B, K):
    """boxes in front of, across and behind a KITTI-like camera -> corners3d (B, K, 8, 3), rows (B, K, 14) (classes in and out of the
    palette's range, NaN among them), counts (B,) (0 and K among them when B allows), P2 (B, 12), affine (B, 6), near.
    Box 0 of every image is axis-aligned with its front face at W == near exactly."""
    from yolov10_3d_amd import plot
    rng = np.random.default_rng(31 * B + K)
    rows = np.zeros((B, K, 14))
    rows[..., 0] = rng.choice([0, 1, 2, 3, 5, 17, -1, -0.5, 2.9, np.nan, np.inf, -np.inf, 1e30], (B, K))
    rows[..., 6], rows[..., 7], rows[..., 8] = rng.uniform(1.2, 2.0, (B, K)), rng.uniform(0.5, 2.0, (B, K)), rng.uniform(0.8, 4.5, (B, K))
    rows[..., 9], rows[..., 10] = rng.uniform(-15, 15, (B, K)), rng.uniform(1.0, 2.0, (B, K))
    rows[..., 11] = rng.uniform(-6, 50, (B, K))  # some behind the camera, some across the near plane
    rows[..., 12] = rng.uniform(-np.pi, np.pi, (B, K))
    near = 0.5
    P2 = np.zeros((B, 12))
    for b in range(B):
        f = 707.0493 + 10 * b
        P2[b] = [f, 0, 604.0814 + 3 * b, 45.75831 - b, 0, f, 180.5066 - 2 * b, -0.3454157 + 0.1 * b, 0, 0, 1, 0.0]
    rows[:, 0, 12], rows[:, 0, 8], rows[:, 0, 7], rows[:, 0, 11] = 0.0, 2.0, 1.0, 1.0  # z in {0.5, 1.5}: W == near on corners 1, 2, 5, 6
    c3 = np.stack([plot.corners3d_of(rows[b]) for b in range(B)])
    counts = np.array([K, 0, K // 2 + 1][:B], np.int32)
    affine = np.array([[0.97 + 0.01 * b, 0.001 * b, 1.5 * b, -0.002 * b, 0.976 - 0.01 * b, -0.75 * b] for b in range(B)])
    return c3, rows, counts, P2, affine, near
