"""NumPy restatements of the reference's foreground depth maps (KITTIDataset with load_depth_maps) and of the loss that consumes
them, and the case lists their tests share.

Depth maps (data/datasets/kitti.py:143-145, 170-201, 234-287, 384-385, 409-417):
  warp_nearest          Pillow's Image.transform(AFFINE, NEAREST, fillcolor=51), all three of its code paths
  kept_depths           the label filter chain -> the depth every kept line paints; line_table: the device path's (2, 64) table
  paint / paint_table   np.where per object, minimum, threshold (float64, the reference) / two table lookups (float32, the device)
  synthetic_mask        the deterministic masks of the fixture tree
  warp_cases, kernel_cases   the cases of tests/test_depth_map_ref_host.py and tests/test_hip_depth_map.py

ForegroundDepthMapLoss (utils/loss.py:1225-1365; LogitFocalLoss / focal_loss / one_hot :1399-1564):
  nearest_exact_index   ATen's nearest-exact source index (torchvision Resize(NEAREST_EXACT) of the depth maps)
  lid_targets           the LID bin of a depth, class num_bins for everything outside
  fgdm_loss_ref         loss, gradient wrt the logits (closed form) and targets, float64
  torch_fgdm            the reference's own formula written with torch.nn.functional, in any dtype (the float64 run checks the
                        restatement, the float32 run is the yardstick of the device tolerances)
  loss_cases            the deterministic cases of tests/test_depth_map_ref_host.py and tests/test_hip_fgdm_loss.py
"""
import math

import numpy as np

# ---- the depth maps --------------------------------------------------------------------------------------------------------------
FILL = 51  # the fillcolor of the reference's mask transform
WRITELIST = ("Car", "Pedestrian", "Cyclist")
MAX_OBJS = 50


def _scale_table(o, step, n):
    """Pillow's ImagingScaleAffine column / row table: a running double sum, -1 left of zero"""
    out = np.empty(n, np.int64)
    for i in range(n):
        out[i] = -1 if o < 0.0 else int(o)
        o += step
    return out


def warp_path(a, wide=False):
    """which of Pillow's NEAREST affine paths a mask takes: a 16-bit one (mode I;16) the generic path, an 8-bit one the scale or the
    fixed path by its matrix"""
    if wide:
        return "generic"
    return "scale" if float(a[1]) == 0.0 and float(a[3]) == 0.0 else "fixed"


def warp_nearest(mask, a, out_wh, flip=False):
    """Image.transform(out_wh, AFFINE, a, resample=NEAREST, fillcolor=51) of the (mirrored) mask, restated: (h, w) -> (H, W)"""
    m = np.asarray(mask)[:, ::-1] if flip else np.asarray(mask)
    h, w = m.shape
    W, H = int(out_wh[0]), int(out_wh[1])
    a = [float(v) for v in np.asarray(a, np.float64).reshape(6)]
    out = np.full((H, W), FILL, m.dtype)
    path = warp_path(a, m.dtype.itemsize == 2)
    if path == "generic":  # ImagingGenericTransform + affine_transform: closed form in double, COORD(v) = v < 0 ? -1 : (int)v
        xc, yc = np.arange(W, dtype=np.float64)[None, :] + 0.5, np.arange(H, dtype=np.float64)[:, None] + 0.5
        fx, fy = a[0] * xc + a[1] * yc + a[2], a[3] * xc + a[4] * yc + a[5]
        xin, yin = np.where(fx < 0, -1, np.trunc(fx)).astype(np.int64), np.where(fy < 0, -1, np.trunc(fy)).astype(np.int64)
        ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
        out[ok] = m[yin[ok], xin[ok]]
        return out
    if path == "scale":
        xin, yin = _scale_table(a[2] + a[0] * 0.5, a[0], W), _scale_table(a[5] + a[4] * 0.5, a[4], H)
        vx, vy = (xin >= 0) & (xin < w), (yin >= 0) & (yin < h)
        out[np.ix_(vy, vx)] = m[np.ix_(yin[vy], xin[vx])]
        return out
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    a0, a1, a3, a4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
    a2, a5 = fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    wrap = lambda v: ((v + 2 ** 31) % 2 ** 32) - 2 ** 31  # int32 arithmetic
    xin, yin = wrap(a2 + y * a1 + x * a0) >> 16, wrap(a5 + y * a4 + x * a3) >> 16
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out[ok] = m[yin[ok], xin[ok]]
    return out


def level_of(box, trunc, occ):
    height = float(box[3]) - float(box[1]) + 1
    if trunc == -1:
        return "DontCare"
    if height >= 40 and trunc <= 0.15 and occ <= 0:
        return "Easy"
    if height >= 25 and trunc <= 0.3 and occ <= 1:
        return "Moderate"
    if height >= 25 and trunc <= 0.5 and occ <= 2:
        return "Hard"
    return "UnKnown"


def parse_label(text):
    """label-file text -> one dict per line: type, trunc, occ, box (float32), h, pos (float32)"""
    out = []
    for ln in text.splitlines():
        if not ln.strip():
            continue
        f = ln.strip().split(" ")
        out.append(dict(type=f[0], trunc=float(f[1]), occ=float(f[2]), box=np.array([float(v) for v in f[4:8]], np.float32), h=float(f[8]),
                        pos=np.array([float(v) for v in f[11:14]], np.float32)))
    return out


def kept_depths(lines, n_cand, P2, trans, flip, scale, img_w, out_wh, dmin, dmax):
    """the filter chain of KITTIDataset.__getitem__ (kitti.py:234-278) over the first n_cand lines of one label file ->
    {line index: depth (float64) the line paints}.  P2: the image's (flipped when flip) float32 projection; trans: the crop matrix."""
    P = np.asarray(P2, np.float32).astype(np.float64)
    T = np.asarray(trans, np.float64).reshape(2, 3)
    out = {}
    for i, o in enumerate(lines[:n_cand]):
        if o["type"] not in WRITELIST:
            continue
        pos = o["pos"].astype(np.float64)
        if flip:
            pos[0] = -pos[0]
        zs = pos[2] * float(scale)
        if level_of(o["box"], o["trunc"], o["occ"]) == "UnKnown" or zs < dmin:
            continue
        if o["trunc"] > 0.5 or o["occ"] > 2:
            continue
        c = pos + np.array([0.0, -o["h"] / 2, 0.0])
        u = (c[0] * P[0, 0] + c[1] * P[0, 1] + c[2] * P[0, 2] + P[0, 3]) / c[2]
        v = (c[0] * P[1, 0] + c[1] * P[1, 1] + c[2] * P[1, 2] + P[1, 3]) / c[2]
        uv = np.array([np.float64(np.float32(u)), np.float64(np.float32(v)), 1.0])
        with np.errstate(invalid="ignore"):
            ctr = (T @ uv).astype(np.int32)
        if ctr[0] < 0 or ctr[0] >= out_wh[0] or ctr[1] < 0 or ctr[1] >= out_wh[1]:
            continue
        if zs > dmax:
            continue
        out[i] = zs
    return out


def line_table(own, partner):
    """kept_depths of the own and the partner's file -> the (2, 64) float32 table of the device path (+inf: no depth)"""
    t = np.full((2, 64), np.inf, np.float32)
    for row, d in enumerate((own, partner or {})):
        for i, v in d.items():
            t[row, i] = np.float32(v)
    return t


def paint(warped, warped_partner, own, partner, max_depth):
    """kitti.py:286-287, 384-385, 409-417: np.where per kept object, pixel-wise minimum, values beyond max_depth -> 0 (float64);
    an image without kept objects: zeros"""
    maps = [np.where(warped == i, d, 1000.0) for i, d in own.items()]
    if warped_partner is not None:
        maps += [np.where(warped_partner == i, d, 1000.0) for i, d in (partner or {}).items()]
    if not maps:
        return np.zeros(warped.shape, np.float64)
    dm = maps[0]
    for m in maps:
        dm = np.minimum(dm, m)
    return np.where(dm > max_depth, 0.0, dm)


def paint_table(warped, warped_partner, table, max_depth):
    """the device formulation: two table lookups per pixel (ids >= 64 match nothing) -> float32"""
    look = lambda ids, row: np.where(ids < 64, table[row][np.minimum(ids, 63)], np.float32(np.inf))
    v = look(warped.astype(np.int64), 0)
    if warped_partner is not None:
        v = np.minimum(v, look(warped_partner.astype(np.int64), 1))
    return np.where((v > np.float32(max_depth)) | np.isinf(v), np.float32(0), v).astype(np.float32)


def synthetic_mask(lines, index, W, H, bits=8):
    """The deterministic instance mask of a frame: background 255 (no line), every label line's 2D box painted with its line index,
    later lines over earlier ones, then vertical stripes of the ids 50, 51, 255 (and 300 in a 16-bit mask) that no kept line can
    carry.  -> (H, W) uint8, or uint16 for bits = 16"""
    m = np.full((H, W), 255, np.uint16 if bits == 16 else np.uint8)
    for i, o in enumerate(lines):
        x1, y1, x2, y2 = (float(v) for v in o["box"])
        xa, xb, ya, yb = max(int(math.floor(x1)), 0), min(int(math.ceil(x2)), W), max(int(math.floor(y1)), 0), min(int(math.ceil(y2)), H)
        if xb > xa and yb > ya:
            m[ya:yb, xa:xb] = i
    ids = [50, 51, 255] + ([300] if bits == 16 else [])
    for k, v in enumerate(ids):
        x0 = (97 * (index + 1) + 211 * k) % max(W - 8, 1)
        m[:, x0:x0 + 5] = v
    return m


def mask_bits(index):
    """frames alternate between 8- and 16-bit mask files"""
    return 16 if index % 3 == 1 else 8


def builder_maps(z, zd, name, dmin=1.0, dmax=120.0):
    """The depth maps of a recorded run restated from the files' text and the draws alone: z = tests/golden/kitti_labels.npz (label
    and calibration text, frame sizes, flipped projections), zd = tests/golden/kitti_depth_map.npz (the run's items and draws).
    -> (float64 maps (B, H, W) as the reference's, float32 maps as the device path's, (B, 2, 64) tables)"""
    res = tuple(int(v) for v in zd["resolution"])
    lines = [parse_label(str(t)) for t in z["label_text"]]
    P2 = lambda i: np.array(str(z["calib_text"][i]).splitlines()[2].split(" ")[1:], np.float32).reshape(3, 4)
    ref, dev, tabs = [], [], []
    for b, item in enumerate(int(i) for i in zd[f"{name}/items"]):
        flip, par = bool(zd[f"{name}/flip"][b]), int(zd[f"{name}/partner"][b])
        W, H = (int(v) for v in z["frame_wh"][item])
        P = z["flip_P2"][item] if flip else P2(item)
        kw = dict(P2=P, trans=zd[f"{name}/trans"][b], flip=flip, scale=float(zd[f"{name}/scale"][b]), img_w=W, out_wh=res, dmin=dmin, dmax=dmax)
        n0 = min(len(lines[item]), MAX_OBJS)
        own = kept_depths(lines[item], n0, **kw)
        a = zd[f"{name}/trans_inv"][b].reshape(6)
        w0 = warp_nearest(synthetic_mask(lines[item], item, W, H, mask_bits(item)), a, res, flip)
        partner, w1 = None, None
        if par >= 0:
            partner = kept_depths(lines[par], min(len(lines[par]), MAX_OBJS - n0), **kw)
            w1 = warp_nearest(synthetic_mask(lines[par], par, W, H, mask_bits(par)), a, res, flip)
        tab = line_table(own, partner)
        ref.append(paint(w0, w1, own, partner, dmax))
        dev.append(paint_table(w0, w1, tab, dmax))
        tabs.append(tab)
    return np.stack(ref), np.stack(dev), np.stack(tabs)


def crop_matrix(src_wh, out_wh, scale, shift, off):
    """the inverse crop matrix of get_affine_transform for an axis-aligned crop of `scale` times the source, its centre moved by
    `shift` (fractions of the source), with the off-diagonal terms set to `off` = (a[1], a[3])"""
    w, h = src_wh
    cw, ch = w * scale, h * scale
    cx, cy = w / 2 + shift[0] * w, h / 2 + shift[1] * h
    return np.array([cw / out_wh[0], off[0], cx - cw / 2, off[1], ch / out_wh[1], cy - ch / 2], np.float64)


KERNEL_MAX_DEPTH = 120.0
_VARIANTS = (  # (off-diagonal terms, flip, crop scale, shift, mask bits)
    ((0.0, 0.0), False, 0.8, (0.31, -0.27), 8), ((1e-17, -1e-17), True, 1.2, (-0.33, 0.21), 8), ((0.0, 0.0), True, 1.2, (0.29, 0.35), 16),
    ((-1e-17, 1e-17), False, 0.8, (-0.4, -0.3), 16), ((-0.0, 0.0), True, 1.0, (0.0, 0.0), 8))


def kernel_cases():
    """The launches of tests/test_hip_depth_map.py, B = 3 images each: a mixed one (90 x 40 source and partner), an unmixed one (61 x 23,
    NULL partner) and one without kept objects (an all-inf table), into outputs (W, H) = (67, 21) and (128, 24): W no multiple of a
    vector width, rows unaligned.  -> list of dict(name, out_wh, masks, partners, wide, flips, trans_inv (3, 6), table (3, 2, 64),
    max_depth, warped [(own, partner or None)], expect (3, H, W) float32)"""
    out = []
    for oi, out_wh in enumerate(((67, 21), (128, 24))):
        for vi, (off, flip, scale, shift, bits) in enumerate(_VARIANTS):
            rng = np.random.default_rng(100 * oi + vi)
            dt = np.uint16 if bits == 16 else np.uint8
            ids = np.array(list(range(12)) + [50, 51, 255] + ([300] if bits == 16 else []))

            def mask(h, w):
                m = ids[rng.integers(len(ids), size=(h // 4 + 1, w // 6 + 1))].repeat(4, 0).repeat(6, 1)[:h, :w]  # blocks of one id
                return np.ascontiguousarray(m.astype(dt))

            masks = [mask(40, 90), mask(23, 61), mask(40, 90)]
            partners = [mask(40, 90).astype(np.uint8 if vi % 2 else dt), None, None]  # a partner of the other bit depth in every other case
            table = np.full((3, 2, 64), np.inf, np.float32)
            table[0, 0, :12] = rng.uniform(2, 119, 12).astype(np.float32)
            table[0, 1, :12] = rng.uniform(2, 119, 12).astype(np.float32)
            table[1, 0, :12] = rng.uniform(2, 119, 12).astype(np.float32)
            table[0, 0, [3, 7]] = np.inf       # dropped lines: their pixels stay 0 unless the partner paints them
            table[0, 1, [2, 7]] = np.inf
            table[1, 0, 5] = np.inf
            table[0, 0, 1] = KERNEL_MAX_DEPTH  # a depth equal to the threshold keeps its pixels
            table[1, 0, 2] = KERNEL_MAX_DEPTH
            table[1, 0, 4] = 130.0             # beyond it (only a caller's own table can hold one): 0
            flips = [flip, not flip, flip]
            tinv = np.stack([crop_matrix((m.shape[1], m.shape[0]), out_wh, scale, (shift[0] * s, shift[1] * s), off)
                             for m, s in zip(masks, (1.0, -1.0, 0.5))])
            wide = [(m.dtype.itemsize == 2, q is not None and q.dtype.itemsize == 2) for m, q in zip(masks, partners)]
            warped = [(warp_nearest(m, a, out_wh, f), None if q is None else warp_nearest(q, a, out_wh, f))
                      for m, q, a, f in zip(masks, partners, tinv, flips)]
            expect = np.stack([paint_table(w0, w1, t, KERNEL_MAX_DEPTH) for (w0, w1), t in zip(warped, table)])
            out.append(dict(name=f"{out_wh[0]}x{out_wh[1]}-v{vi}", out_wh=out_wh, masks=masks, partners=partners, wide=wide, flips=flips,
                            trans_inv=tinv, table=table, max_depth=KERNEL_MAX_DEPTH, warped=warped, expect=expect))
    return out


DMIN, DMAX = 1.0, 120.0  # kitti.DATA_ARGS: min_depth_threshold, max_depth_threshold
ALPHA, GAMMA, FG_W, BG_W = 0.25, 2.0, 13.0, 1.0


def nearest_exact_index(out, inn):
    """aten/src/ATen/native/UpSample.h nearest_neighbor_exact_compute_source_index: scale = float(in) / out in float32, the product
    (dst + 0.5) * scale in double, floorf of its float32 rounding, clamped to in - 1"""
    scale = np.float32(inn) / np.float32(out)
    prod = (np.arange(out, dtype=np.float64) + 0.5) * np.float64(scale)
    return np.minimum(np.floor(prod.astype(np.float32)).astype(np.int64), inn - 1)


def bin_size(dmin, dmax, num_bins):
    return 2 * (dmax - dmin) / (num_bins * (1 + num_bins))


def bin_edge(k, dmin, dmax, num_bins):
    """the depth at which the LID index is exactly k"""
    return dmin + bin_size(dmin, dmax, num_bins) * k * (k + 1) / 2


def lid_targets(d, dmin, dmax, num_bins):
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore"):
        idx = -0.5 + 0.5 * np.sqrt(1 + 8 * (d - dmin) / bin_size(dmin, dmax, num_bins))
        bad = (idx < 0) | (idx > num_bins) | ~np.isfinite(idx)
    return np.where(bad, num_bins, np.where(bad, 0.0, idx).astype(np.int64)).astype(np.int64)


def sample_maps(maps, h, w):
    maps = np.asarray(maps)
    ys, xs = nearest_exact_index(h, maps.shape[1]), nearest_exact_index(w, maps.shape[2])
    return maps[:, ys][:, :, xs]


def fgdm_loss_ref(z, maps, num_bins=80, dmin=DMIN, dmax=DMAX, alpha=ALPHA, gamma=GAMMA, fg_weight=FG_W, bg_weight=BG_W):
    """z: (B, num_bins + 1, h, w), maps: (B, H, W) -> (loss, d loss / d z (B, C, h, w), targets (B, h, w)), all in float64"""
    z = np.asarray(z, np.float64)
    B, C, h, w = z.shape
    assert C == num_bins + 1 and (h, w) == (maps.shape[1] // 16, maps.shape[2] // 16)
    d = sample_maps(maps, h, w).astype(np.float64)
    t = lid_targets(d, dmin, dmax, num_bins)
    zm = z - z.max(1, keepdims=True)
    ls = np.log(np.exp(zm).sum(1, keepdims=True))
    lp = zm - ls
    p = np.exp(lp)
    q = 1 - p
    wgt = (np.arange(C)[None, :, None, None] == t[:, None]).astype(np.float64) + 1e-6
    cell = (wgt * (-alpha * q ** gamma * lp)).sum(1)
    bal = np.where(d > 0, float(fg_weight), float(bg_weight))
    n = B * h * w
    loss = (bal * cell).sum() / n
    # p f'(p) without a division by p
    second = gamma * q ** (gamma - 1) * p * lp if gamma != 0 else 0.0
    g = -alpha * (q ** gamma - second)
    S = (wgt * g).sum(1, keepdims=True)
    grad = (bal / n)[:, None] * (wgt * g - p * S)
    return loss, grad, t


def torch_fgdm(z, maps, dtype, num_bins=80, dmin=DMIN, dmax=DMAX, alpha=ALPHA, gamma=GAMMA, fg_weight=FG_W, bg_weight=BG_W):
    """the reference's formula with torch.nn.functional on the CPU, logits and focal arithmetic in `dtype`, the depth maps and their
    bins in float64 -> (loss, autograd gradient, targets) as float64 / int64 arrays"""
    import torch
    import torch.nn.functional as F

    z = torch.as_tensor(np.asarray(z)).to(dtype).requires_grad_(True)
    dm = torch.as_tensor(np.asarray(maps)).double()
    h, w = dm.shape[1] // 16, dm.shape[2] // 16
    d = F.interpolate(dm[:, None], size=(h, w), mode="nearest-exact")[:, 0]
    idx = -0.5 + 0.5 * torch.sqrt(1 + 8 * (d - dmin) / bin_size(dmin, dmax, num_bins))
    idx[(idx < 0) | (idx > num_bins) | ~torch.isfinite(idx)] = num_bins
    t = idx.long()
    soft, logsoft = F.softmax(z, dim=1), F.log_softmax(z, dim=1)
    onehot = torch.zeros_like(soft).scatter_(1, t[:, None], 1.0) + 1e-6
    focal = -alpha * torch.pow(-soft + 1.0, gamma) * logsoft
    cell = torch.einsum("bc...,bc...->b...", onehot, focal)
    fg = d > 0
    weights = fg_weight * fg + bg_weight * ~fg
    cell = cell * weights
    num = fg.sum() + (~fg).sum()
    loss = cell[fg].sum() / num + cell[~fg].sum() / num
    loss.backward()
    return float(loss.detach().double()), z.grad.double().numpy(), t.numpy()


# ---- cases ---------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = (((2, 48, 80), (3, 5)), ((1, 37, 53), (2, 3)))  # (maps (B, H, W), grid (h, w)); the second: sides that are no multiple of 16
LOSS_BINS = (80, 4)
LOSS_KINDS = ("random", "saturated", "background", "foreground", "edges")


def _map_of(kind, shape, num_bins, rng):
    n = int(np.prod(shape))
    if kind == "background":
        m = np.zeros(n)
    elif kind == "foreground":
        m = rng.uniform(DMIN, DMAX, n)
    elif kind == "edges":
        # every bin edge (the float32 rounding decides the side), dmax itself, beyond dmax, below dmin, the background
        vals = [bin_edge(k, DMIN, DMAX, num_bins) for k in range(num_bins + 1)] + [DMAX, DMAX + 1e-3, 500.0, 0.5, 0.0]
        m = np.resize(np.asarray(vals), n).reshape(shape)
        # the loss reads one pixel per cell: lay the values along those pixels as well, so that every kind of value is sampled
        h, w = shape[1] // 16, shape[2] // 16
        ys, xs = nearest_exact_index(h, shape[1]), nearest_exact_index(w, shape[2])
        k = 0
        for b in range(shape[0]):
            for y in ys:
                for x in xs:
                    m[b, y, x] = vals[(k * 7) % len(vals)]
                    k += 1
        return m.astype(np.float32)
    else:
        # half background, the rest anywhere from below dmin to beyond dmax
        m = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.5, 130.0, n))
    return m.reshape(shape).astype(np.float32)


def loss_cases():
    """-> list of dict(name, num_bins, z (B, C, h, w) float32, maps (B, H, W) float32), the same on every call"""
    out = []
    for si, (mshape, (h, w)) in enumerate(LOSS_SHAPES):
        for nb in LOSS_BINS:
            for ki, kind in enumerate(LOSS_KINDS):
                rng = np.random.default_rng(1000 * si + 10 * nb + ki)
                maps = _map_of(kind, mshape, nb, rng)
                z = rng.normal(0.0, 2.0, (mshape[0], nb + 1, h, w))
                if kind == "saturated":
                    # +-80 in one channel of every cell: alternately the target's channel and another one, alternately + and -
                    t = lid_targets(sample_maps(maps, h, w), DMIN, DMAX, nb)
                    k = 0
                    for b in range(mshape[0]):
                        for i in range(h):
                            for j in range(w):
                                c = int(t[b, i, j]) if k % 2 == 0 else (int(t[b, i, j]) + 1 + k) % (nb + 1)
                                z[b, c, i, j] = 80.0 if (k // 2) % 2 == 0 else -80.0
                                k += 1
                out.append(dict(name=f"{kind}-{mshape[1]}x{mshape[2]}-b{nb}", kind=kind, num_bins=nb, z=z.astype(np.float32), maps=maps))
    return out


def rel_max(a, ref):
    """largest element distance over the largest reference magnitude"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))
