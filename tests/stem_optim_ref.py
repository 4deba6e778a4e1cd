"""Host references for the stem kernels (csrc/stem_fused.hip, y3d_stem_im2col* of csrc/misc.hip), the multi-tensor optimizer kernels
(csrc/optim.hip) and y3d_bn_eval_scale, written from the operations' definitions; nothing here calls the code under test.

* stem: explicit window arithmetic in torch (any device: the one large case computes its reference where its data is), bf16 rounding by
  integer arithmetic on the bit pattern, the conv as a float64 contraction;
* optimizer: float32 restatements in numpy with ONE float32 operation per kernel operation in the kernel's order (the build compiles with
  -ffp-contract=off and the kernels are element-wise, so the device can be held to bit equality), and the same rules in float64;
* stem_path: per work item of stem_fused.hip, which of its two gather paths it takes, and how items fall on waves.
tests/test_stem_optim_ref_host.py pins every function against torch on the CPU."""
import math

import numpy as np
import torch

U = 2.0 ** -24  # fp32 unit roundoff
F = np.float32

# ------------------------------------------------------------------------------------------------------------------------- stem


def rne_bf16(x):
    """float32 tensor -> the nearest bf16 value (ties to even) as float32, by integer arithmetic on the bit pattern (finite inputs)"""
    assert x.dtype == torch.float32
    b = x.contiguous().view(torch.int32)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & -65536
    return r.view(torch.float32)


_LUT = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255))  # np.float32(v) / np.float32(255): one fp32 division


def stem_columns(img, in_mode):
    """img: in_mode 0 float32 (B, 3, H, W); 1 uint8 (B, 3, H, W); 2 uint8 (B, H, W, 3) -> float32 (B, Ho, Wo, 32): column (r*3+q)*3+ci
    is sample (ci, 2*oy-1+r, 2*ox-1+q) of the 3x3 stride-2 pad-1 window; padding and columns 27..31 are +0"""
    if in_mode == 0:
        assert img.dtype == torch.float32
        x = img
    else:
        assert img.dtype == torch.uint8
        x = _LUT.to(img.device)[img.long()]
        if in_mode == 2:
            x = x.permute(0, 3, 1, 2)
    B, C, H, W = x.shape
    assert C == 3
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = torch.zeros(B, 3, 2 * Ho + 1, 2 * Wo + 1, dtype=torch.float32, device=x.device)  # pad[.., i + 1, j + 1] = x[.., i, j]
    pad[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(B, Ho, Wo, 32, dtype=torch.float32, device=x.device)
    for r in range(3):
        for q in range(3):
            for ci in range(3):
                out[..., (r * 3 + q) * 3 + ci] = pad[:, ci, r:r + 2 * Ho:2, q:q + 2 * Wo:2]
    return out


def stem_conv(cols, wcol):
    """float64 (B, Ho, Wo, Cout): the contraction of the bf16-rounded columns with the bf16-rounded weights wcol (Cout, 32)"""
    return rne_bf16(cols).double() @ rne_bf16(wcol).double().T


def wcol_from_oihw(w):
    """(Cout, 3, 3, 3) OIHW -> (Cout, 32) with column (r*3+q)*3+ci, columns 27..31 zero"""
    Cout = w.shape[0]
    out = torch.zeros(Cout, 32, dtype=w.dtype, device=w.device)
    out[:, :27] = w.permute(0, 2, 3, 1).reshape(Cout, 27)
    return out


def stem_path(B, H, W):
    """stem_fused.hip's work decomposition restated: item it = (b * Ho + oy) * nxb + xb covers 64 output pixels of one row; wave
    w of the grid (min(2048, ceil(items / 4)) blocks of 4 waves) takes items w, w + waves, ...; an item takes the fast gather when its
    three input rows and its 128 input columns all lie inside the image and its 64 output pixels inside the row"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nxb = -(-Wo // 64)
    items = B * Ho * nxb
    grid = min(2048, -(-items // 4))
    waves = grid * 4
    it = np.arange(items)
    xb = it % nxb
    oy = (it // nxb) % Ho
    b = it // nxb // Ho
    fast = (2 * oy - 1 >= 0) & (2 * oy + 1 < H) & (xb * 128 + 128 <= W) & (xb * 64 + 64 <= Wo)
    valid = np.minimum(64, Wo - xb * 64)
    per_wave = np.bincount(it % waves, minlength=waves)
    return {"Ho": Ho, "Wo": Wo, "nxb": nxb, "items": items, "grid": grid, "waves": waves, "rows": waves, "b": b, "oy": oy, "xb": xb,
            "fast": fast, "valid": valid, "per_wave": per_wave, "n_max": int(-(-items // waves)) * 64}


def stem_features(B, H, W):
    """the set of path names (see test_stem_optim_ref_host.py) that a stem case reaches"""
    p = stem_path(B, H, W)
    f = set()
    fast, xb, oy, valid = p["fast"], p["xb"], p["oy"], p["valid"]
    if (fast & (xb == 0)).any():
        f.add("fast_xb0")
    if (fast & (xb >= 1)).any():
        f.add("fast_xb1+")
    if (~fast & (valid == 64)).any():
        f.add("border_full")
    if (~fast & (valid < 16)).any():
        f.add("border_lt16")
    if (2 * oy - 1 < 0).any():
        f.add("top_row")
    last = 2 * oy.max() + 1  # the last window row of the last output row
    f.add("bottom_padded" if last >= H else "bottom_unpadded")
    if (p["per_wave"] == 0).any():
        f.add("idle_wave")
    if (p["per_wave"] >= 2).any():
        f.add("wave_2_items")
    return f


# -------------------------------------------------------------------------------------------------------------------- optimizer
# Every function takes and returns numpy arrays of dtype `dt` (np.float32: the kernel's arithmetic, one rounding per operation;
# np.float64: the same rule in double).  Scalars are converted to `dt` first: the kernels receive them as fp32.


def _sgd(dt, p, g, buf, lr, wd, momentum, nesterov, first, coef=1.0):
    """optim.hip mt_sgd_kernel: gv = g*c (+ wd*p when wd != 0); bv = first ? gv : momentum*buf + gv; p -= lr * (nesterov ? gv +
    momentum*bv : bv) -> (p, buf)"""
    p, g, buf = p.astype(dt), g.astype(dt), buf.astype(dt)
    lr, wd, mom, c = dt(F(lr)), dt(F(wd)), dt(F(momentum)), dt(F(coef))
    gv = g * c
    if wd != 0:
        gv = gv + wd * p
    bv = gv if first else mom * buf + gv
    step = gv + mom * bv if nesterov else bv
    return p - lr * step, bv


def sgd_f32(*a, **k):
    return _sgd(np.float32, *a, **k)


def sgd_f64(*a, **k):
    return _sgd(np.float64, *a, **k)


def bias_corrections(beta1, beta2, t):
    """(bc1, bc2s) fp32: computed in float64 from the fp32 betas and the applied-step count, then cast (mt_adamw_kernel)"""
    b1, b2 = float(F(beta1)), float(F(beta2))
    return F(1.0 - b1 ** float(t)), F(math.sqrt(1.0 - b2 ** float(t)))


def _adamw(dt, p, g, m, v, lr, wd, beta1, beta2, eps, bc1, bc2s, coef=1.0):
    """optim.hip mt_adamw_kernel -> (p, m, v)"""
    p, g, m, v = p.astype(dt), g.astype(dt), m.astype(dt), v.astype(dt)
    lr, wd, b1, b2, eps, bc1, bc2s, c = (dt(F(x)) for x in (lr, wd, beta1, beta2, eps, bc1, bc2s, coef))
    one = dt(1)
    step_size, decay, w1, w2 = lr / bc1, one - lr * wd, one - b1, one - b2
    gv = g * c
    pv = p * decay
    mv = m + w1 * (gv - m)
    vv = v * b2 + w2 * gv * gv
    return pv - step_size * (mv / (np.sqrt(vv) / bc2s + eps)), mv, vv


def adamw_f32(*a, **k):
    return _adamw(np.float32, *a, **k)


def adamw_f64(*a, **k):
    return _adamw(np.float64, *a, **k)


def adamw_bound(p, g, m, v, lr, wd, beta1, beta2, eps, bc1, bc2s, coef=1.0):
    """|fp32 result - adamw_f64| bounds (tol_p, tol_m, tol_v) for ONE step from fp32 inputs, from the operation count (u = 2^-24):
    gv = g*c: u.  mv = m + w1*(gv - m): w1 = 1-beta1 (u), the difference (u, + u|gv| inherited), the product (u), the sum (u):
    tol_m = u|mv| + 4u w1 (|gv| + |m|).  vv = v*beta2 + (w2*gv)*gv: every term is positive, so the roundings of w2, gv (twice), the two
    products, v*beta2 and the sum stay relative: tol_v = 6u vv.  denom = sqrtf(vv)/bc2s + eps: half of 6u through the root + the root's
    own u + the division's u + the sum's u <= 6u denom.  T = step_size * (mv / denom): denom 6u + division u + step_size = lr/bc1 u +
    product u = 9u|T|, plus tol_m (which holds mv's own rounding, the tenth) scaled by step_size / denom.  pv = p*decay with
    decay = 1 - lr*wd (two roundings of a value near 1, then the product): 3u|p|; p' = pv - T: u|p'|.  (1 + 2^-10) covers second order."""
    f = lambda x: np.float64(F(x))
    lr, wd, b1, b2, eps, bc1, bc2s, c = (f(x) for x in (lr, wd, beta1, beta2, eps, bc1, bc2s, coef))
    p64, g64, m64, v64 = (x.astype(np.float64) for x in (p, g, m, v))
    pn, mn, vn = adamw_f64(p, g, m, v, lr, wd, b1, b2, eps, bc1, bc2s, c)
    gv = np.abs(g64 * c)
    tol_m = U * np.abs(mn) + 4 * U * (1 - b1) * (gv + np.abs(m64))
    tol_v = 6 * U * vn
    denom = np.sqrt(vn) / bc2s + eps
    T = np.abs(lr / bc1 * mn / denom)
    tol_p = U * (np.abs(pn) + 3 * np.abs(p64)) + 9 * U * T + (lr / bc1) / denom * tol_m
    s = 1 + 2.0 ** -10
    return tol_p * s + 1e-45, tol_m * s + 1e-45, tol_v * s + 1e-45


def _ema(dt, e, m, decay, one_minus_decay, reps):
    """optim.hip mt_ema_kernel: mv = omd*m once, then e = e*d + mv `reps` times"""
    e, m = e.astype(dt), m.astype(dt)
    d, omd = dt(F(decay)), dt(F(one_minus_decay))
    mv = omd * m
    for _ in range(reps):
        e = e * d + mv
    return e


def ema_f32(*a, **k):
    return _ema(np.float32, *a, **k)


def ema_f64(*a, **k):
    return _ema(np.float64, *a, **k)


def copy_f32(src, scale):
    return src.astype(F) * F(scale)


def sqnorm_partials(grads, chunk):
    """float64 sum of squares per chunk, chunks in table order (tensor by tensor) -> float64 array"""
    out = []
    for g in grads:
        g = g.astype(np.float64).reshape(-1)
        for o in range(0, g.size, chunk):
            out.append(np.sum(g[o:o + chunk] ** 2))
    return np.array(out, dtype=np.float64)


def _clip(dt, partials, max_norm):
    """mt_clip_kernel -> (norm, coef, finite flag): norm = dt(sqrt(float64 sum of the fp32 partials)), coef = min(1, max_norm /
    (norm + 1e-6))"""
    with np.errstate(all="ignore"):
        norm = dt(np.sqrt(np.sum(np.asarray(partials, dtype=F).astype(np.float64))))
        c = dt(F(max_norm)) / (norm + dt(F(1e-6)))
        coef = c if c < 1 else dt(1)
    return norm, coef, F(1.0 if np.isfinite(norm) else 0.0)


def clip_f32(partials, max_norm):
    return _clip(np.float32, partials, max_norm)


def clip_f64(partials, max_norm):
    return _clip(np.float64, partials, max_norm)


def chunk_table(sizes, chunk):
    """(chunk_tensor, chunk_off) as optim.py builds them: tensor by tensor, ceil(n / chunk) chunks each"""
    ct, co = [], []
    for t, n in enumerate(sizes):
        for c in range(-(-n // chunk)):
            ct.append(t)
            co.append(c)
    return ct, co


# ---------------------------------------------------------------------------------------------------------------- bn_eval_scale


def _bn_eval_scale(dt, gamma, beta, mean, var, eps):
    """scale = gamma / sqrt(var + eps); shift = beta - mean * scale"""
    gamma, beta, mean, var = (x.astype(dt) for x in (gamma, beta, mean, var))
    sc = gamma / np.sqrt(var + dt(F(eps)))
    return sc, beta - mean * sc


def bn_eval_scale_f32(*a):
    return _bn_eval_scale(np.float32, *a)


def bn_eval_scale_f64(*a):
    return _bn_eval_scale(np.float64, *a)


def bn_eval_scale_bound(gamma, beta, mean, var, eps):
    """scale: the sum var + eps (u), the root (half of that + its own u), the division (u): 3 roundings <= 3u|scale|.  shift: the
    product mean*scale (u, and the scale error times |mean|) and the difference (u): 4u|mean*scale| + u|shift|"""
    sc, sh = bn_eval_scale_f64(gamma, beta, mean, var, eps)
    s = 1 + 2.0 ** -10
    ms = np.abs(mean.astype(np.float64) * sc)
    return 3 * U * np.abs(sc) * s + 1e-45, (4 * U * ms + U * np.abs(sh)) * s + 1e-45
