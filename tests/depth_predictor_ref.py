"""float64 restatement of the reference's DepthPredictor (nn/modules/head.py:978-1042) and of the pieces the HIP kernels of
csrc/group_norm.hip / resize.hip compute, in plain NumPy / torch.nn.functional:

  gn_fwd / gn_bwd        GroupNorm over a biased input, x = y + b, summed over 1 or 3 sources, scaled, optionally ReLU'd; the backward is the
                         closed form (no autograd): dzh = dz scale mask, s1 = sum dzh gamma, s2 = sum dzh gamma xhat per (sample, group),
                         dy = rstd (dzh gamma - (s1 + xhat s2) / n), dgamma = sum dzh xhat, dbeta = sum dzh, db = sum dy
  bil_matrix / resize / resize_adj   ATen's align_corners=False bilinear rule as an (out x in) matrix per axis.  The source index and the
                         weights are computed in float32, as ATen (and the kernel) compute them; the interpolation itself is float64
  run                    the whole predictor forward and backward for a fixed cotangent of the logits, in the reference's order
                         (`device_order=False`: resize P5, then the 1x1 conv) or the device's (conv at P5's size, then resize the 128
                         channels); `rnd` rounds every tensor the device stores in the compute dtype (identity, or `bf16`)

CASES are the end-to-end cases of tools/make_golden_depth_predictor.py and tests/test_hip_depth_predictor.py; their inputs are drawn from
seeds (`case_inputs`), the parameters are the module's own initialisation under `SEED` with the GroupNorm affine pairs redrawn
(`redraw_affine`: the default gamma = 1, beta = 0 would hide a swapped pair)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HIDDEN, GROUPS, BINS, EPS = 128, 32, 80, 1e-5
SEED = 1042
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_predictor.npz")
CASES = (dict(name="x2", B=2, ch=(16, 32, 64), p3=(12, 20), p4=(6, 10), p5=(3, 5)),       # exact 2x
         dict(name="odd", B=3, ch=(8, 8, 8), p3=(9, 13), p4=(5, 7), p5=(3, 4)),           # P5 is not half of P4
         dict(name="s3d", B=2, ch=(128, 256, 512), p3=(48, 160), p4=(24, 80), p5=(12, 40)))  # the S-3D widths at 1280 x 384
SAMPLES = 1024  # the fixture keeps at most this many values of a tensor: flat[::ceil(numel / SAMPLES)], next to its sum
BRANCHES = (("downsample", 0, 1, 2, 1), ("proj", 0, 1, 1, 0), ("upsample", 0, 1, 1, 0))  # name, conv index, norm index, stride, padding
STAGES = (("depth_head", 0, 1), ("depth_head", 3, 4))


def ident(t):
    return t


def bf16(t):
    """round to bfloat16 as the device does: from the float32 value"""
    return t.float().bfloat16().double()


def sample(t):
    flat = np.asarray(t, dtype=np.float64).reshape(-1)
    return flat[::-(-flat.size // SAMPLES)]


def case_inputs(case):
    """-> ([P3, P4, P5] float32, cotangent of the logits float32), drawn from the case's own seed"""
    g = torch.Generator().manual_seed(SEED + 7 * (1 + [c["name"] for c in CASES].index(case["name"])))
    feats = [torch.randn(case["B"], c, *s, generator=g) for c, s in zip(case["ch"], (case["p3"], case["p4"], case["p5"]))]
    cot = torch.randn(case["B"], BINS + 1, *case["p4"], generator=g)
    return feats, cot


def redraw_affine(module, seed=SEED):
    """GroupNorm weights ~ U(0.5, 1.5), biases ~ U(-0.5, 0.5), in state_dict order from a generator of their own"""
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    return module


# ---- GroupNorm over a biased input -------------------------------------------------------------------------------------------------
def _per_channel(v, C, G):
    return v.repeat_interleave(C // G, 1).view(v.shape[0], C, 1, 1)


def gn_fwd(ys, bs, gammas, betas, eps=EPS, scale=1.0, relu=False, G=GROUPS):
    """-> (out, cache); ys: (B, C, H, W) float64 tensors"""
    tot, cache = 0.0, []
    for y, b, g, be in zip(ys, bs, gammas, betas):
        B, C, H, W = y.shape
        xg = (y + b.view(1, -1, 1, 1)).reshape(B, G, -1)
        mean = xg.mean(2, keepdim=True)
        rstd = 1.0 / torch.sqrt(((xg - mean) ** 2).mean(2, keepdim=True) + eps)
        xhat = ((xg - mean) * rstd).reshape(B, C, H, W)
        tot = tot + (xhat * g.view(1, -1, 1, 1) + be.view(1, -1, 1, 1))
        cache.append((xhat, rstd.reshape(B, G), mean.reshape(B, G)))
    pre = tot * scale
    return (pre.clamp_min(0.0) if relu else pre), (cache, pre)


def gn_bwd(dz, gammas, cache, scale=1.0, relu=False, G=GROUPS):
    """-> per source (dy, dgamma, dbeta, db_conv)"""
    srcs, pre = cache
    dzh = dz * scale * ((pre > 0).to(dz.dtype) if relu else 1.0)
    out = []
    for (xhat, rstd, _), g in zip(srcs, gammas):
        B, C, H, W = xhat.shape
        n = H * W * (C // G)
        dg = dzh * g.view(1, -1, 1, 1)
        s1 = _per_channel(dg.reshape(B, G, -1).sum(2), C, G)
        s2 = _per_channel((dg * xhat).reshape(B, G, -1).sum(2), C, G)
        dy = _per_channel(rstd, C, G) * (dg - (s1 + xhat * s2) / n)
        out.append((dy, (dzh * xhat).sum((0, 2, 3)), dzh.sum((0, 2, 3)), dy.sum((0, 2, 3))))
    return out


# ---- bilinear resize ---------------------------------------------------------------------------------------------------------------
def bil_matrix(inn, out):
    """(out, inn) float64 matrix of ATen's align_corners=False rule; indices and weights in float32 as ATen computes them"""
    f = np.float32
    scale = f(inn) / f(out)
    m = np.zeros((out, inn))
    for d in range(out):
        s = max(f(scale * f(f(d) + f(0.5))) - f(0.5), f(0.0))
        s = f(s)
        i0 = min(int(s), inn - 1)
        i1 = i0 + (1 if i0 < inn - 1 else 0)
        l1 = f(min(max(f(s - f(i0)), f(0.0)), f(1.0)))
        l0 = f(f(1.0) - l1)
        m[d, i0] += float(l0)
        m[d, i1] += float(l1)
    return m


def resize(x, size):
    ry, rx = (torch.from_numpy(bil_matrix(x.shape[2], size[0])), torch.from_numpy(bil_matrix(x.shape[3], size[1])))
    return torch.einsum("oh,bchw,pw->bcop", ry.to(x.dtype), x, rx.to(x.dtype))


def resize_adj(dy, size):
    """the adjoint of resize from an input of (H, W) = size"""
    ry, rx = (torch.from_numpy(bil_matrix(size[0], dy.shape[2])), torch.from_numpy(bil_matrix(size[1], dy.shape[3])))
    return torch.einsum("oh,bcop,pw->bchw", ry.to(dy.dtype), dy, rx.to(dy.dtype))


# ---- the predictor -----------------------------------------------------------------------------------------------------------------
def bin_values():
    size = 2 * (70 - 1) / (BINS * (1 + BINS))
    idx = torch.linspace(0, BINS - 1, BINS)
    return torch.cat([(idx + 0.5).pow(2) * size / 2 - size / 8 + 1, torch.tensor([70.0])])


def run(P, feats, cot, device_order=False, rnd=ident, dtype=torch.float64):
    """P: state_dict (any float dtype); feats: [P3, P4, P5]; cot: cotangent of the logits.  -> {"logits", "weighted_depth", "features",
    "d_feat0..2", "d_<state_dict key>"} as float64 tensors.  dtype=torch.float32 runs the same formulas in float32 (the yardstick)."""
    P = {k: v.detach().to(dtype) for k, v in P.items()}
    x = [rnd(f.detach().to(dtype)) for f in feats]
    size = tuple(x[1].shape[2:])
    ys, xs_conv, resized_branch = [], [], []
    for (name, ci, ni, s, p), xi in zip(BRANCHES, x):
        w = rnd(P[f"{name}.{ci}.weight"])
        resized_branch.append(tuple(F.conv2d(xi[:1], w, stride=s, padding=p).shape[2:]) != size)
        if not resized_branch[-1]:
            xs_conv.append(xi)
            ys.append(rnd(F.conv2d(xi, w, stride=s, padding=p)))
        elif device_order:
            xs_conv.append(xi)
            ys.append(rnd(resize(rnd(F.conv2d(xi, w, stride=s, padding=p)), size)))
        else:
            xs_conv.append(resize(xi, size))
            ys.append(F.conv2d(xs_conv[-1], w, stride=s, padding=p))
    names = [b[0] for b in BRANCHES]
    src, c0 = gn_fwd(ys, [P[f"{n}.0.bias"] for n in names], [P[f"{n}.1.weight"] for n in names], [P[f"{n}.1.bias"] for n in names], EPS, 1.0 / 3.0,
                     False)
    src = rnd(src)
    stage_in, stage_cache, features = [], [], None
    for name, ci, ni in STAGES:
        stage_in.append(src)
        y = rnd(F.conv2d(src, rnd(P[f"{name}.{ci}.weight"]), padding=1))
        src, c = gn_fwd([y], [P[f"{name}.{ci}.bias"]], [P[f"{name}.{ni}.weight"]], [P[f"{name}.{ni}.bias"]], EPS, 1.0, True)
        src = rnd(src)
        stage_cache.append(c)
        if features is None:
            features = src
    wc = rnd(P["depth_classifier.weight"])
    logits = rnd(F.conv2d(src, wc) + P["depth_classifier.bias"].view(1, -1, 1, 1))
    out = {"logits": logits, "features": features,
           "weighted_depth": (logits.softmax(1) * P["depth_bin_values"].view(1, -1, 1, 1)).sum(1)}
    # backward
    dz = rnd(cot.detach().to(dtype))
    out["d_depth_classifier.bias"] = dz.sum((0, 2, 3))
    out["d_depth_classifier.weight"] = torch.nn.grad.conv2d_weight(src, wc.shape, dz)
    d = rnd(torch.nn.grad.conv2d_input(src.shape, wc, dz))
    for (name, ci, ni), xin, c in zip(reversed(STAGES), reversed(stage_in), reversed(stage_cache)):
        (dy, dg, db, dbc), = gn_bwd(d, [P[f"{name}.{ni}.weight"]], c, 1.0, True)
        dy = rnd(dy)
        w = rnd(P[f"{name}.{ci}.weight"])
        out[f"d_{name}.{ni}.weight"], out[f"d_{name}.{ni}.bias"], out[f"d_{name}.{ci}.bias"] = dg, db, dbc
        out[f"d_{name}.{ci}.weight"] = torch.nn.grad.conv2d_weight(xin, w.shape, dy, padding=1)
        d = rnd(torch.nn.grad.conv2d_input(xin.shape, w, dy, padding=1))
    back = gn_bwd(d, [P[f"{n}.1.weight"] for n in names], c0, 1.0 / 3.0, False)
    for i, ((name, ci, ni, s, p), (dy, dg, db, dbc)) in enumerate(zip(BRANCHES, back)):
        dy = rnd(dy)
        w = rnd(P[f"{name}.{ci}.weight"])
        out[f"d_{name}.{ni}.weight"], out[f"d_{name}.{ni}.bias"], out[f"d_{name}.{ci}.bias"] = dg, db, dbc
        xin, resized = xs_conv[i], resized_branch[i]
        if resized and device_order:
            dy = rnd(resize_adj(dy, tuple(x[i].shape[2:])))  # 1x1 conv: its output has the input's size
        out[f"d_{name}.{ci}.weight"] = torch.nn.grad.conv2d_weight(xin, w.shape, dy, stride=s, padding=p)
        dx = torch.nn.grad.conv2d_input(xin.shape, w, dy, stride=s, padding=p)
        if resized and not device_order:
            dx = resize_adj(dx, tuple(x[i].shape[2:]))
        out[f"d_feat{i}"] = rnd(dx)
    return {k: v.double() for k, v in out.items()}


def rel_max(a, b):
    """max |a - b| / max |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
