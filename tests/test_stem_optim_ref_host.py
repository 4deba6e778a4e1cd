"""CPU: the host references of stem_optim_ref.py against independent statements (torch.nn.functional.conv2d in float64,
torch.optim.SGD / AdamW and clip_grad_norm_ in float64), the float32 restatements against the bounds the device is held to, and the
coverage that the case lists of test_hip_stem.py / test_hip_optim.py claim, checked from the lists themselves."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_optim_ref as S
import test_hip_optim as O
import test_hip_stem as T

# ------------------------------------------------------------------------------------------------------------------------- stem


def test_rne_bf16_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(0)
    x = torch.cat((torch.randn(100000, generator=g) * 10, torch.tensor(T.TIES, dtype=torch.float32),
                   torch.tensor([0.0, -0.0, 1.0, 255.0, 257.0, 259.0, 3.3895314e38, 1e-40, -1e-40, 2.0 ** -126])))
    r = S.rne_bf16(x)
    assert torch.equal(r.view(torch.int32), x.to(torch.bfloat16).float().view(torch.int32))
    assert S.rne_bf16(torch.tensor(T.TIES, dtype=torch.float32)).tolist() == [1.0, 1.015625, -1.0, -1.015625]
    assert S.rne_bf16(torch.tensor([257.0, 259.0])).tolist() == [256.0, 260.0]
    assert not torch.equal(r, x)


def test_uint8_samples_are_one_float32_division():
    v = torch.arange(256, dtype=torch.uint8).view(1, 1, 1, 256).expand(1, 3, 1, 256).contiguous()
    cols = S.stem_columns(v, 1)
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    # column (1*3+1)*3+0: the centre tap of channel 0 = pixel 2*ox
    assert np.array_equal(cols[0, 0, :, 12].numpy().view(np.int32), want[::2].view(np.int32))
    assert torch.equal(S._LUT, torch.arange(256).float() / 255)  # torch's CPU division is the same operation


@pytest.mark.parametrize("case", T.STEM_CASES + [(2, 6, 10)], ids=str)
def test_stem_reference_vs_conv2d_float64(case):
    """columns x weights == F.conv2d(stride 2, padding 1) in float64 on bf16-rounded operands, all three input modes"""
    B, H, W = case
    g = torch.Generator().manual_seed(sum(case))
    w = torch.randn(24, 3, 3, 3, generator=g)
    wcol = S.wcol_from_oihw(w)
    assert bool((wcol[:, 27:] == 0).all())
    for mode in (0, 1, 2):
        img = T.real_image(B, H, W, 3) if mode == 0 else T.u8_image(B, H, W, mode == 2, 4)
        cols = S.stem_columns(img, mode)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        assert cols.shape == (B, Ho, Wo, 32) and cols.dtype == torch.float32
        assert bool((cols[..., 27:] == 0).all()) and not bool(torch.signbit(cols[..., 27:]).any())
        x = img if mode == 0 else (img.permute(0, 3, 1, 2) if mode == 2 else img).float() / 255
        ref = F.conv2d(S.rne_bf16(x.contiguous()).double(), S.rne_bf16(w).double(), stride=2, padding=1).permute(0, 2, 3, 1)
        got = S.stem_conv(cols, wcol)
        assert got.dtype == torch.float64
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
        # the unrounded columns are the unfolded image itself
        unf = F.unfold(x.contiguous(), 3, padding=1, stride=2).view(B, 3, 9, Ho, Wo).permute(0, 3, 4, 2, 1).reshape(B, Ho, Wo, 27)
        assert torch.equal(cols[..., :27], unf)


def test_stem_case_list_reaches_every_path():
    allowed_h, allowed_w = {1, 2, 4, 5, 7}, {1, 2, 31, 127, 128, 129, 255, 256, 257}
    assert all(h in allowed_h and w in allowed_w for _, h, w in T.STEM_CASES) and 10 <= len(T.STEM_CASES) <= 14
    assert {h for _, h, _ in T.STEM_CASES} == allowed_h and {w for _, _, w in T.STEM_CASES} == allowed_w
    assert any(b >= 2 for b, _, _ in T.STEM_CASES) and any(h < 4 for _, h, _ in T.STEM_CASES)
    small = set().union(*(S.stem_features(*c) for c in T.STEM_CASES))
    assert small == {"fast_xb0", "fast_xb1+", "border_full", "border_lt16", "top_row", "bottom_padded", "bottom_unpadded", "idle_wave"}, small
    big = S.stem_features(*T.BIG_CASE)
    assert "wave_2_items" in big and "fast_xb1+" in big
    p = S.stem_path(*T.BIG_CASE)
    assert p["items"] == 8448 and p["grid"] == 2048 and p["waves"] == 8192 and p["n_max"] == 128 and (p["per_wave"] == 2).sum() == 256
    # a fast block with xb >= 1 in more than one image (the image offset matters), Wo off the 16- and 64-pixel grids
    assert any(c[0] >= 2 and "fast_xb1+" in S.stem_features(*c) for c in T.STEM_CASES)
    wos = {(w - 1) // 2 + 1 for _, _, w in T.STEM_CASES}
    assert any(wo % 16 and wo > 16 for wo in wos) and any(wo % 64 and wo > 64 for wo in wos)
    for B, H, W in T.STEM_CASES + [T.BIG_CASE]:
        p = S.stem_path(B, H, W)
        items = B * ((H + 1) // 2) * -(-((W + 1) // 2) // 64)
        assert p["items"] == items and p["grid"] == min(2048, math.ceil(items / 4)) and p["rows"] == 4 * p["grid"]
        assert p["per_wave"].sum() == items and len(p["fast"]) == items
        for it in range(min(items, 64)):  # the predicate, item by item, as the issue states it
            oy, xb = int(p["oy"][it]), int(p["xb"][it])
            assert bool(p["fast"][it]) == (2 * oy - 1 >= 0 and 2 * oy + 1 < H and xb * 128 + 128 <= W and xb * 64 + 64 <= p["Wo"])


@pytest.mark.parametrize("case", T.STEM_CASES, ids=str)
def test_stem_operands_have_the_properties_the_gpu_tests_rely_on(case):
    B, H, W = case
    n_max = S.stem_path(B, H, W)["n_max"]
    for Cout in T.COUTS:
        img, w, cols, acc = T.int_case(case, Cout)
        T.check_int_reference(acc, f"{case} Cout={Cout}")
        assert bool((acc == acc.round()).all()) and bool((img >= 0).all())
        assert torch.equal(S.rne_bf16(cols), cols) and torch.equal(S.rne_bf16(w), w)
        ys = S.rne_bf16(acc.float()).double()
        assert n_max * float(ys.abs().max()) < 2 ** 24
        assert T.stats_distinguishable(ys, acc, n_max)
        w1 = T.onehot_w(Cout)
        assert bool(((w1 != 0).sum(1) == 1).all()) and set(w1.abs().unique().tolist()) == {0.0, 1.0, 2.0, 4.0}
        assert bool((w1 < 0).any()) and bool((w1 > 0).any())
        assert (w1 != 0).any(0)[:min(Cout, 27)].all() and not (w1[:, 27:] != 0).any()
    img = T.real_image(B, H, W, sum(case))
    assert bool((img < 0).any()) and bool((img > 1).any())
    flat = img.view(-1)[:4].tolist()
    assert flat == [float(np.float32(t)) for t in T.TIES[:len(flat)]]
    assert not torch.equal(S.rne_bf16(img), img)
    for hwc in (False, True):
        u8 = T.u8_image(B, H, W, hwc, 1)
        assert u8.shape == ((B, H, W, 3) if hwc else (B, 3, H, W))
        if u8.numel() >= 256:
            assert len(u8.unique()) == 256


def test_some_uint8_case_holds_every_byte_value():
    assert sum(B * 3 * H * W >= 256 for B, H, W in T.STEM_CASES) >= 8


# -------------------------------------------------------------------------------------------------------------------- optimizer


def _rand(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


@pytest.mark.parametrize("nesterov,momentum,wd", [(1, 0.937, 5e-4), (0, 0.937, 5e-4), (1, 0.0, 0.0), (0, 0.9, 0.0)])
def test_sgd_f64_vs_torch_optim(nesterov, momentum, wd):
    if nesterov and momentum == 0:
        momentum_t, nesterov_t = 0.0, False  # torch refuses nesterov without momentum; the rule degenerates to plain SGD either way
    else:
        momentum_t, nesterov_t = momentum, bool(nesterov)
    lr = float(np.float32(0.013))
    wd, momentum_t = float(np.float32(wd)), float(np.float32(momentum_t))
    p0 = _rand(1000, 1)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum_t, nesterov=nesterov_t, weight_decay=wd)
    p, b = p0.astype(np.float64), np.full(1000, np.nan)
    for step in range(4):
        g = _rand(1000, 10 + step)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, b = S.sgd_f64(p, g, b, lr, wd, momentum, nesterov, int(step == 0))
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-14 * np.abs(p).max()
    # first = 0 on a zero buffer is the same first step (optim.py relies on it)
    a = S.sgd_f32(p0, g, np.zeros(1000), lr, wd, momentum, nesterov, 0)
    c = S.sgd_f32(p0, g, np.full(1000, np.nan), lr, wd, momentum, nesterov, 1)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[0].dtype == np.float32


def test_adamw_f64_vs_torch_optim():
    lr, wd, b1, b2, eps = (float(np.float32(x)) for x in (0.002, 0.01, 0.9, 0.999, 1e-8))
    p0 = _rand(1000, 2)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.astype(np.float64), np.zeros(1000), np.zeros(1000)
    for step in range(1, 5):
        g = _rand(1000, 20 + step, 0.3)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
        f1, f2 = S.bias_corrections(b1, b2, step)
        assert f1 == np.float32(bc1) and f2 == np.float32(bc2s)
        # float64 rule with unrounded bias corrections (np.float64 passes through _adamw's fp32 cast, so restate the cast here)
        p64, m64, v64 = p.copy(), m.copy(), v.copy()
        gv = g.astype(np.float64)
        m64 = m64 + (1 - b1) * (gv - m64)
        v64 = v64 * b2 + (1 - b2) * gv * gv
        p64 = p64 * (1 - lr * wd) - lr / bc1 * (m64 / (np.sqrt(v64) / bc2s + eps))
        assert np.abs(p64 - tp.detach().numpy()).max() <= 1e-13 * np.abs(p64).max()
        pn, mn, vn = S.adamw_f64(p, g, m, v, lr, wd, b1, b2, eps, f1, f2)
        # the cast of the bias corrections is the only difference: 2^-24 relative on the update term
        assert np.abs(pn - p64).max() <= 2.0 ** -22 * lr / float(f1)
        assert np.abs(mn - m64).max() <= 1e-15 and np.abs(vn - v64).max() <= 1e-15
        p, m, v = p64, m64, v64


def test_clip_vs_clip_grad_norm():
    grads = [_rand(n, n, 2.0) for n in (5, 300, 1027)]
    for max_norm in (0.5, 10.0, 1e6):
        ts = [torch.zeros(len(g), dtype=torch.float64, requires_grad=True) for g in grads]
        for t, g in zip(ts, grads):
            t.grad = torch.tensor(g, dtype=torch.float64)
        total = torch.nn.utils.clip_grad_norm_(ts, max_norm)
        part = S.sqnorm_partials(grads, 256)
        assert len(part) == 1 + 2 + 5
        n, c, f = S.clip_f64(part, max_norm)  # partials pass through fp32, as the device stores them
        assert abs(n - float(total)) <= 2.0 ** -23 * float(total) and f == 1
        for t, g in zip(ts, grads):
            assert np.abs(t.grad.numpy() - g.astype(np.float64) * c).max() <= 1e-6 * np.abs(g).max()
        assert (c == 1) == (max_norm >= float(total))
    with np.errstate(all="ignore"):
        assert S.clip_f32(np.array([1.0, np.inf], dtype=np.float32), 10.0)[2] == 0
        assert S.clip_f32(np.array([1.0, np.nan], dtype=np.float32), 10.0)[2] == 0
        assert S.clip_f32(np.array([4.0], dtype=np.float32), np.inf)[:2] == (2.0, 1.0)
        assert S.clip_f32(np.zeros(3, dtype=np.float32), 10.0) == (0.0, 1.0, 1.0)


def test_ema_and_copy_restatements():
    e, m = _rand(500, 3), _rand(500, 4)
    d = 0.9999 * (1 - math.exp(-3 / 2000))
    d32, o32 = float(np.float32(d)), float(np.float32(1 - d))
    for reps in (1, 2, 3):
        ref = e.astype(np.float64)
        for _ in range(reps):
            ref = ref * d32 + o32 * m.astype(np.float64)   # utils/torch_utils.py ModelEMA.update: v *= d; v += (1 - d) * model
        assert np.abs(S.ema_f64(e, m, d, 1 - d, reps) - ref).max() <= 1e-15
        got = S.ema_f32(e, m, d, 1 - d, reps)
        assert got.dtype == np.float32 and np.abs(got - ref).max() <= 3 * reps * S.U * (np.abs(e) + np.abs(m)).max()
    assert not np.array_equal(S.ema_f32(e, m, d, 1 - d, 1), S.ema_f32(e, m, d, 1 - d, 2))
    s = np.array([-0.0, 1.0, 3.0], dtype=np.float32)
    assert np.array_equal(S.copy_f32(s, 1.0).view(np.int32), s.view(np.int32))
    assert S.copy_f32(s, 1 / 3)[2] == np.float32(3.0) * np.float32(1 / 3)


def test_float32_restatements_fit_the_bounds_the_device_is_held_to():
    """adamw_f32 within adamw_bound of adamw_f64, bn_eval_scale_f32 within its bound, fp32 chunk sums within (chunk + 1) 2^-24"""
    rng = np.random.default_rng(0)
    n = 200000
    p, g = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.random(n) * 10.0 ** rng.uniform(-12, 1, n)).astype(np.float32)
    g[:100], m[:50], v[:200] = 0, 0, 0
    worst = 0.0
    for lr, wd, t, coef in ((0.002, 0.0, 1, 1.0), (0.02, 0.05, 2, 0.37), (1e-4, 5e-4, 1000, 1.0)):
        bc1, bc2s = S.bias_corrections(0.9, 0.999, t)
        args = (p, g, m, v, lr, wd, 0.9, 0.999, 1e-8, bc1, bc2s, coef)
        a, r, tol = S.adamw_f32(*args), S.adamw_f64(*args), S.adamw_bound(*args)
        for k in range(3):
            assert a[k].dtype == np.float32 and r[k].dtype == np.float64
            ratio = np.abs(a[k].astype(np.float64) - r[k]) / tol[k]
            assert ratio.max() <= 1, (k, ratio.max())
            worst = max(worst, ratio.max())
    assert worst > 0.05, "a bound that the float32 restatement does not come near would check little"
    for C in (1, 255, 256, 257, 5000):
        gamma, beta, mean = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
        var = (rng.random(C) ** 4 * 10).astype(np.float32)
        var[::5] = 0
        for eps in (1e-3, 1e-5):
            a, r, tol = (fn(gamma, beta, mean * 4, var, eps) for fn in (S.bn_eval_scale_f32, S.bn_eval_scale_f64, S.bn_eval_scale_bound))
            for k in range(2):
                assert (np.abs(a[k].astype(np.float64) - r[k]) <= tol[k]).all()
    for chunk in (256, 16384):
        x = (rng.standard_normal(chunk) * 3).astype(np.float32)
        want = np.sum(x.astype(np.float64) ** 2)
        sq = x * x
        seq = np.float32(0)
        for s in sq[:256]:
            seq = np.float32(seq + s)  # sequential
        strided = sq.reshape(-1, 256).sum(0, dtype=np.float32).sum(dtype=np.float32)  # the kernel's shape: per-thread, then a tree
        assert abs(float(strided) - want) <= (chunk + 1) * S.U * want
        assert abs(float(seq) - np.sum(x[:256].astype(np.float64) ** 2)) <= 257 * S.U * want
        nrm = S.clip_f32(np.array([strided]), 1.0)[0]
        assert abs(float(nrm) - math.sqrt(want)) <= ((chunk + 1) * S.U + 2.0 ** -23) * math.sqrt(want)


def test_optimizer_case_lists_reach_every_branch():
    for chunk, sizes in O.SIZES.items():
        assert any(n < chunk for n in sizes) and chunk in sizes and chunk + 1 in sizes and any(n > 2 * chunk for n in sizes)
        tails = {(n % chunk) & 3 for n in sizes}
        assert tails >= {0, 1, 3}  # empty and non-empty `n & 3` tails behind the 16-byte loop
        ct, co = S.chunk_table(sizes, chunk)
        assert len(ct) == sum(-(-n // chunk) for n in sizes) > len(sizes)  # more chunks than tensors: lr[chunk] != lr[tensor]
        assert all(c * chunk < sizes[t] for t, c in zip(ct, co))
    assert O.SIZES[256] == [1, 3, 4, 5, 255, 256, 257, 511, 512, 1027] and O.SIZES[16384] == [16383, 16384, 16385, 3 * 16384 + 5]
    assert {r for c, r in O.CFG if c == 256} == {0, 1, 2, 3} == {r for c, r in O.CFG if c == 16384}
    lr, wd = O.hyper(10)
    assert len(set(lr)) == 10 and 0.0 in wd and len(set(wd)) > 5
    assert {bool(v[2]) for v in O.SGD_VARIANTS} == {True, False} and {v[0] for v in O.SGD_VARIANTS} == {0, 1}
    assert any(v[1] == 0 for v in O.SGD_VARIANTS) and {v[3] is None for v in O.SGD_VARIANTS} == {True, False}
