"""The multi-tensor optimizer kernels of csrc/optim.hip through the C ABI, with the test's own pointer / size / chunk tables:
y3d_mt_sqnorm, y3d_mt_clip_coef, y3d_mt_sgd, y3d_mt_adamw, y3d_mt_ema, y3d_mt_copy, and FusedSGD / FusedAdamW checkpoints.

* the kernels are element-wise fp32 and the build uses -ffp-contract=off, so the float32 restatements of stem_optim_ref.py (one numpy
  float32 operation per kernel operation, in the kernel's order) are held to BIT equality: parameters AND momentum / Adam state.  No
  update is idempotent, so bit equality also shows that every element was updated exactly once;
* tensors, state and copy destinations are slices of sentinel-filled arenas with gaps between them, slice starts at element offsets
  0, 1, 2, 3 (mod 4): the 16-byte and the scalar branches of mt_sqnorm / mt_copy both run, with `n & 3` tails; after every launch the
  gaps still hold the sentinel;
* chunk = 256 (the smallest the ABI takes) and 16384, sizes on both sides of every chunk edge; every tensor has its own lr and
  weight decay (some 0), so a table indexed by chunk instead of by tensor fails;
* mt_sqnorm: integer gradients |g| <= 8 make every partial an exact integer in any order: partials, norm and coefficient are
  bit-equal to clip_f32.  Real gradients: a chunk's sum of n <= chunk squares (each one rounding) accumulated in fp32 in any order is
  within (chunk + 1) 2^-24 relative of the float64 sum; the norm adds the root's and the cast's roundings, 2^-23;
* mt_adamw is additionally held to float64 within stem_optim_ref.adamw_bound (derived there from the operation count).
tests/test_stem_optim_ref_host.py pins the restatements to torch.optim on the CPU."""
import math

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import Y3DError

import stem_optim_ref as S
import tail_ref as R
from test_hip_eval_tail import assert_bits

DEV = "cuda"
F = np.float32
SIZES = {256: [1, 3, 4, 5, 255, 256, 257, 511, 512, 1027], 16384: [16383, 16384, 16385, 3 * 16384 + 5]}
CFG = [(256, 0), (256, 1), (256, 2), (256, 3), (16384, 0), (16384, 1), (16384, 2), (16384, 3)]  # (chunk, rotation of the start offsets)
CFG_IDS = [f"chunk{c}-rot{r}" for c, r in CFG]


def hyper(n):
    """per-tensor lr and weight decay, every third tensor without decay"""
    return [0.01 * (1 + t / 7) for t in range(n)], [0.0 if t % 3 == 0 else 5e-4 * (t + 1) for t in range(n)]


class Arena:
    """tensors of `sizes` as slices of ONE sentinel-filled fp32 buffer: tensor i starts at an element offset = (i + rot) mod 4, gaps of
    at least 5 sentinel elements on both sides of every slice"""

    def __init__(self, sizes, rot):
        pos, self.spans = 8, []
        for i, n in enumerate(sizes):
            pos = (pos + 3) // 4 * 4 + (i + rot) % 4
            self.spans.append((pos, n))
            pos += n + 5
        self.buf = R.sentinel((pos + 8,), torch.float32, DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + n] for o, n in self.spans]
        gap = torch.ones(pos + 8, dtype=torch.bool)
        for o, n in self.spans:
            gap[o:o + n] = False
        self.gap = gap.to(DEV)
        self.ptrs = torch.tensor([v.data_ptr() for v in self.views], dtype=torch.int64, device=DEV)

    def put(self, arrays):
        for v, a in zip(self.views, arrays):
            v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F)))
        return self

    def get(self):
        return [v.cpu().numpy().copy() for v in self.views]

    def check_gaps(self, what):
        assert bool(R.untouched(self.buf[self.gap]).all()), f"{what}: a store went outside its tensor"


class Tables:
    def __init__(self, sizes, chunk):
        ct, co = S.chunk_table(sizes, chunk)
        self.n, self.chunk = len(ct), chunk
        self.sizes = torch.tensor(sizes, dtype=torch.int64, device=DEV)
        self.ct = torch.tensor(ct, dtype=torch.int32, device=DEV)
        self.co = torch.tensor(co, dtype=torch.int32, device=DEV)
        lr, wd = hyper(len(sizes))
        self.lr_h, self.wd_h = lr, wd
        self.lr = torch.tensor(lr, dtype=torch.float32, device=DEV)
        self.wd = torch.tensor(wd, dtype=torch.float32, device=DEV)

    @property
    def tail(self):
        return self.sizes.data_ptr(), self.ct.data_ptr(), self.co.data_ptr(), self.n, self.chunk


def rand_list(sizes, rng, scale=1.0):
    return [(rng.standard_normal(n) * scale).astype(F) for n in sizes]


def int_list(sizes, rng):
    return [rng.integers(-8, 9, n).astype(F) for n in sizes]


def same_bits(got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert_bits(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b, dtype=F)), f"{what} tensor {t}")


def guarded_out(n, zero=True):
    """(buffer, first n elements): sentinel behind; the n elements zeroed (the clip counters accumulate)"""
    buf = R.sentinel((n + 64,), torch.float32, DEV)
    if zero:
        buf[:n] = 0
    return buf, buf[:n]


def sqnorm_clip(ar_g, tb, max_norm, out):
    """mt_sqnorm -> mt_clip_coef; -> partials (numpy)"""
    L, st = y3d.lib(), ops.stream()
    pbuf = R.sentinel((tb.n + 64,), torch.float32, DEV)
    L.mt_sqnorm(ar_g.ptrs.data_ptr(), *tb.tail, pbuf.data_ptr(), st)
    L.mt_clip_coef(pbuf.data_ptr(), tb.n, max_norm, out.data_ptr(), st)
    torch.cuda.synchronize()
    assert not bool(R.untouched(pbuf[:tb.n]).any()) and bool(R.untouched(pbuf[tb.n:]).all()), "mt_sqnorm: partials written outside [0, nchunks)"
    return pbuf[:tb.n].cpu().numpy()


# ---- mt_sqnorm + mt_clip_coef ----------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rot", CFG, ids=CFG_IDS)
def test_sqnorm_and_clip_integer_gradients_bit_for_bit(chunk, rot):
    sizes = SIZES[chunk]
    rng = np.random.default_rng(chunk + rot)
    tb = Tables(sizes, chunk)
    grads = int_list(sizes, rng)
    ar = Arena(sizes, rot).put(grads)
    want_p = S.sqnorm_partials(grads, chunk)
    assert want_p.max() < 2 ** 24 and len(want_p) == tb.n
    norm = math.sqrt(want_p.sum())
    for max_norm in (norm / 3, norm * 2, float("inf"), 1e-3):  # above the bound, below it (coefficient exactly 1), no bound, tiny
        obuf, out = guarded_out(5)
        part = sqnorm_clip(ar, tb, max_norm, out)
        same_bits([part], [want_p.astype(F)], f"mt_sqnorm chunk={chunk} rot={rot} partials")
        n, c, f = S.clip_f32(want_p.astype(F), max_norm)
        same_bits([out.cpu().numpy()], [np.array([n, c, f, 1, 0], dtype=F)], f"mt_clip_coef max_norm={max_norm}")
        if max_norm >= norm:
            assert float(out[1]) == 1.0
        else:
            assert float(out[1]) < 1.0
        assert bool(R.untouched(obuf[5:]).all())
    ar.check_gaps("mt_sqnorm")
    # all-zero gradients: norm 0, coefficient min(1, max_norm / 1e-6) = 1
    ar.put([np.zeros(n) for n in sizes])
    _, out = guarded_out(5)
    part = sqnorm_clip(ar, tb, 10.0, out)
    assert not part.any()
    same_bits([out.cpu().numpy()], [np.array([0, 1, 1, 1, 0], dtype=F)], "mt_clip_coef zero gradients")
    n, c, f = S.clip_f32(part, 1e-7)  # max_norm below the 1e-6 of the denominator: the one case where zero gradients give c < 1
    _, out = guarded_out(5)
    sqnorm_clip(ar, tb, 1e-7, out)
    same_bits([out.cpu().numpy()[:3]], [np.array([n, c, f], dtype=F)], "mt_clip_coef zero gradients, max_norm 1e-7")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rot", CFG, ids=CFG_IDS)
def test_sqnorm_real_gradients_within_the_any_order_bound(chunk, rot):
    sizes = SIZES[chunk]
    rng = np.random.default_rng(7 * chunk + rot)
    tb = Tables(sizes, chunk)
    grads = rand_list(sizes, rng, 3.0)
    ar = Arena(sizes, rot).put(grads)
    _, out = guarded_out(5)
    part = sqnorm_clip(ar, tb, 1.0, out).astype(np.float64)
    want = S.sqnorm_partials(grads, chunk)
    rel = np.abs(part - want) / want
    print(f"mt_sqnorm chunk={chunk} rot={rot}: worst partial {rel.max():.3g} relative, bound {(chunk + 1) * S.U:.3g}")
    assert (rel <= (chunk + 1) * S.U).all()
    norm = math.sqrt(want.sum())
    assert abs(float(out[0]) - norm) <= ((chunk + 1) * S.U + 2.0 ** -23) * norm
    n, c, f = S.clip_f32(part.astype(F), 1.0)  # from the device's own partials the tail is exact again
    same_bits([out.cpu().numpy()[:3]], [np.array([n, c, f], dtype=F)], "mt_clip_coef from the device's partials")


@pytest.mark.gpu
def test_nonfinite_gradients_clear_the_flag_and_count_as_skipped():
    """chunk 256, tensors at offsets 0..3 (mod 4).  NaN in the last element of the tail chunk of an unaligned tensor; +inf in a
    vector-path element of an aligned one; finite 1e20 whose squares overflow.  Counters over applied, skipped, skipped, applied"""
    sizes = SIZES[256]
    rng = np.random.default_rng(3)
    tb = Tables(sizes, 256)
    ar = Arena(sizes, 0)
    assert ar.spans[9][0] % 4 == 1 and sizes[9] == 1027 and ar.spans[8][0] % 4 == 0
    good = rand_list(sizes, rng)
    nan = [g.copy() for g in good]
    nan[9][-1] = np.nan      # element 1026: chunk 4 of the tensor (3 elements), scalar branch
    inf = [g.copy() for g in good]
    inf[8][256 + 17] = np.inf  # aligned tensor, second chunk, float4 loop
    big = [g.copy() for g in good]
    big[4][100] = 1e20
    obuf, out = guarded_out(5)
    applied, skipped = [], []
    for grads, flag in ((good, 1), (nan, 0), (inf, 0), (good, 1)):
        ar.put(grads)
        sqnorm_clip(ar, tb, 10.0, out)
        o = out.cpu().numpy()
        assert o[2] == flag, f"finite flag {o[2]} expected {flag}"
        applied.append(float(o[3])), skipped.append(float(o[4]))
    assert applied == [1, 1, 1, 2] and skipped == [0, 1, 2, 2], (applied, skipped)
    ar.put(big)
    part = sqnorm_clip(ar, tb, 10.0, out)
    o = out.cpu().numpy()
    assert np.isinf(part).sum() == 1 and np.isinf(o[0]) and o[2] == 0 and o[3] == 2 and o[4] == 3
    assert bool(R.untouched(obuf[5:]).all())


# ---- mt_sgd ----------------------------------------------------------------------------------------------------------------------------

# (nesterov, momentum, first step with a NaN-filled buffer, clip: None | coefficient)
SGD_VARIANTS = [(1, 0.937, False, None), (0, 0.937, False, None), (1, 0.0, False, None), (1, 0.937, True, None), (0, 0.9, True, 0.37),
                (1, 0.937, False, 0.37)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", SGD_VARIANTS, ids=[f"nesterov{a}-mom{b}-first{int(c)}-clip{d}" for a, b, c, d in SGD_VARIANTS])
@pytest.mark.parametrize("chunk,rot", [(256, 0), (256, 1), (16384, 2)], ids=["chunk256-rot0", "chunk256-rot1", "chunk16384-rot2"])
def test_sgd_bit_for_bit(chunk, rot, variant):
    nesterov, momentum, first_nan, coef = variant
    L, st = y3d.lib(), ops.stream()
    sizes = SIZES[chunk]
    rng = np.random.default_rng(chunk + rot + 11)
    tb = Tables(sizes, chunk)
    p, b = rand_list(sizes, rng), rand_list(sizes, rng, 0.1)
    ap, ag, ab = Arena(sizes, rot).put(p), Arena(sizes, rot + 1), Arena(sizes, rot + 2)
    ab.put([np.full(n, np.nan) for n in sizes] if first_nan else b)
    clip = None
    if coef is not None:
        clip = torch.tensor([5.0, coef, 1.0, 0.0, 0.0], device=DEV)
    what = f"mt_sgd chunk={chunk} rot={rot} {variant}"

    def launch(first, cl):
        L.mt_sgd(ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), ab.ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                 tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, chunk, momentum, nesterov, first, cl.data_ptr() if cl is not None else None, st)
        torch.cuda.synchronize()
        for a in (ap, ag, ab):
            a.check_gaps(what)

    for step in range(3):
        g = rand_list(sizes, rng)
        ag.put(g)
        first = int(first_nan and step == 0)
        launch(first, clip)
        new = [S.sgd_f32(p[t], g[t], b[t], tb.lr_h[t], tb.wd_h[t], momentum, nesterov, first, 1.0 if coef is None else coef)
               for t in range(len(sizes))]
        p, b = [x[0] for x in new], [x[1] for x in new]
        same_bits(ap.get(), p, f"{what} step {step} p")
        same_bits(ab.get(), b, f"{what} step {step} momentum buffer")
        same_bits(ag.get(), g, f"{what} step {step}: the gradients must not change")
    # a skipped step (finite flag 0) leaves p and the buffer as they are
    launch(0, torch.tensor([float("nan"), float("nan"), 0.0, 3.0, 1.0], device=DEV))
    same_bits(ap.get(), p, f"{what} skipped step p")
    same_bits(ab.get(), b, f"{what} skipped step momentum buffer")


# ---- mt_adamw --------------------------------------------------------------------------------------------------------------------------


def _adamw_step_check(what, pre, post, g, tb, hp, bc1, bc2s, coef):
    """one applied step: bit equality with adamw_f32 and the float64 bound of adamw_bound, from the device's own pre-step state"""
    b1, b2, eps = hp
    worst = 0.0
    for t in range(len(g)):
        args = (pre[0][t], g[t], pre[1][t], pre[2][t], tb.lr_h[t], tb.wd_h[t], b1, b2, eps, bc1, bc2s, coef)
        ref = S.adamw_f64(*args)
        tol = S.adamw_bound(*args)
        for k, name in enumerate(("p", "m", "v")):
            err = np.abs(post[k][t].astype(np.float64) - ref[k])
            assert (err <= tol[k]).all(), f"{what} tensor {t} {name}: {float((err / tol[k]).max()):.3g} x the float64 bound"
            worst = max(worst, float((err / tol[k]).max()))
    want = [S.adamw_f32(pre[0][t], g[t], pre[1][t], pre[2][t], tb.lr_h[t], tb.wd_h[t], b1, b2, eps, bc1, bc2s, coef) for t in range(len(g))]
    for k, name in enumerate(("p", "m", "v")):
        same_bits(post[k], [w[k] for w in want], f"{what} {name}")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rot", [(256, 0), (256, 3), (16384, 1)], ids=["chunk256-rot0", "chunk256-rot3", "chunk16384-rot1"])
def test_adamw_float64_bound_and_bit_for_bit(chunk, rot):
    """applied, skipped (NaN gradient), applied, applied with the clip pointer: the bias corrections follow the device's count of
    APPLIED steps (t = 1, -, 2, 3) and the skipped step leaves p, m, v as they are; then the clip-pointer-null form with the host's
    bias corrections.

    The assertion against float64 (u = 2^-24, one step from the device's own fp32 state; stem_optim_ref.adamw_bound): m within
    u|m'| + 4u (1-beta1)(|g c| + |m|); v within 6u v' (all terms positive); the update term T = lr/bc1 * m' / (sqrt(v')/bc2s + eps)
    carries about ten roundings - 6u on the denominator, one each for the division, lr/bc1 and the product, and m's own - so
    9u|T| + lr/bc1 / denom * tol_m; the decayed parameter p (1 - lr wd) 3u|p| and the final difference u|p'|; all times (1 + 2^-10).
    Bit equality with adamw_f32 is asserted on top: fp32 division and sqrtf are correctly rounded in this build.  Measured on the
    device: bit-identical on every element; the largest distance from float64 is 0.78 of the bound."""
    L, st = y3d.lib(), ops.stream()
    sizes = SIZES[chunk]
    rng = np.random.default_rng(chunk + rot + 23)
    tb = Tables(sizes, chunk)
    hp = (0.9, 0.999, 1e-8)
    ap, ag, am, av = (Arena(sizes, rot + i) for i in range(4))
    ap.put(rand_list(sizes, rng))
    am.put([np.zeros(n) for n in sizes])
    av.put([np.zeros(n) for n in sizes])
    _, out = guarded_out(5)
    what = f"mt_adamw chunk={chunk} rot={rot}"

    def launch(cl, bc1, bc2s):
        L.mt_adamw(ap.ptrs.data_ptr(), ag.ptrs.data_ptr(), am.ptrs.data_ptr(), av.ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(),
                   tb.wd.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), tb.n, chunk, *hp, bc1, bc2s, cl, st)
        torch.cuda.synchronize()
        for a in (ap, ag, am, av):
            a.check_gaps(what)

    worst, t_applied = 0.0, 0
    for step, skip in enumerate((False, True, False, False)):
        g = rand_list(sizes, rng, 0.5)
        if step == 3:
            g[2][:] = 0  # zero gradients on a tensor with m, v != 0
        if skip:
            g[-1][3] = np.nan  # the tail of the last tensor's first chunk
        ag.put(g)
        pre = (ap.get(), am.get(), av.get())
        sqnorm_clip(ag, tb, 2.0 if step == 2 else float("inf"), out)
        o = out.cpu().numpy()
        launch(out.data_ptr(), 0.5, 0.5)  # the host's bias corrections are placeholders when the clip pointer is given
        post = (ap.get(), am.get(), av.get())
        if skip:
            assert o[2] == 0
            for k, name in enumerate(("p", "m", "v")):
                same_bits(post[k], pre[k], f"{what} skipped step {name}")
            continue
        t_applied += 1
        assert o[2] == 1 and o[3] == t_applied
        assert (o[1] < 1) == (step == 2), "step 2 is clipped, the others are not"
        bc1, bc2s = S.bias_corrections(hp[0], hp[1], t_applied)
        worst = max(worst, _adamw_step_check(f"{what} step {step} (t = {t_applied})", pre, post, g, tb, hp, bc1, bc2s, o[1]))
    # clip pointer null: the host's bias corrections, coefficient 1, no skip rule
    g = rand_list(sizes, rng, 0.5)
    ag.put(g)
    pre = (ap.get(), am.get(), av.get())
    bc1, bc2s = S.bias_corrections(hp[0], hp[1], 7)
    launch(None, float(bc1), float(bc2s))
    worst = max(worst, _adamw_step_check(f"{what} null clip", pre, (ap.get(), am.get(), av.get()), g, tb, hp, bc1, bc2s, 1.0))
    print(f"{what}: largest error {worst:.3g} x the float64 bound")
    for bad in (0.0, -0.1):
        with pytest.raises(Y3DError):
            launch(None, bad, 0.5)
    with pytest.raises(Y3DError):
        launch(None, 0.5, 0.0)


# ---- mt_ema ----------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,rot", [(256, 0), (256, 2), (16384, 3)], ids=["chunk256-rot0", "chunk256-rot2", "chunk16384-rot3"])
def test_ema_bit_for_bit_and_guard(chunk, rot):
    L, st = y3d.lib(), ops.stream()
    sizes = SIZES[chunk]
    rng = np.random.default_rng(chunk + rot + 31)
    tb = Tables(sizes, chunk)
    reps_h = [1 + (t + rot) % 3 for t in range(len(sizes))]
    reps = torch.tensor(reps_h, dtype=torch.int32, device=DEV)
    e, m = rand_list(sizes, rng), rand_list(sizes, rng)
    ae, am = Arena(sizes, rot).put(e), Arena(sizes, rot + 1).put(m)
    d = 0.9999 * (1 - math.exp(-3 / 2000))
    what = f"mt_ema chunk={chunk} rot={rot}"

    def launch(guard):
        L.mt_ema(ae.ptrs.data_ptr(), am.ptrs.data_ptr(), tb.sizes.data_ptr(), reps.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), tb.n,
                 chunk, d, 1 - d, guard.data_ptr() if guard is not None else None, st)
        torch.cuda.synchronize()
        ae.check_gaps(what), am.check_gaps(what)

    for guard, applied in ((None, True), (torch.tensor([1.0, 1.0, 1.0, 1.0, 0.0], device=DEV), True),
                           (torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0], device=DEV), False), (None, True)):
        launch(guard)
        if applied:
            e = [S.ema_f32(e[t], m[t], d, 1 - d, reps_h[t]) for t in range(len(sizes))]
        same_bits(ae.get(), e, f"{what} guard={'null' if guard is None else guard.tolist()}")
        same_bits(am.get(), m, f"{what}: the model tensors must not change")


# ---- mt_copy ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("rots", [(0, 0), (1, 1), (0, 1), (1, 0), (2, 3)], ids=lambda r: f"src{r[0]}-dst{r[1]}")
@pytest.mark.parametrize("chunk", [256, 16384])
def test_copy_bit_for_bit(chunk, rots):
    """src / dst starts rotate independently: both 16-byte aligned (vector loop + scalar tail), both unaligned, and one of each"""
    L, st = y3d.lib(), ops.stream()
    sizes = SIZES[chunk]
    rng = np.random.default_rng(chunk + 5 * rots[0] + rots[1])
    tb = Tables(sizes, chunk)
    src = rand_list(sizes, rng)
    for s in src:
        s[::7] = -0.0
    asrc = Arena(sizes, rots[0]).put(src)
    al = [(a[0] % 4 == 0, b[0] % 4 == 0) for a, b in zip(asrc.spans, Arena(sizes, rots[1]).spans)]
    if rots == (0, 0):
        assert (True, True) in al
    if rots[0] != rots[1]:
        assert (True, False) in al and (False, True) in al
    for scale in (1.0, 0.5, 1.0 / 3.0):
        adst = Arena(sizes, rots[1])
        L.mt_copy(asrc.ptrs.data_ptr(), adst.ptrs.data_ptr(), *tb.tail, scale, st)
        torch.cuda.synchronize()
        what = f"mt_copy chunk={chunk} rots={rots} scale={scale}"
        adst.check_gaps(what), asrc.check_gaps(what)
        same_bits(adst.get(), src if scale == 1.0 else [S.copy_f32(s, scale) for s in src], what)
        same_bits(asrc.get(), src, what + ": the source must not change")


# ---- rejected arguments ----------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_optimizer_rejected_arguments():
    L, st = y3d.lib(), ops.stream()
    sizes = [300, 5]
    tb = Tables(sizes, 256)
    a = [Arena(sizes, i).put([np.ones(n) for n in sizes]) for i in range(4)]
    reps = torch.ones(2, dtype=torch.int32, device=DEV)
    pbuf = R.sentinel((64,), torch.float32, DEV)
    for n, chunk in ((0, 256), (tb.n, 255), (-1, 256), (tb.n, 0)):
        tail = (tb.sizes.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), n, chunk)
        with pytest.raises(Y3DError):
            L.mt_sqnorm(a[1].ptrs.data_ptr(), *tail, pbuf.data_ptr(), st)
        with pytest.raises(Y3DError):
            L.mt_copy(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), *tail, 1.0, st)
        with pytest.raises(Y3DError):
            L.mt_sgd(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), a[2].ptrs.data_ptr(), tb.sizes.data_ptr(), tb.lr.data_ptr(), tb.wd.data_ptr(),
                     tb.ct.data_ptr(), tb.co.data_ptr(), n, chunk, 0.9, 1, 0, None, st)
        with pytest.raises(Y3DError):
            L.mt_adamw(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), a[2].ptrs.data_ptr(), a[3].ptrs.data_ptr(), tb.sizes.data_ptr(),
                       tb.lr.data_ptr(), tb.wd.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), n, chunk, 0.9, 0.999, 1e-8, 0.1, 0.1, None, st)
        with pytest.raises(Y3DError):
            L.mt_ema(a[0].ptrs.data_ptr(), a[1].ptrs.data_ptr(), tb.sizes.data_ptr(), reps.data_ptr(), tb.ct.data_ptr(), tb.co.data_ptr(), n,
                     chunk, 0.9, 0.1, None, st)
    torch.cuda.synchronize()
    for x in a:
        same_bits(x.get(), [np.ones(n) for n in sizes], "a rejected call changed a tensor")
    assert bool(R.untouched(pbuf).all())


# ---- FusedSGD / FusedAdamW: checkpoint and resume -------------------------------------------------------------------------------------


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in ((16385,), (33, 7), (5,), (20000,), (64, 3, 3, 3))]


def _make(kind, ps):
    from yolov10_3d_amd.optim import FusedAdamW, FusedSGD
    groups = [{"params": ps[:2], "weight_decay": 5e-4}, {"params": ps[2:], "weight_decay": 0.0, "lr": 0.02}]
    if kind == "sgd":
        return FusedSGD(groups, lr=0.01, momentum=0.937, nesterov=True)
    return FusedAdamW(groups, lr=0.002, betas=(0.9, 0.999), weight_decay=0.0)


def _set_grads(ps, seed, nan=False):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    if nan:
        ps[1].grad[2, 3] = float("nan")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_fused_optimizer_state_dict_round_trip_bit_for_bit(kind):
    """3 steps (the second skipped by a NaN gradient), then state_dict() -> load_state_dict() of a fresh optimizer over cloned
    parameters, once before that optimizer's first step and once after it (its tables exist, its own state is overwritten and its
    parameters are set back); two more steps leave parameters, state buffers and counters bit-identical to the original's"""
    ps = _params(1)
    opt = _make(kind, ps)
    for s in range(3):
        _set_grads(ps, 10 + s, nan=(s == 1))
        opt.step(max_norm=5.0)
    torch.cuda.synchronize()
    assert opt.last_norm.tolist()[3:] == [2.0, 1.0]
    sd = opt.state_dict()
    clones = []
    for after_first_step in (False, True):
        qs = [p.detach().clone().requires_grad_(True) for p in ps]
        o2 = _make(kind, qs)
        if after_first_step:
            _set_grads(qs, 99)
            o2.step(max_norm=5.0)
            with torch.no_grad():
                for q, p in zip(qs, ps):
                    q.copy_(p)
        o2.load_state_dict(sd)
        clones.append((qs, o2))
    for s in range(2):
        for params, o in [(ps, opt)] + clones:
            _set_grads(params, 20 + s)
            o.step(max_norm=5.0)
    torch.cuda.synchronize()
    ref = opt.state_dict()
    assert ref["norm_clip"].tolist()[3:] == [4.0, 1.0]
    for i, (qs, o2) in enumerate(clones):
        tag = f"{kind} resumed {'after' if i else 'before'} the first step"
        for t, (q, p) in enumerate(zip(qs, ps)):
            assert_bits(q.detach(), p.detach(), f"{tag}: parameter {t}")
        got = o2.state_dict()
        assert got["steps"] == ref["steps"]
        assert_bits(got["flat"], ref["flat"], f"{tag}: flat state")
        assert_bits(got["norm_clip"], ref["norm_clip"], f"{tag}: norm_clip")
