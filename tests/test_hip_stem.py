"""The stem kernels through the C ABI against the host references of stem_optim_ref.py: y3d_stem_conv_train (+ _rows),
y3d_stem_conv_eval (csrc/stem_fused.hip), y3d_stem_im2col and y3d_stem_im2col_u8 (csrc/misc.hip).

* the column tensor is held to BIT equality with rne_bf16(stem_columns(image)) in all three input modes (fp32 images with negative
  values, values above 1 and exact bf16 ties in both directions: a truncating conversion fails; uint8 images with all 256 byte
  values: the on-device / 255 is the host's fp32 division for every byte);
* the raw conv output y is held to BIT equality: integer operands (the accumulator is an exact integer below 2^24, so y is its one
  RNE rounding; at least 25 % of the accumulators exceed 256 and some are exact ties, asserted) and one-hot weights (channel c sees
  +-2^(c mod 3) times column c mod 27, so every tap, input channel and output channel must land where the layout says);
* BatchNorm partials: y3d_stem_conv_train_rows rows, rows of idle waves exactly 0; folded in fp64, Sum y is exact (integers, each
  row's Sum |y| < 2^24, asserted) and Sum y^2, a sum of n exact squares in fp32 in any order, is within (n_max - 1) 2^-24 (1 + 2^-10)
  Sum y^2 + the fp64 fold, n_max = ceil(items / waves) * 64 pixels per wave.  The statistics of the UNROUNDED accumulators miss that
  bound (asserted): a kernel that sums the accumulator fails;
* eval: act = 0 with power-of-two scales and integer shifts is exact (bit equality); act = 1 is held to `bound` of
  test_hip_eval_epilogues.py on exact integer accumulators (its derivation: one bf16 rounding + the fp32 epilogue arithmetic);
* placement: y is a channel slot of a wider sentinel-filled buffer (ysw > Cout), xcol and part have guard space behind them; every
  element outside the written region keeps the sentinel and every element inside was written.
tests/test_stem_optim_ref_host.py pins the references and shows from STEM_CASES + BIG_CASE that every path of the kernel is reached."""
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops
from yolov10_3d_amd._lib import BF16, F32, Y3DError

import stem_optim_ref as S
import tail_ref as R
from test_hip_eval_epilogues import bound
from test_hip_eval_tail import assert_bits, check_guard, guarded
from test_hip_train_convs import _is_tie

DEV = "cuda"
OFF, EXTRA = 8, 24  # y slot: channels [OFF, OFF + Cout) of a buffer with Cout + EXTRA channels (pitch % 8 == 0, slot 16-byte aligned)
COUTS = [16, 32, 48, 64, 80]
# (B, H, W): H in {1, 2, 4, 5, 7} x W in {1, 2, 31, 127, 128, 129, 255, 256, 257}; what each reaches is asserted on the CPU
STEM_CASES = [(2, 1, 1), (1, 2, 2), (2, 5, 2), (3, 4, 31), (1, 1, 128), (2, 5, 127), (2, 4, 128), (2, 7, 129), (1, 5, 255), (2, 4, 256),
              (2, 2, 257), (1, 7, 257)]
BIG_CASE = (33, 128, 512)  # 33 * 64 * 4 = 8448 items > 8192 waves: the grid-stride loop gives 256 waves a second item
IDS = ["x".join(map(str, c)) for c in STEM_CASES]


# ---- operands (CPU generators: the host test checks their properties without a device) -----------------------------------------------


def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def int_operands(B, H, W, Cout, seed, device="cpu"):
    """non-negative integer image (0..63), integer weights (-15..15) + 6: 27 * 63 * 21 < 2^24, accumulators in the thousands"""
    g = _gen(seed, device)
    img = torch.randint(0, 64, (B, 3, H, W), generator=g, device=device).float()
    w = torch.zeros(Cout, 32, device=device)
    w[:, :27] = (torch.randint(-15, 16, (Cout, 27), generator=g, device=device) + 6).float()
    return img, w


def int_case(case, Cout):
    """(img, w, columns, exact accumulators) of the integer case: the first seed whose REFERENCE meets check_int_reference (the
    one-pixel maps have 16 outputs: not every draw holds a tie)"""
    B, H, W = case
    for k in range(64):
        img, w = int_operands(B, H, W, Cout, seed=sum(case) + Cout + 1000 * k)
        cols = S.stem_columns(img, 0)
        acc = S.stem_conv(cols, w)
        if float((acc.abs() > 256).double().mean()) >= 0.25 and bool(_is_tie(acc).any()) and \
                stats_distinguishable(S.rne_bf16(acc.float()).double(), acc, S.stem_path(B, H, W)["n_max"]):
            return img, w, cols, acc
    raise AssertionError(f"{case} Cout={Cout}: no seed gives an integer case that tests the rounding")


def small_int_operands(B, H, W, Cout, seed):
    """image 0..3, weights -2..2: accumulators of a few tens, so that random scales put u = acc * scale + shift where SiLU bends"""
    g = _gen(seed)
    img = torch.randint(0, 4, (B, 3, H, W), generator=g).float()
    w = torch.zeros(Cout, 32)
    w[:, :27] = torch.randint(-2, 3, (Cout, 27), generator=g).float()
    return img, w


TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)]  # round to 1 (down, even) and 1 + 2^-6 (up, even)


def real_image(B, H, W, seed):
    """fp32 image with negative values, values above 1 and exact bf16 ties in both directions"""
    img = torch.randn(B, 3, H, W, generator=_gen(seed)) * 1.5
    flat = img.view(-1)
    n = min(4, flat.numel())
    flat[:n] = torch.tensor(TIES[:n])
    return img


def u8_image(B, H, W, hwc, seed):
    """random bytes; images of 256 samples or more carry every byte value once more (planted run)"""
    g = _gen(seed)
    shape = (B, H, W, 3) if hwc else (B, 3, H, W)
    img = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    flat = img.view(-1)
    if flat.numel() >= 256:
        o = int(torch.randint(0, flat.numel() - 255, (1,), generator=g))
        flat[o:o + 256] = torch.arange(256, dtype=torch.int64)[torch.randperm(256, generator=g)].to(torch.uint8)
    return img


def onehot_w(Cout):
    w = torch.zeros(Cout, 32)
    for c in range(Cout):
        w[c, c % 27] = (-1.0) ** c * 2.0 ** (c % 3)
    return w


def _canon(t):
    """fp32 copy with -0 folded into +0 (a zero may carry either sign)"""
    return t.float() + 0.0


def _bf16(x):
    """float32 values that are bf16-representable -> bf16 storage (exact)"""
    return x.to(torch.bfloat16)


# ---- launches -------------------------------------------------------------------------------------------------------------------------


def _y_slot(B, Ho, Wo, Cout):
    buf = R.sentinel((B, Ho, Wo, Cout + EXTRA), torch.bfloat16, DEV)
    return buf, buf[..., OFF:OFF + Cout]


def _check_slot(buf, y, Cout, what):
    assert bool(R.untouched(buf[..., :OFF]).all()) and bool(R.untouched(buf[..., OFF + Cout:]).all()), f"{what}: a store left the y slot"
    assert not bool(R.untouched(y).any()), f"{what}: {int(R.untouched(y).sum())} elements of y were never written"


def run_train(img, in_mode, wcol, B, H, W, Cout):
    """y3d_stem_conv_train into sentinel-filled buffers -> (y (B, Ho, Wo, Cout) bf16, xcol (B, Ho, Wo, 32) bf16, part (rows, Cout, 2))"""
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    what = f"stem_conv_train {(B, H, W)} Cout={Cout} in_mode={in_mode}"
    ybuf, y = _y_slot(B, Ho, Wo, Cout)
    xbuf, xcol = guarded((B, Ho, Wo, 32), torch.bfloat16)
    rows = L.stem_conv_train_rows(B, H, W)
    pbuf, part = guarded((rows, Cout, 2), torch.float32)
    L.stem_conv_train(img.data_ptr(), in_mode, wcol.data_ptr(), y.data_ptr(), ybuf.stride(2), xcol.data_ptr(), part.data_ptr(), B, H, W,
                      Cout, st)
    torch.cuda.synchronize()
    _check_slot(ybuf, y, Cout, what)
    check_guard(xbuf, xcol, what + " xcol")
    check_guard(pbuf, part, what + " part")
    return y.contiguous(), xcol, part


def run_eval(img, in_mode, wcol, scale, shift, act, B, H, W, Cout):
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    ybuf, y = _y_slot(B, Ho, Wo, Cout)
    L.stem_conv_eval(img.data_ptr(), in_mode, wcol.data_ptr(), scale.data_ptr(), shift.data_ptr(), act, y.data_ptr(), ybuf.stride(2),
                     B, H, W, Cout, st)
    torch.cuda.synchronize()
    _check_slot(ybuf, y, Cout, f"stem_conv_eval {(B, H, W)} Cout={Cout} in_mode={in_mode} act={act}")
    return y.contiguous()


def check_int_reference(acc, tag):
    """the three conditions that make the integer case a test of the store's rounding"""
    assert float(acc.abs().max()) < 2 ** 24, f"{tag}: accumulators not exact in fp32"
    frac = float((acc.abs() > 256).double().mean())
    assert frac >= 0.25, f"{tag}: only {frac:.0%} of the accumulators exceed 256 - the store is barely rounding"
    assert bool(_is_tie(acc).any()), f"{tag}: no exact bf16 tie among the accumulators"


def check_partials(part, y, acc, B, H, W, tag):
    """part (rows, Cout, 2) against the stored y (module docstring); acc: the exact accumulators"""
    p = S.stem_path(B, H, W)
    assert part.shape[0] == p["rows"], f"{tag}: y3d_stem_conv_train_rows gives {part.shape[0]}, the restated grid {p['rows']}"
    idle = torch.from_numpy(p["per_wave"] == 0).to(part.device)
    assert bool((R.bits(part[idle]) == 0).all()), f"{tag}: the rows of waves without an item must be exactly 0"
    ys = y.double()
    n = p["n_max"]
    assert n * float(ys.abs().max()) < 2 ** 24, f"{tag}: a partial row's sum |y| may not be exact in fp32"
    pd = part.double()
    s1, s2 = pd[:, :, 0].sum(0), pd[:, :, 1].sum(0)
    r1, r2 = ys.sum((0, 1, 2)), (ys * ys).sum((0, 1, 2))
    assert bool((s1 == r1).all()), f"{tag}: Sum y differs from the sum of the stored y: {(s1 - r1).abs().max().item()}"
    tol = (n - 1) * 2.0 ** -24 * (1 + 2.0 ** -10) * r2 + 2.0 ** -40 * r2
    err = (s2 - r2).abs()
    assert bool((err <= tol).all()), f"{tag}: Sum y^2 off by {float((err / r2.clamp_min(1)).max()):.3g} relative (n_max {n})"
    assert stats_distinguishable(ys, acc.to(ys.device), n), f"{tag}: accumulator and stored statistics indistinguishable"


def stats_distinguishable(ys, acc, n):
    """True when Sum / Sum of squares of the exact accumulators miss the bound that the stored values' statistics are held to"""
    r1, r2 = ys.sum((0, 1, 2)), (ys * ys).sum((0, 1, 2))
    tol = (n - 1) * 2.0 ** -24 * (1 + 2.0 ** -10) * r2 + 2.0 ** -40 * r2
    gap1 = (acc.sum((0, 1, 2)) - r1).abs()
    gap2 = ((acc * acc).sum((0, 1, 2)) - r2).abs()
    return bool((gap1 > 0).any()) and bool((gap2 > tol).any())


# ---- y3d_stem_conv_train ---------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=IDS)
def test_stem_train_fp32_columns_bit_for_bit(case):
    """fp32 image with negatives, values above 1 and bf16 ties: xcol == rne_bf16(stem_columns), every Cout"""
    B, H, W = case
    img = real_image(B, H, W, seed=sum(case))
    want = _bf16(S.rne_bf16(S.stem_columns(img, 0)))
    imgd = img.to(DEV)
    for Cout in COUTS:
        _, w = int_operands(B, H, W, Cout, 1)
        _, xcol, _ = run_train(imgd, 0, w.to(DEV), B, H, W, Cout)
        assert_bits(xcol, want, f"stem_conv_train {case} Cout={Cout} fp32 xcol")


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=IDS)
def test_stem_train_integer_case_bit_for_bit(case):
    """fp32 mode, integer operands: y == RNE(exact accumulator), xcol exact, BatchNorm partials of the stored y"""
    B, H, W = case
    for Cout in COUTS:
        tag = f"stem_conv_train int {case} Cout={Cout}"
        img, w, cols, acc = int_case(case, Cout)
        check_int_reference(acc, tag)
        y, xcol, part = run_train(img.to(DEV), 0, w.to(DEV), B, H, W, Cout)
        assert_bits(xcol, _bf16(cols), tag + " xcol")
        assert_bits(_canon(y), _canon(_bf16(S.rne_bf16(acc.float()))), tag + " y")
        check_partials(part, y, acc, B, H, W, tag)


@pytest.mark.gpu
@pytest.mark.parametrize("in_mode", [1, 2])
@pytest.mark.parametrize("case", STEM_CASES, ids=IDS)
def test_stem_train_uint8_one_hot_bit_for_bit(case, in_mode):
    """uint8 NCHW / NHWC, all byte values: xcol == rne_bf16(byte / 255); one-hot weights: y[c] == +-2^(c mod 3) * xcol[c mod 27]"""
    B, H, W = case
    img = u8_image(B, H, W, in_mode == 2, seed=sum(case) + in_mode)
    cols = S.rne_bf16(S.stem_columns(img, in_mode))
    imgd = img.to(DEV)
    for Cout in COUTS:
        tag = f"stem_conv_train one-hot {case} Cout={Cout} in_mode={in_mode}"
        w = onehot_w(Cout)
        y, xcol, part = run_train(imgd, in_mode, w.to(DEV), B, H, W, Cout)
        assert_bits(xcol, _bf16(cols), tag + " xcol")
        c = torch.arange(Cout)
        want = cols[..., c % 27] * w[c, c % 27]  # a bf16 value times a power of two: exact
        assert_bits(_canon(y), _canon(_bf16(want)), tag + " y")
        assert not bool(part.isnan().any()), tag + ": NaN in the partials"


@pytest.mark.gpu
@pytest.mark.parametrize("in_mode", [0, 2])
def test_stem_train_grid_stride_loop(in_mode):
    """B = 33, 128 x 512: 8448 items on 8192 waves, so 256 waves take a second item; reference in float64 on the device"""
    B, H, W = BIG_CASE
    Cout = 32 if in_mode == 0 else 48
    tag = f"stem_conv_train {BIG_CASE} Cout={Cout} in_mode={in_mode}"
    if in_mode == 0:
        img, w = int_operands(B, H, W, Cout, 5, device=DEV)
    else:
        img, w = u8_image(B, H, W, True, 6).to(DEV), onehot_w(Cout).to(DEV)
    cols = S.stem_columns(img, in_mode)
    y, xcol, part = run_train(img, in_mode, w, B, H, W, Cout)
    assert_bits(xcol, _bf16(S.rne_bf16(cols)), tag + " xcol")
    acc = S.stem_conv(cols, w)
    if in_mode == 0:
        check_int_reference(acc, tag)
        check_partials(part, y, acc, B, H, W, tag)
    assert_bits(_canon(y), _canon(_bf16(S.rne_bf16(acc.float()))), tag + " y")


# ---- y3d_stem_conv_eval ----------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("case", STEM_CASES, ids=IDS)
def test_stem_eval_exact_affine_and_identity(case):
    """act = 0, scale in {1/2, 1, 2}, integer shift on the integer case: u = acc * scale + shift is exact in fp32, y its one rounding;
    identity scale and zero shift give the train y bit for bit"""
    B, H, W = case
    for Cout in COUTS:
        tag = f"stem_conv_eval int {case} Cout={Cout}"
        g = _gen(Cout + sum(case))
        img, w, _, acc = int_case(case, Cout)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=g)]
        shift = torch.randint(-50, 51, (Cout,), generator=g).float()
        u = acc * scale.double() + shift.double()
        assert float(u.abs().max()) < 2 ** 24
        imgd, wd = img.to(DEV), w.to(DEV)
        y = run_eval(imgd, 0, wd, scale.to(DEV), shift.to(DEV), 0, B, H, W, Cout)
        assert_bits(_canon(y), _canon(_bf16(S.rne_bf16(u.float()))), tag + " act=0")
        ye = run_eval(imgd, 0, wd, torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV), 0, B, H, W, Cout)
        yt, _, _ = run_train(imgd, 0, wd, B, H, W, Cout)
        assert_bits(ye, yt, tag + " identity epilogue vs train y")


@pytest.mark.gpu
@pytest.mark.parametrize("in_mode", [0, 1, 2])
@pytest.mark.parametrize("case", STEM_CASES, ids=IDS)
def test_stem_eval_silu_within_the_epilogue_bound(case, in_mode):
    """act = 1, random scale / shift, against float64 from the bf16-rounded operands.  fp32 mode: small integers, so the accumulator is
    exact and `bound` of test_hip_eval_epilogues.py (one bf16 rounding + the fp32 epilogue) applies as derived there.  uint8 modes:
    one-hot weights, the accumulator is +-2^k times one bf16 sample, exact as well"""
    B, H, W = case
    for Cout in COUTS:
        g = _gen(Cout + sum(case) + in_mode)
        if in_mode == 0:
            img, w = small_int_operands(B, H, W, Cout, seed=sum(case) + Cout)
            scale = 0.05 + 0.45 * torch.rand(Cout, generator=g)
        else:
            img, w = u8_image(B, H, W, in_mode == 2, seed=sum(case) + Cout), onehot_w(Cout) * 2
            scale = (0.05 + 1.95 * torch.rand(Cout, generator=g)) * torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
        shift = torch.randn(Cout, generator=g)
        acc = S.stem_conv(S.stem_columns(img, in_mode), w)
        prod = acc * scale.double()
        u = prod + shift.double()
        ref = u * torch.sigmoid(u)
        y = run_eval(img.to(DEV), in_mode, w.to(DEV), scale.to(DEV), shift.to(DEV), 1, B, H, W, Cout).double().cpu()
        tol = bound(BF16, ref, ref, torch.zeros_like(ref), u, prod, shift.double().expand_as(u))
        bad = ~((y - ref).abs() <= tol)
        assert not bool(bad.any()), (f"stem_conv_eval act=1 {case} Cout={Cout} in_mode={in_mode}: {int(bad.sum())} of {bad.numel()} outside "
                                     f"the bound, worst {float(((y - ref).abs() / tol).max()):.3g} x")


# ---- y3d_stem_im2col / y3d_stem_im2col_u8 ----------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [BF16, F32])
@pytest.mark.parametrize("case", STEM_CASES + [(3, 64, 160)], ids=IDS + ["3x64x160"])
def test_stem_im2col_bit_for_bit(case, dt):
    """the two-step form's column tensor: F32 == stem_columns, BF16 == rne_bf16(stem_columns); fp32 NCHW, uint8 NCHW, uint8 NHWC"""
    B, H, W = case
    L, st = y3d.lib(), ops.stream()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tdt = torch.bfloat16 if dt == BF16 else torch.float32
    for mode in (0, 1, 2):
        img = real_image(B, H, W, sum(case)) if mode == 0 else u8_image(B, H, W, mode == 2, sum(case) + mode)
        cols = S.stem_columns(img, mode)
        want = _bf16(S.rne_bf16(cols)) if dt == BF16 else cols
        imgd = img.to(DEV)
        buf, out = guarded((B, Ho, Wo, 32), tdt)
        if mode == 0:
            L.stem_im2col(dt, imgd.data_ptr(), out.data_ptr(), B, H, W, Ho, Wo, st)
        else:
            L.stem_im2col_u8(dt, imgd.data_ptr(), int(mode == 2), out.data_ptr(), B, H, W, Ho, Wo, st)
        torch.cuda.synchronize()
        what = f"stem_im2col{'_u8' if mode else ''} {case} dt={dt} mode={mode}"
        check_guard(buf, out, what)
        assert_bits(out, want, what)


# ---- rejected arguments ----------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_stem_rejected_arguments():
    """every buffer is large enough for Cout = 80, so no argument set below could write out of bounds; nothing may be written"""
    L, st = y3d.lib(), ops.stream()
    B, H, W = 2, 4, 31
    Ho, Wo = 2, 16
    img = torch.rand(B, 3, H, W, device=DEV)
    w = torch.zeros(96, 32, device=DEV)
    sc, sh = torch.ones(96, device=DEV), torch.zeros(96, device=DEV)
    ybuf = R.sentinel((B * Ho * Wo * 128 + 64,), torch.bfloat16, DEV)
    xbuf = R.sentinel((B * Ho * Wo * 32 + 64,), torch.bfloat16, DEV)
    pbuf = R.sentinel((L.stem_conv_train_rows(B, H, W) * 96 * 2,), torch.float32, DEV)
    cbuf = R.sentinel((B * 4 * 32 * 32,), torch.float32, DEV)
    y, x, p = ybuf.data_ptr(), xbuf.data_ptr(), pbuf.data_ptr()

    def train(in_mode=0, Cout=32, ysw=128, yp=y, xp=x):
        L.stem_conv_train(img.data_ptr(), in_mode, w.data_ptr(), yp, ysw, xp, p, B, H, W, Cout, st)

    def evl(in_mode=0, Cout=32, ysw=128, yp=y):
        L.stem_conv_eval(img.data_ptr(), in_mode, w.data_ptr(), sc.data_ptr(), sh.data_ptr(), 1, yp, ysw, B, H, W, Cout, st)

    bad = [dict(in_mode=3), dict(in_mode=-1), dict(Cout=8), dict(Cout=24), dict(Cout=96), dict(Cout=80, ysw=72), dict(Cout=32, ysw=36),
           dict(yp=y + 2), dict(yp=y + 8)]
    for kw in bad:
        for fn in (train, evl):
            with pytest.raises(Y3DError):
                fn(**kw)
    for xp in (x + 2, x + 8):
        with pytest.raises(Y3DError):
            train(xp=xp)
    u8 = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=DEV)
    for ho, wo in ((Ho + 1, Wo), (Ho, Wo - 1), (Ho, Wo + 1), (H, W)):
        for dt in (BF16, F32):
            with pytest.raises(Y3DError):
                L.stem_im2col(dt, img.data_ptr(), cbuf.data_ptr(), B, H, W, ho, wo, st)
            for hwc in (0, 1):
                with pytest.raises(Y3DError):
                    L.stem_im2col_u8(dt, u8.data_ptr(), hwc, cbuf.data_ptr(), B, H, W, ho, wo, st)
    with pytest.raises(Y3DError):
        L.stem_im2col(2, img.data_ptr(), cbuf.data_ptr(), B, H, W, Ho, Wo, st)
    torch.cuda.synchronize()
    for buf in (ybuf, xbuf, pbuf, cbuf):
        assert bool(R.untouched(buf).all()), "a rejected call wrote to an output"
    train(), evl()  # the defaults are a valid call: each rejection above is due to the one argument it changes
    torch.cuda.synchronize()
    assert bool(R.untouched(xbuf[B * Ho * Wo * 32:]).all())
