"""Case tables, deterministic generators and host references for the three kernels of csrc/post.hip that sit around the eval and
training hot path: y3d_kde_depth_fusion, y3d_kitti_image_aug and y3d_kitti_decode (kitti_row.h).  The references are
oracle/restate.py's (`kde_fuse_depth`, `box_iou_xyxy`, `kitti_image_aug`, `kitti_decode`) behind thin wrappers; `fusion_rows` adds,
per one-to-one row, what the near-maximiser rule of the fusion test needs.  Nothing here touches the device or the library.

tests/test_val_tail_ref_host.py pins the references against independent statements (Pillow, scikit-learn) and checks, from the
references alone, every condition tests/test_hip_val_tail.py relies on."""
import math

import numpy as np
import torch

from oracle import restate as RS

F32 = np.float32
THRES = float(F32(0.1))      # the validator's defaults as the float32 values the C ABI receives: the reference then compares
IOU_THRES = float(F32(0.9))  # against the same number, whichever precision torch compares a tensor with a scalar in
TAU_EQUAL = 1e-12            # equal weights: only double exp / log rounding differs (1e-15 relative on <= 301 positive terms)
TAU_MIXED = 1e-6             # mixed weights: <= 4 float32 ulps per weight (expf vs torch.exp, one division each side), the common
#                              1 / sum moves no arg-max: two log-densities shift against each other by <= 2 * 4 * 2^-24 = 4.8e-7


# ---------------------------------------------------------------------------------------------------------------- depth fusion
# name: (B, K, KM, nprop, family, C, tau, cap) - cap: the largest share of fused rows whose reference margin may be <= tau (None:
# the case exists for its ties)
FUSION_CASES = {
    "crowded-equal-500": (2, 4, 300, 500, "equal", 37, TAU_EQUAL, 0.0),
    "crowded-mixed-33": (2, 4, 300, 33, "mixed", 37, TAU_MIXED, 0.05),
    "crowded-mixed-64": (2, 4, 300, 64, "mixed", 37, TAU_MIXED, 0.05),
    "sparse-mixed-33": (3, 50, 300, 33, "mixed", 37, TAU_MIXED, 0.05),
    "nprop-2": (1, 5, 40, 2, "equal", 37, TAU_EQUAL, 0.0),
    "nprop-257": (1, 5, 40, 257, "equal", 37, TAU_EQUAL, 0.0),
    "nprop-500-small": (1, 5, 40, 500, "mixed", 37, TAU_MIXED, 0.0),
    "c8-mixed-33": (2, 4, 60, 33, "mixed", 8, TAU_MIXED, 0.05),
    "km1": (1, 5, 1, 33, "km1", 37, TAU_EQUAL, 0.0),
    "nomatch": (2, 4, 40, 33, "nomatch", 37, TAU_MIXED, 0.0),
    "own-excluded": (1, 3, 12, 33, "own-excluded", 37, TAU_MIXED, 0.05),
    "hi-eq-lo": (1, 3, 12, 33, "hi-eq-lo", 37, TAU_MIXED, 0.0),
    "tie2": (1, 2, 4, 33, "tie2", 37, TAU_EQUAL, None),
    "iou-boundary": (1, 3, 3, 33, "iou-boundary", 37, TAU_MIXED, 0.0),
    "thres-boundary": (1, 3, 6, 33, "thres-boundary", 37, TAU_MIXED, 0.0),
    "large-km": (1, 2, 3800, 33, "mixed", 37, TAU_MIXED, 0.05),
}
FUSION_THRES = {"thres-boundary": 1.0}  # everything else runs at THRES / IOU_THRES
FUSION_SEEDS = {"nprop-500-small": 2}   # chosen on the reference alone so that no margin of the case is under its tau
FUSION_KM_MAX = 3902                   # the largest KM y3d_kde_depth_fusion admits (16 * KM + 3088 + 16 bytes of LDS <= 64 KiB)


def fusion_thresholds(name):
    return FUSION_THRES.get(name, THRES), IOU_THRES


def _clear_of(u, thres, gen):
    """resample the log-variances whose exp(-u) sits within 1e-5 * thres of thres: expf and torch.exp may differ in the last bit
    there, so the reference does not define the vote"""
    for _ in range(100):
        bad = (torch.exp(-u.double()) - thres).abs() < 1e-5 * thres
        if not bool(bad.any()):
            return u
        u = torch.where(bad, torch.rand(u.shape, generator=gen) * 3.3, u)
    raise AssertionError("could not move the log-variances off the threshold")


def _base_rows(B, K, C, gen, mixed):
    """one-to-one rows: boxes 150 px apart and at most 80 px wide (a jittered copy overlaps its own source only), depth in 5..60,
    log-variance 0 or uniform in 0..3.3 (exp(-u) straddles 0.1 at u = 2.303), labels over three classes"""
    O = torch.randn(B, K, C, generator=gen)
    j = torch.arange(K)
    cx = 100.0 + 150.0 * (j % 8) + torch.rand(B, K, generator=gen) * 20
    cy = 100.0 + 150.0 * (j // 8) + torch.rand(B, K, generator=gen) * 20
    w, h = 40 + 40 * torch.rand(B, K, generator=gen), 30 + 30 * torch.rand(B, K, generator=gen)
    O[..., 0], O[..., 1], O[..., 2], O[..., 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    O[..., C - 4] = 5 + 55 * torch.rand(B, K, generator=gen)
    O[..., C - 3] = torch.rand(B, K, generator=gen) * 3.3 if mixed else 0.0
    O[..., C - 2] = torch.rand(B, K, generator=gen)
    O[..., C - 1] = torch.randint(0, 3, (B, K), generator=gen).float()
    return O


def _jittered(O, KM, gen, mixed, jit=0.045):
    """one-to-many rows: row m copies one-to-one row m % K, its box corners moved by up to `jit` of the box size each (IoU straddles
    0.9), its depth by a normal of 1.5, one label in five changed, log-variances as the family says"""
    B, K, C = O.shape
    src = torch.arange(KM) % K
    M = O[:, src].clone()
    M[..., 4:C - 4] = torch.randn(B, KM, C - 8, generator=gen)
    wh = torch.stack((M[..., 2] - M[..., 0], M[..., 3] - M[..., 1]), -1).repeat(1, 1, 2)
    M[..., :4] += (torch.rand(B, KM, 4, generator=gen) * 2 - 1) * jit * wh
    M[..., C - 4] += torch.randn(B, KM, generator=gen) * 1.5
    M[..., C - 3] = torch.rand(B, KM, generator=gen) * 3.3 if mixed else 0.0
    M[..., C - 2] = torch.rand(B, KM, generator=gen)
    change = torch.rand(B, KM, generator=gen) < 0.2
    M[..., C - 1] = torch.where(change, (M[..., C - 1] + 1) % 3, M[..., C - 1])
    return M


def fusion_inputs(name):
    """-> predsO (B, K, C), predsM (B, KM, C) float32 host tensors of the named case"""
    B, K, KM, nprop, fam, C, tau, cap = FUSION_CASES[name]
    gen = torch.Generator().manual_seed(FUSION_SEEDS.get(name, 1000 + sorted(FUSION_CASES).index(name)))
    thres, _ = fusion_thresholds(name)
    mixed = fam in ("mixed", "nomatch", "own-excluded", "thres-boundary")
    O = _base_rows(B, K, C, gen, mixed)
    if fam in ("equal", "mixed"):
        M = _jittered(O, KM, gen, mixed)
    elif fam == "km1":       # the only one-to-many row copies row 0 and votes, row 0's own vote is below the threshold: n = 1
        M = O[:, :1].clone()
        O[0, 0, C - 3] = 5.0
        O[0, 1, C - 3] = 5.0  # n = 0
    elif fam == "nomatch":   # jittered copies moved off their sources: no IoU above 0
        M = _jittered(O, KM, gen, True)
        M[..., 0] += 90.0
        M[..., 2] += 90.0
        O[0, 0, C - 3] = 5.0
    elif fam == "own-excluded":  # four exact copies of each box vote; the row's own depth is far outside them and must not count
        M = O[:, torch.arange(KM) % K].clone()
        M[..., C - 4] += torch.randn(B, KM, generator=gen) * 1.5
        M[..., C - 3] = torch.rand(B, KM, generator=gen) * 2.0
        O[..., C - 3] = 4.0
        O[..., C - 4] = 1000.0
    elif fam == "hi-eq-lo":  # every voter at the row's own depth, with different weights
        M = O[:, torch.arange(KM) % K].clone()
        M[..., C - 3] = torch.rand(B, KM, generator=gen) * 2.0
        O[..., C - 3] = torch.rand(B, K, generator=gen) * 2.0
    elif fam == "tie2":      # two voters of weight 1/2 each at 10 and 14: the 33 proposals are k / 8 apart and exact, the density
        #                      is symmetric about 12 and, 4 > 2 h apart, has two equal maxima; row 1 the same with its own vote out
        M = O[:, [0, 0, 1, 1]].clone()
        O[..., C - 3] = 0.0
        M[..., C - 3] = 0.0
        O[0, 0, C - 4], M[0, 0, C - 4], M[0, 1, C - 3] = 10.0, 14.0, 5.0
        O[0, 1, C - 3], M[0, 2, C - 4], M[0, 3, C - 4] = 5.0, 20.0, 24.0
    elif fam == "iou-boundary":
        # row 0: [0,0,10,10] against [0,0,10,9]: 90 / (100 + 90 - 90 + 1e-7) is float32(0.9) = iou_thres exactly: no vote, n = 1
        # row 1: against [0,0,10,9.5]: 0.95, votes, n = 2;  row 2: no partner
        # the one-to-many vote is the heavier one (two equal votes 3 apart would tie; a lighter one would leave the pick on the row's
        # own depth, and a boundary row that wrongly voted would not show)
        O[..., C - 3] = 1.0
        O[0, :, :4] = torch.tensor([[0.0, 0, 10, 10], [200.0, 0, 210, 10], [400.0, 0, 410, 10]])
        M = O.clone()
        M[0, :, :4] = torch.tensor([[0.0, 0, 10, 9], [200.0, 0, 210, 9.5], [800.0, 0, 810, 10]])
        M[..., C - 4] += 3.0
        M[..., C - 3] = 0.0
    elif fam == "thres-boundary":
        # thres = 1: u = 0 gives exp(-0) = 1, not above it.  row 0: own u = 0 and two copies with u = 0: n = 0; row 1: own u = 0, two
        # copies with u = -0.5: n = 2, own vote excluded; row 2: own u = -1, one copy u = 0, one u = -0.25: n = 2
        M = O[:, [0, 0, 1, 1, 2, 2]].clone()
        M[..., C - 4] += torch.randn(B, KM, generator=gen) * 1.5
        O[0, :, C - 3] = torch.tensor([0.0, 0.0, -1.0])
        M[0, :, C - 3] = torch.tensor([0.0, 0.0, -0.5, -0.5, 0.0, -0.25])
    else:
        raise KeyError(fam)
    if fam not in ("thres-boundary",):
        O[..., C - 3] = _clear_of(O[..., C - 3], thres, gen)
        M[..., C - 3] = _clear_of(M[..., C - 3], thres, gen)
    return O.contiguous(), M.contiguous()


def kde_fuse_depth(O, M, thres, iou_thres, nprop):
    return RS.kde_fuse_depth(O, M, thres, iou_thres, nprop)


def box_iou_xyxy(a, b):
    return RS.box_iou_xyxy(a, b)


def fusion_rows(O, M, thres, iou_thres, nprop):
    """per one-to-one row (b, j), in row order, a dict: `n` the reference's vote count, `own` whether the row's own vote counts,
    `lo`, `hi` float32 extreme votes, and for n > 1 `grid` (nprop,) the float32 proposals and `ld` (nprop,) the float64 log-density
    on them, `pick` the index of its first maximum, `margin` = ld[pick] - the best ld among proposals of another VALUE than the
    pick's (inf when every proposal has the pick's value).  The arithmetic is `oracle.restate.kde_fuse_depth`'s, statement by
    statement; the host test holds grid[pick] against that function's output."""
    B, K, C = O.shape
    rows = []
    for i in range(B):
        iou = box_iou_xyxy(O[i, :, :4], M[i, :, :4])
        for j in range(K):
            m = iou[j] > iou_thres
            d = torch.cat((O[i, j, C - 4:C - 3], M[i, m, C - 4]))
            u = torch.cat((O[i, j, C - 3:C - 2], M[i, m, C - 3]))
            c = torch.cat((O[i, j, C - 1:], M[i, m, C - 1]))
            s = torch.exp(-u)
            mask = (s > thres) & (c == O[i, j, C - 1])
            n = int(mask.sum())
            row = {"n": n, "own": bool(mask[0]), "matched": int(m.sum())}
            if n > 1:
                s, d = s[mask], d[mask]
                w = (s / s.sum()).numpy().astype(np.float64)
                x = d.numpy().astype(np.float64)
                h = (n * 3 / 4.0) ** (-1 / 5.0)
                lo, hi = F32(d.min()), F32(d.max())
                step = F32((hi - lo) / F32(nprop - 1))
                grid = (np.arange(nprop, dtype=F32) * step + lo).astype(F32)
                grid[-1] = hi
                pp = grid.astype(np.float64)
                ld = np.log((w[None, :] * np.exp(-0.5 * ((pp[:, None] - x[None, :]) / h) ** 2)).sum(1))
                pick = int(np.argmax(ld))
                other = ld[grid != grid[pick]]
                row.update(lo=lo, hi=hi, grid=grid, ld=ld, pick=pick, equal_weights=bool((s == s[0]).all()),
                           margin=float(ld[pick] - other.max()) if other.size else math.inf)
            rows.append(row)
    return rows


def fusion_stats(rows, tau):
    """-> (fused rows, rows with margin <= tau, smallest margin) of a case"""
    fused = [r for r in rows if r["n"] > 1]
    return len(fused), sum(r["margin"] <= tau for r in fused), min((r["margin"] for r in fused), default=math.inf)


def check_fusion(out, O, rows, tau, what):
    """the assertions of the fusion test on a fused tensor `out` (host), whoever made it:
    1. every column but the depth is predsO's, bit for bit;  2. rows with n <= 1 keep their depth bit for bit;
    3. a fused depth is bitwise one of the reference's float32 proposals;
    4. its reference log-density is within tau of the maximum, and where the reference's margin exceeds tau it is the reference's pick
    -> (the largest log-density gap of a fused row, the fused rows whose depth is not the reference's pick)"""
    B, K, C = O.shape
    ob, gb = O.contiguous().view(torch.int32), out.contiguous().view(torch.int32)
    assert out.shape == O.shape and out.dtype == torch.float32
    other = torch.ones(C, dtype=torch.bool)
    other[C - 4] = False
    ne = (ob[..., other] != gb[..., other]).any(-1)
    assert not bool(ne.any()), f"{what}: columns other than the depth changed in rows {ne.nonzero().tolist()[:8]}"
    worst, off_pick = 0.0, 0
    for idx, r in enumerate(rows):
        b, j = divmod(idx, K)
        got = out[b, j, C - 4].numpy()
        if r["n"] <= 1:
            assert int(gb[b, j, C - 4]) == int(ob[b, j, C - 4]), f"{what}: row {(b, j)} has {r['n']} votes but its depth moved to {got!r}"
            continue
        hit = (r["grid"].view(np.int32) == got.view(np.int32)).nonzero()[0]
        assert hit.size, (f"{what}: row {(b, j)} (n = {r['n']}): depth {got!r} is none of the {r['grid'].size} proposals between "
                          f"{r['lo']!r} and {r['hi']!r} (reference: {r['grid'][r['pick']]!r})")
        gap = float(r["ld"][r["pick"]] - r["ld"][hit[0]])
        assert gap <= tau, f"{what}: row {(b, j)} (n = {r['n']}): log-density at {got!r} is {gap:.3e} below the maximum (tau {tau:g})"
        if r["margin"] > tau:
            assert got.view(np.int32) == r["grid"][r["pick"]].view(np.int32), (
                f"{what}: row {(b, j)}: {got!r} instead of the reference's {r['grid'][r['pick']]!r} (margin {r['margin']:.3e})")
        worst, off_pick = max(worst, gap), off_pick + int(got.view(np.int32) != r["grid"][r["pick"]].view(np.int32))
    return worst, off_pick


# ---------------------------------------------------------------------------------------------------------------- image crop
# name: (source H, W, output (W, H), trans_inv (output -> source))
def _kitti_like():
    # the dataset's crop matrix for a 24 x 80 frame: crop centre off the middle, crop 0.9 of the frame, to 61 x 19
    _, tinv = RS.get_affine_transform(np.array([43.0, 11.0]), np.array([72.0, 21.6]), (61, 19), inv=True)
    return [float(v) for v in tinv.reshape(6)]


AUG_CASES = {
    "identity": (7, 9, (7, 9), [1, 0, 0, 0, 1, 0]),               # output rows 7, 8 and source columns 7, 8 have no counterpart
    "upscale-odd": (5, 6, (19, 13), [6 / 19, 0, 0, 0, 5 / 13, 0]),
    "downscale": (37, 53, (8, 5), [53 / 8, 0, 0, 0, 37 / 5, 0]),
    "shift-outside": (12, 10, (11, 9), [1, 0, -5.25, 0, 1, 7.5]),
    "half-pixel": (8, 9, (9, 7), [1, 0, -0.5, 0, 1, 0.5]),        # x - 0.5 < 0 at the left border: floor, not truncation
    "all-outside": (6, 7, (9, 5), [1, 0, 1000, 0, 1, 1000]),
    "shear-rotation": (11, 13, (13, 11), [0.8, 0.6, -3, -0.6, 0.8, 6]),
    "mirror-map": (9, 16, (17, 9), [-1, 0, 16, 0, 1, 0]),
    "src-1x1": (1, 1, (5, 3), [1 / 5, 0, 0, 0, 1 / 3, 0]),
    "src-one-row": (1, 8, (9, 3), [0.7, 0, 0.3, 0, 0.4, -0.1]),
    "src-one-column": (8, 1, (3, 9), [0.4, 0, -0.1, 0, 0.7, 0.3]),
    "kitti-like": (24, 80, (61, 19), _kitti_like()),
}
AUG_MIXED = ["shear-rotation", "half-pixel", "src-1x1", "upscale-odd", "mirror-map"]  # one batch: sizes, maps, flips, partners mixed
AUG_MIXED_FLIP = [1, 0, 1, 0, 1]
AUG_MIXED_PARTNER = [True, False, False, True, False]   # the partner table is there, these entries are NULL or not
AUG_MIXED_OUT = (13, 11)
AUG_BIG = (3, 16, 16, (384, 512))                       # B, source H, W, output (W, H): 589 824 pixels, above 2 048 * 256


def aug_sources(H, W, seed):
    """-> (image, partner) (H, W, 3) uint8 arrays with random content"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def blend_pair_sources():
    """src[y, x] = y, partner[y, x] = x on 256 x 256: under the identity map every blend pair (a, b) occurs"""
    y, x = np.mgrid[0:256, 0:256]
    return (np.repeat(y[..., None], 3, 2).astype(np.uint8).copy(), np.repeat(x[..., None], 3, 2).astype(np.uint8).copy())


def kitti_image_aug(img, img2, flip, trans_inv, out_wh):
    """-> (outH, outW, 3) uint8, the reference's crop"""
    return RS.kitti_image_aug(img, img2, bool(flip), np.asarray(trans_inv, np.float64), out_wh)


def aug_float(u8):
    """the reference's tensor of a crop: / 255 in float32, CHW"""
    return (u8.astype(F32) / F32(255)).transpose(2, 0, 1).copy()


def aug_reach(H, W, out_wh, trans_inv):
    """which branches of the crop the output pixels of a case reach, from the map alone: `outside` (source position outside the
    image), `neg` (x - 0.5 or y - 0.5 negative), `clamp_l/r/t` (a clamped neighbour at the left / right / top border), `no_row`
    (y + 1 is not a source row), `inner` (four distinct taps)"""
    t = np.asarray(trans_inv, np.float64).reshape(2, 3)
    ys, xs = np.mgrid[0:out_wh[1], 0:out_wh[0]]
    xin = t[0, 0] * (xs + 0.5) + t[0, 1] * (ys + 0.5) + t[0, 2]
    yin = t[1, 0] * (xs + 0.5) + t[1, 1] * (ys + 0.5) + t[1, 2]
    ins = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    x, y = np.floor(xin - 0.5).astype(int), np.floor(yin - 0.5).astype(int)
    return {"outside": bool((~ins).any()), "neg": bool((ins & ((xin < 0.5) | (yin < 0.5))).any()),
            "clamp_l": bool((ins & (x < 0)).any()), "clamp_r": bool((ins & (x + 1 >= W)).any()), "clamp_t": bool((ins & (y < 0)).any()),
            "no_row": bool((ins & (y + 1 >= H)).any()),
            "inner": bool((ins & (x >= 0) & (x + 1 < W) & (y >= 0) & (y + 1 < H)).any())}


# ---------------------------------------------------------------------------------------------------------------- KITTI decode
DECODE_SHAPES = [(5, 150), (1, 257)]   # B * K = 750: three blocks of 256 rows, the last one ragged; 257: one row into a second block
DECODE_THRESHOLD = 0.5                 # sigmoid(0) * exp(-0) exactly: both factors are exact on either side
DECODE_THRESHOLDS = [0.5, float(np.nextafter(0.5, 1.0)), float(np.nextafter(0.5, 0.0))]
DECODE_CLEAR = 1e-5                    # generated scores stay this far (relative) off every threshold: far more than the 2-3 float32
#                                        ulps (3e-7) expf may move a score by
PI_F = F32(math.pi)
BIN_W = F32(2 * math.pi / 12.0)
PLANTED = ["tie2-bin0", "tie3", "tie-10-11", "max-11", "ang-at-pi", "ang-above-pi", "ang-below-pi", "ry-plus", "ry-minus", "score-at-thr",
           "camdis-nan"]


def _res_for(bin_, target):
    """the float32 residual r with float32(bin * (2 pi / 12)) + r == target in float32"""
    base = F32(bin_) * BIN_W
    r = F32(target - base)
    for _ in range(8):
        got = F32(base + r)
        if got == target:
            return r
        r = np.nextafter(r, F32(np.inf) if got < target else F32(-np.inf))
    raise AssertionError("no residual reaches the target angle")


def decode_inputs(B, K):
    """-> preds (B, K, 37) float32, calib (B, 6), ratio (B, 2), inv_trans (B, 2, 3) float64 host tensors and {planted name: (b, k)}.
    Every image has its own calibration, ratio and inverse map, so a row decoded with another image's constants shows."""
    gen = torch.Generator().manual_seed(7000 + B * 1000 + K)
    P = torch.zeros(B, K, 37)
    x1, y1 = torch.rand(B, K, generator=gen) * 1100, torch.rand(B, K, generator=gen) * 300
    P[..., 0], P[..., 1] = x1, y1
    P[..., 2], P[..., 3] = x1 + 10 + torch.rand(B, K, generator=gen) * 150, y1 + 10 + torch.rand(B, K, generator=gen) * 80
    P[..., 4] = (P[..., 0] + P[..., 2]) / 2 + torch.randn(B, K, generator=gen) * 3
    P[..., 5] = (P[..., 1] + P[..., 3]) / 2 + torch.randn(B, K, generator=gen) * 3
    P[..., 6:9] = torch.randn(B, K, 3, generator=gen) * 0.3
    P[..., 9:21] = torch.randn(B, K, 12, generator=gen) * 2
    P[..., 21:33] = torch.rand(B, K, 12, generator=gen) * 0.5 - 0.25
    P[..., 33] = 2 + torch.rand(B, K, generator=gen) * 58
    P[..., 34] = torch.rand(B, K, generator=gen) * 3 - 1
    P[..., 35] = torch.randn(B, K, generator=gen) * 3
    P[..., 36] = torch.randint(0, 3, (B, K), generator=gen).float()
    i = torch.arange(B, dtype=torch.float64)
    calib = torch.stack((600 + 7 * i, 170 + 3 * i, 700 + 5 * i, 705 + 4 * i, 0.06 - 0.01 * i, -0.002 + 0.001 * i), 1)
    ratio = torch.stack((1.0 + 0.03 * i, 1.02 - 0.015 * i), 1)
    inv = torch.stack([torch.tensor([[0.97 + 0.01 * b, 0.002 * b, -3.0 + b], [-0.001 * b, 0.975 + 0.004 * b, 1.5 - 0.7 * b]],
                                    dtype=torch.float64) for b in range(B)])
    # resample the score logits whose reference score is close to a threshold
    for _ in range(100):
        sg = 1.0 / (1.0 + torch.exp(-P[..., 35].double()))
        sc = sg * torch.exp(-P[..., 34].double())
        bad = (sc - DECODE_THRESHOLD).abs() < 10 * DECODE_CLEAR * DECODE_THRESHOLD
        if not bool(bad.any()):
            break
        P[..., 35] = torch.where(bad, torch.randn(B, K, generator=gen) * 3, P[..., 35])
    # planted rows: first, last, both sides of each block border, the rest spread out
    n = B * K
    spots = sorted({0, 255, 256, n - 1})
    spots += [int(v) for v in np.linspace(3, n - 4, len(PLANTED) - len(spots))]
    assert len(set(spots)) == len(PLANTED)
    where = {}
    for name, flat in zip(PLANTED, spots):
        b, k = divmod(flat, K)
        where[name] = (b, k)
        r = P[b, k]
        cu, fu, rw = float(calib[b, 0]), float(calib[b, 2]), float(ratio[b, 0])
        if name in ("tie2-bin0", "tie3", "tie-10-11", "max-11"):
            top = {"tie2-bin0": [0, 4], "tie3": [3, 7, 11], "tie-10-11": [10, 11], "max-11": [11]}[name]
            r[9:21] = -1.0
            r[9 + torch.tensor(top)] = 2.0
            r[21:33] = 0.02 * (torch.arange(12) - 5.5)   # every bin its own residual
        elif name.startswith("ang-"):
            target = {"ang-at-pi": PI_F, "ang-above-pi": np.nextafter(PI_F, F32(4)), "ang-below-pi": np.nextafter(PI_F, F32(0))}[name]
            r[9:21] = -1.0
            r[9 + 5] = 2.0
            r[21 + 5] = float(_res_for(5, target))
        elif name in ("ry-plus", "ry-minus"):
            sgn = 1.0 if name == "ry-plus" else -1.0
            r[9:21] = -1.0
            r[9 + (5 if sgn > 0 else 7)] = 2.0          # 5: 2.618 + 0.38 = 2.998; 7: 3.665 - 0.38 = 3.285 > pi -> -2.998
            r[21:33] = sgn * 0.38
            xc = (cu + sgn * 600.0) * rw                # atan2(+-600, fu) = +-0.7: ry passes +-pi
            r[0], r[2] = xc - 20.0, xc + 20.0
        elif name == "score-at-thr":
            r[34], r[35] = 0.0, 0.0
        elif name == "camdis-nan":
            r[33] = 0.01                                # smaller than the lateral offset tx
    return P.contiguous(), calib.contiguous(), ratio.contiguous(), inv.contiguous(), where


def kitti_decode(P, calib, ratio, inv, use_camera_dis, threshold):
    """-> rows (B, K, 14) float64, keep (B, K) bool, host tensors"""
    with np.errstate(invalid="ignore"):   # the planted row whose depth is below its lateral offset: sqrt of a negative number
        rows, keep = RS.kitti_decode(P, calib.numpy(), ratio.numpy(), None if inv is None else inv.numpy(), threshold=threshold,
                                     use_camera_dis=bool(use_camera_dis))
    return torch.from_numpy(rows), torch.from_numpy(keep)


def p2_of(calib):
    """(B, 6) calibration constants -> the (B, 3, 4) float32 projection matrices they come from"""
    c = calib.double()
    P = torch.zeros(c.shape[0], 3, 4, dtype=torch.float64)
    P[:, 0, 0], P[:, 0, 2], P[:, 0, 3] = c[:, 2], c[:, 0], -c[:, 4] * c[:, 2]
    P[:, 1, 1], P[:, 1, 2], P[:, 1, 3] = c[:, 3], c[:, 1], -c[:, 5] * c[:, 3]
    P[:, 2, 2] = 1.0
    return P.float()


# ---------------------------------------------------------------------------------------------------------------- shared references
_CACHE = {}


def fusion_reference(name):
    """-> (predsO, predsM, rows of `fusion_rows`) of a case, computed once per process; callers leave them unchanged"""
    if ("f", name) not in _CACHE:
        O, M = fusion_inputs(name)
        thres, iou_thres = fusion_thresholds(name)
        _CACHE["f", name] = (O, M, fusion_rows(O, M, thres, iou_thres, FUSION_CASES[name][3]))
    return _CACHE["f", name]


def decode_reference(B, K, with_inv, cam, threshold):
    """-> (rows, keep) of `kitti_decode` on `decode_inputs(B, K)`, computed once per process"""
    key = ("d", B, K, bool(with_inv), bool(cam), threshold)
    if key not in _CACHE:
        P, calib, ratio, inv, _ = decode_inputs(B, K)
        _CACHE[key] = kitti_decode(P, calib, ratio, inv if with_inv else None, cam, threshold)
    return _CACHE[key]
