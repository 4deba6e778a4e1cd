"""The validator's depth fusion, the KITTI image crop and the KITTI decode (csrc/post.hip, csrc/kitti_row.h) against the references
of val_tail_ref.py, at the shapes and edges its case tables list.

* every output is a sentinel-filled buffer with guard elements behind it: what must be written was written, nothing behind it was;
* the crop is held to bit equality at every pixel, the decode's conversions and float32 sums to bit equality, its transcendental
  columns to 1e-6, the fusion to the near-maximiser rule of `val_tail_ref.check_fusion`;
* calls go through the C ABI, and through kitti.aggregate_o2m_preds / augment_images / decode_preds_device wherever those can
  express the arguments; both must give the same bits.
tests/test_val_tail_ref_host.py pins the references and checks, from them alone, every condition relied on here."""
import math

import numpy as np
import pytest
import torch

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, ops, predict
from yolov10_3d_amd._lib import Y3DError

import tail_ref as R
import val_tail_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"


def guarded(shape, dtype, guard=256):
    """(whole buffer, view of `shape` at its start): sentinel everywhere, `guard` elements behind the view"""
    n = math.prod(shape)
    buf = R.sentinel(n + guard, dtype, DEV)
    return buf, buf[:n].view(shape)


def check_guard(buf, view, what):
    assert not bool(R.untouched(view).any()), f"{what}: {int(R.untouched(view).sum())} elements were never written"
    assert bool(R.untouched(buf[view.numel():]).all()), f"{what}: a store went past the end of the output"


def same_bits(a, b):
    return torch.equal(R.bits(a.cpu()), R.bits(b.cpu()))


# ---------------------------------------------------------------------------------------------------------------- depth fusion
@pytest.mark.parametrize("name", list(V.FUSION_CASES))
def test_kde_fusion_near_maximiser(name):
    """columns other than the depth and rows with at most one vote are predsO's bit for bit; a fused depth is bitwise one of the
    reference's float32 proposals, its float64 reference log-density is within tau of the maximum, and it IS the reference's pick
    wherever the reference's margin exceeds tau (the host test caps how many rows may fall under it)"""
    B, K, KM, nprop, fam, C, tau, cap = V.FUSION_CASES[name]
    O, M, rows = V.fusion_reference(name)
    thres, iou_thres = V.fusion_thresholds(name)
    Od, Md = O.to(DEV), M.to(DEV)
    buf, out = guarded((B, K, C), torch.float32)
    y3d.lib().kde_depth_fusion(Od.data_ptr(), B, K, Md.data_ptr(), KM, C, thres, iou_thres, nprop, out.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    check_guard(buf, out, f"kde_depth_fusion {name}")
    got = out.cpu()
    worst, off_pick = V.check_fusion(got, O, rows, tau, name)
    changed = (got[..., C - 4].view(torch.int32) != O[..., C - 4].view(torch.int32)).reshape(-1).nonzero().flatten().tolist()
    assert set(changed) <= {i for i, r in enumerate(rows) if r["n"] > 1}
    print(f"\n[fusion gpu] {name}: {sum(r['n'] > 1 for r in rows)} fused rows, {len(changed)} depths changed, {off_pick} not the "
          f"reference's pick, largest log-density gap {worst:.3e} (tau {tau:g})")
    if fam == "hi-eq-lo":
        assert same_bits(got, O)          # every voter at the row's own depth: the fused depth is that depth
    assert same_bits(kitti.aggregate_o2m_preds(Od, Md, thres, iou_thres, nprop), got), "the wrapper and the C ABI disagree"


def test_kde_fusion_refuses_without_writing():
    """KM past the LDS bound (4096 and the first size above the bound), nprop = 1, C = 7 and a NULL pointer are errors before any
    launch: the sentinel output is untouched"""
    L, st = y3d.lib(), ops.stream()
    O = torch.zeros(1, 2, 37, device=DEV)
    M = torch.zeros(1, 4096, 37, device=DEV)
    buf, out = guarded((1, 2, 37), torch.float32)
    for km in (4096, V.FUSION_KM_MAX + 1):
        with pytest.raises(Y3DError, match="kde_depth_fusion"):
            L.kde_depth_fusion(O.data_ptr(), 1, 2, M.data_ptr(), km, 37, V.THRES, V.IOU_THRES, 33, out.data_ptr(), st)
    with pytest.raises(Y3DError, match="kde_depth_fusion"):
        L.kde_depth_fusion(O.data_ptr(), 1, 2, M.data_ptr(), 40, 37, V.THRES, V.IOU_THRES, 1, out.data_ptr(), st)
    with pytest.raises(Y3DError, match="kde_depth_fusion"):
        L.kde_depth_fusion(O.data_ptr(), 1, 2, M.data_ptr(), 40, 7, V.THRES, V.IOU_THRES, 33, out.data_ptr(), st)
    for args in ((None, M.data_ptr(), out.data_ptr()), (O.data_ptr(), None, out.data_ptr()), (O.data_ptr(), M.data_ptr(), None)):
        with pytest.raises(Y3DError, match="kde_depth_fusion"):
            L.kde_depth_fusion(args[0], 1, 2, args[1], 40, 37, V.THRES, V.IOU_THRES, 33, args[2], st)
    torch.cuda.synchronize()
    assert bool(R.untouched(buf).all()), "a refused call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------- image crop
def run_aug(imgs, parts, flips, tinvs, out_wh, mode, what):
    """y3d_kitti_image_aug through the C ABI into a guarded buffer.  imgs: host (H, W, 3) uint8 arrays; parts: None (no partner
    table at all) or a list with None entries (NULL entries of a table that is there) -> the output on the host"""
    B = len(imgs)
    di = [torch.from_numpy(a).to(DEV).contiguous() for a in imgs]
    dp = None if parts is None else [None if p is None else torch.from_numpy(p).to(DEV).contiguous() for p in parts]
    src = torch.tensor([t.data_ptr() for t in di], dtype=torch.int64).to(DEV)
    src2 = None if dp is None else torch.tensor([0 if t is None else t.data_ptr() for t in dp], dtype=torch.int64).to(DEV)
    hw = torch.tensor([a.shape[:2] for a in imgs], dtype=torch.int32).to(DEV)
    fl = torch.tensor([int(f) for f in flips], dtype=torch.int32).to(DEV)
    ti = torch.tensor(np.asarray(tinvs, np.float64).reshape(B, 6), dtype=torch.float64).to(DEV)
    W, H = out_wh
    buf, out = guarded((B, 3, H, W), torch.float32) if mode == 0 else guarded((B, H, W, 3), torch.uint8)
    y3d.lib().kitti_image_aug(src.data_ptr(), None if src2 is None else src2.data_ptr(), hw.data_ptr(), fl.data_ptr(), ti.data_ptr(), B, H, W, mode,
                              out.data_ptr(), ops.stream())
    torch.cuda.synchronize()
    if mode == 0:
        check_guard(buf, out, what)
    else:  # a pixel may legitimately equal the byte sentinel: only the guard is checked
        assert bool(R.untouched(buf[out.numel():]).all()), f"{what}: a store went past the end of the output"
    return out.cpu()


def assert_aug(got, want_u8, mode, what):
    """uint8 NHWC: the reference's pixels; float NCHW: those / 255 in float32; bit for bit"""
    want = torch.from_numpy(np.stack(want_u8) if mode == 1 else np.stack([V.aug_float(w) for w in want_u8]))
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype}"
    ne = R.bits(got) != R.bits(want)
    if bool(ne.any()):
        i = tuple(ne.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} values differ; first at {i}: got {got[i]!r}, expected {want[i]!r}")


@pytest.mark.parametrize("name", list(V.AUG_CASES))
def test_image_aug_equals_reference_every_pixel(name):
    """each map unflipped and flipped in one batch, with and without the partner, in both output modes"""
    H, W, out_wh, tinv = V.AUG_CASES[name]
    img, part = V.aug_sources(H, W, 11)
    for parts in (None, [part, part]):
        p = None if parts is None else part
        want = [V.kitti_image_aug(img, p, f, tinv, out_wh) for f in (0, 1)]
        if name == "all-outside":
            assert not any(w.any() for w in want)
        for mode in (0, 1):
            what = f"kitti_image_aug {name} partner {parts is not None} mode {mode}"
            got = run_aug([img, img], parts, [0, 1], [tinv, tinv], out_wh, mode, what)
            assert_aug(got, want, mode, what)
            di, dq = torch.from_numpy(img).to(DEV), torch.from_numpy(part).to(DEV)
            via = kitti.augment_images([di, di], [None if parts is None else dq] * 2, [False, True], [tinv, tinv], out_wh,
                                       "float" if mode == 0 else "uint8")
            assert same_bits(via, got), f"{what}: augment_images and the C ABI disagree"


def test_image_aug_mixed_batch_with_null_partner_entries():
    """one launch over sources of different sizes, different maps, mixed flips, and a partner table some of whose entries are NULL
    (a flipped image without a partner next to an unflipped one with: only the C ABI expresses it)"""
    imgs, parts, tinvs, want = [], [], [], []
    for i, (name, f, hasp) in enumerate(zip(V.AUG_MIXED, V.AUG_MIXED_FLIP, V.AUG_MIXED_PARTNER)):
        H, W, _, tinv = V.AUG_CASES[name]
        img, part = V.aug_sources(H, W, 20 + i)
        imgs.append(img)
        parts.append(part if hasp else None)
        tinvs.append(tinv)
        want.append(V.kitti_image_aug(img, parts[-1], f, tinv, V.AUG_MIXED_OUT))
    for mode in (0, 1):
        got = run_aug(imgs, parts, V.AUG_MIXED_FLIP, tinvs, V.AUG_MIXED_OUT, mode, f"kitti_image_aug mixed batch mode {mode}")
        assert_aug(got, want, mode, f"kitti_image_aug mixed batch mode {mode}")


def test_image_aug_every_blend_pair():
    """src[y, x] = y and partner[y, x] = x under the identity map: all 65 536 pairs of the mixup blend, unflipped and flipped"""
    img, part = V.blend_pair_sources()
    ident = [1, 0, 0, 0, 1, 0]
    want = [V.kitti_image_aug(img, part, f, ident, (256, 256)) for f in (0, 1)]
    for mode in (0, 1):
        got = run_aug([img, img], [part, part], [0, 1], [ident, ident], (256, 256), mode, f"kitti_image_aug blend pairs mode {mode}")
        assert_aug(got, want, mode, f"kitti_image_aug blend pairs mode {mode}")


def test_image_aug_past_the_grid_cap():
    """3 x 512 x 384 output pixels from 16 x 16 sources: more than 2 048 blocks of 256, the grid-stride loop takes a second trip"""
    B, H, W, out_wh = V.AUG_BIG
    assert B * out_wh[0] * out_wh[1] > 2048 * 256
    sx, sy = W / out_wh[0], H / out_wh[1]
    tinvs = [[sx, 0, 0, 0, sy, 0], [sx * 0.8, sy * 0.3, -1.5, -sx * 0.3, sy * 0.8, 3.0], [sx * 1.2, 0, -2.25, 0, sy * 1.1, 1.5]]
    flips = [0, 1, 0]
    src = [V.aug_sources(H, W, 40 + b) for b in range(B)]
    imgs, parts = [s[0] for s in src], [None, src[1][1], None]
    want = [V.kitti_image_aug(imgs[b], parts[b], flips[b], tinvs[b], out_wh) for b in range(B)]
    for mode in (0, 1):
        got = run_aug(imgs, parts, flips, tinvs, out_wh, mode, f"kitti_image_aug big mode {mode}")
        assert_aug(got, want, mode, f"kitti_image_aug big mode {mode}")


# ---------------------------------------------------------------------------------------------------------------- KITTI decode
BIT_COLS = [0, 2, 3, 4, 5, 6, 7, 8]      # cls, x1, y1, x2, y2 (conversions and one float64 division), h, w, l (one rounded sum)
TOL_COLS = [1, 9, 10, 11, 12, 13]        # alpha, x, y, z, ry, score: behind expf / atan2 / sqrt
DECODE_RUNS = [(B, K, inv, cam) for B, K in V.DECODE_SHAPES for inv in (True, False) for cam in (False, True)]


@pytest.mark.parametrize("run", DECODE_RUNS, ids=[f"B{b}-K{k}-{'inv' if i else 'fixed'}-{'camdis' if c else 'rect'}" for b, k, i, c in DECODE_RUNS])
def test_kitti_decode_rows_blocks_and_planted_edges(run):
    """generated rows over three blocks with a ragged last one, every image its own constants, with heading-bin ties, angles at and
    around pi, rotation_y wraps, a score exactly at the threshold (and the threshold at its two float64 neighbours), a NaN depth
    under camera distance: keep exactly the reference's, conversions and float32 sums bit for bit, the rest within 1e-6;
    y3d_predict3d_rows keeps the same rows with the same 14 values bit for bit"""
    B, K, with_inv, cam = run
    P, calib, ratio, inv, where = V.decode_inputs(B, K)
    L, st = y3d.lib(), ops.stream()
    Pd, cd, rd = P.to(DEV), calib.to(DEV), ratio.to(DEV)
    ivd = inv.to(DEV) if with_inv else None
    ms = torch.tensor(kitti.CLS_MEAN_SIZE, dtype=torch.float64, device=DEV)
    thresholds = V.DECODE_THRESHOLDS if (with_inv and not cam) else V.DECODE_THRESHOLDS[:1]
    for thr in thresholds:
        want, wkeep = V.decode_reference(B, K, with_inv, cam, thr)
        obuf = R.sentinel(B * K * 14 + 256, torch.int64, DEV)      # float64 rows behind an int64 sentinel (a NaN with a payload)
        kbuf, keep = guarded((B, K), torch.uint8)
        L.kitti_decode(Pd.data_ptr(), B, K, cd.data_ptr(), rd.data_ptr(), None if ivd is None else ivd.data_ptr(), ms.data_ptr(), 3, int(cam), thr,
                       obuf.data_ptr(), keep.data_ptr(), st)
        torch.cuda.synchronize()
        assert not bool(R.untouched(obuf[:B * K * 14]).any()) and bool(R.untouched(obuf[B * K * 14:]).all()), "rows: unwritten values or a store past the end"
        assert bool(R.untouched(kbuf[B * K:]).all()) and bool((keep <= 1).all()), "keep: a store past the end or an unwritten flag"
        got = obuf[:B * K * 14].view(torch.float64).view(B, K, 14).cpu()
        gkeep = keep.cpu().bool()
        bad = (gkeep != wkeep).nonzero().tolist()
        assert not bad, f"threshold {thr!r}: keep differs from `not (score < threshold)` of the reference in rows {bad[:8]}"
        b, k = where["score-at-thr"]
        assert bool(gkeep[b, k]) == (thr <= 0.5) and got[b, k, 13].item() == 0.5
        ne = (got[..., BIT_COLS].view(torch.int64) != want[..., BIT_COLS].view(torch.int64)).nonzero().tolist()
        assert not ne, f"{len(ne)} conversion / float32 values differ; first (b, k, column index in {BIT_COLS}): {ne[0]}"
        err = (got[..., TOL_COLS] - want[..., TOL_COLS]).abs()
        print(f"\n[decode gpu] {run} threshold {thr!r}: kept {int(gkeep.sum())} of {B * K}, largest error of the transcendental columns "
              f"{float(err[~err.isnan()].max()):.3e}")
        torch.testing.assert_close(got[..., TOL_COLS], want[..., TOL_COLS], rtol=1e-6, atol=1e-6, equal_nan=True)
        if cam:
            b, k = where["camdis-nan"]
            assert math.isnan(got[b, k, 11].item()) and int(got.isnan().sum()) == 1
        rows2, keep2 = kitti.decode_preds_device(Pd, cd, rd, inv if with_inv else None, undo_augment=with_inv, threshold=thr, use_camera_dis=cam)
        assert torch.equal(rows2.cpu().view(torch.int64), got.view(torch.int64)) and torch.equal(keep2.cpu(), gkeep), "decode_preds_device and the C ABI disagree"
    # the predictor's row pass on the same rows: the kept rows, in order, with this kernel's bits
    thr = thresholds[0]
    prow, _, _, cnt = predict.predict3d_rows(Pd, cd, V.p2_of(calib), rd, ivd, thr, use_camera_dis=cam)
    prow, cnt = prow.cpu(), cnt.cpu()
    want, wkeep = V.decode_reference(B, K, with_inv, cam, thr)
    assert cnt.tolist() == wkeep.sum(1).tolist()
    got1, _ = kitti.decode_preds_device(Pd, cd, rd, inv if with_inv else None, undo_augment=with_inv, threshold=thr, use_camera_dis=cam)
    got1 = got1.cpu()
    for b in range(B):
        assert torch.equal(prow[b, :int(cnt[b])].view(torch.int64), got1[b][wkeep[b]].view(torch.int64)), f"image {b}: predict3d rows differ from the decode's"
