"""GPU: the KITTI split resident on the device (kitti.DeviceSplit, csrc/kitti_cache.hip).  The plan kernel against its numpy restatement
(tests/kitti_cache_ref.py) bit for bit with guard rows; that restatement against `kitti.pack_labels` and the frames' pixels; the
cached `build_batch` against the path-based one, tensor for tensor, for every recorded argument set, both image modes and both label
layouts (the existing tests tie the path-based builder to the reference's recorded run); no file access after the load; the byte
budget; the pinned ring under reuse; `val.Validator3d` on a resident split."""
import os
import shutil

import numpy as np
import pytest
import torch

import kitti_cache_ref as R
from kitti_labels_tree import argset, fixture, frame_pixels, write_tree

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import kitti, val  # noqa: E402
from yolov10_3d_amd import ops as P_ops  # noqa: E402
from yolov10_3d_amd._lib import Y3DError  # noqa: E402

DEV = "cuda"
ARGSETS = ["default", "camdis", "val", "nomix"]
GUARD, SENTINEL = 3, 0xA5
BLANK = 3  # the frame whose label file is emptied in the second tree: item 4's recorded mixup partner, and a primary


@pytest.fixture(scope="module")
def z():
    z = fixture()
    # frames that share a calibration share a size: the condition under which the resident split's frame_info (true sizes of every
    # frame) and the path-based builder's (sizes of the batch's own frames only) accept the same mixup partners
    groups = {}
    for i, text in enumerate(z["calib_text"]):
        groups.setdefault(str(text), set()).add(tuple(int(v) for v in z["frame_wh"][i]))
    assert len(groups) == 3 and all(len(s) == 1 for s in groups.values()), groups
    assert [tuple(int(v) for v in wh) for wh in z["frame_wh"]] == [(1242, 375)] * 6 + [(1224, 370)] * 3 + [(1238, 374)] * 3
    return z


@pytest.fixture(scope="module")
def root(tmp_path_factory, z):
    return write_tree(str(tmp_path_factory.mktemp("kitti_cache")), z, images=True)


@pytest.fixture(scope="module")
def split(root):
    return kitti.DeviceSplit(root, device=DEV)


@pytest.fixture(scope="module")
def blank(tmp_path_factory, z, root):
    """the tree with one empty label file (the PNGs are copied, not encoded again) and its resident split"""
    zb = {k: z[k] for k in z.files}
    zb["label_text"] = zb["label_text"].copy()
    zb["label_text"][BLANK] = ""
    r = os.path.join(str(tmp_path_factory.mktemp("kitti_cache_blank")), "tree")
    shutil.copytree(root, r)
    write_tree(r, zb)
    assert open(os.path.join(r, "training/label_2", f"{BLANK:06d}.txt")).read() == ""
    return r, kitti.DeviceSplit(r, device=DEV)


def wh(z, pos):
    return tuple(int(v) for v in z["frame_wh"][pos])


def need_bytes(z):
    return sum((w * h * 3 + 15) // 16 * 16 for w, h in (wh(z, p) for p in range(len(z["frame_wh"]))))


def host_tables(split):
    """the frame tables as the kernel reads them, read back"""
    return (split.arena.data_ptr(), split.img_off.cpu().numpy(), split.frame_hw.cpu().numpy(), split.rec_span.cpu().numpy(),
            split.P2.cpu().numpy())


def made_draws(z, positions, partners, flips, scales):
    """a draw table over the fixture's frames: a crop of the given scale, shifted off the centre, through get_affine_transform"""
    tr = []
    for pos, s in zip(positions, scales):
        size = np.array(wh(z, pos), np.float64)
        tr.append(kitti.get_affine_transform(size / 2 + np.array([7.0, -3.0]) * (s != 1.0), size * s, kitti.RESOLUTION, inv=True))
    return R.draw_rows(positions, partners, flips, scales, [t[0] for t in tr], [t[1] for t in tr])


def recorded_draws(z, name):
    items = argset(z, name)[3]
    return R.draw_rows(items, z[f"{name}/partner"], z[f"{name}/flip"], z[f"{name}/scale"], z[f"{name}/trans"], z[f"{name}/trans_inv"])


def guarded_plan(split, draws):
    """the plan kernel into buffers with GUARD sentinel rows behind the B it may write -> the B rows of each output"""
    B = len(draws)
    bufs = {}
    for k, dt, s in kitti.PLAN_TABLES:
        bufs[k] = torch.empty(B + GUARD, *s, dtype=dt, device=DEV)
        bufs[k].view(torch.uint8).fill_(SENTINEL)
    out = kitti.plan_batch(split, draws, out=bufs)
    assert all(out[k] is bufs[k] for k in bufs)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        guard = t[B:].contiguous().view(torch.uint8)
        assert bool((guard == SENTINEL).all()), f"{k}: the rows behind the batch were written"
    return {k: t[:B].cpu().numpy() for k, t in bufs.items()}


def check_plan(split, draws):
    got, want = guarded_plan(split, draws), R.plan(*host_tables(split), draws)
    assert [k for k, _, _ in kitti.PLAN_TABLES] == [k for k, _, _ in R.OUTPUTS]
    for k, dt, s in R.OUTPUTS:
        assert got[k].dtype == dt and got[k].shape == want[k].shape == (len(draws),) + s, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    return got


# ------------------------------------------------------------------------------------------------------------ the split's tables
def test_split_tables(z, root, split):
    N = len(z["label_text"])
    assert len(split) == N and split.ids == list(range(N)) and split.nbytes == need_bytes(z) == split.arena.numel()
    assert split.arena.dtype == torch.uint8 and split.arena.data_ptr() % 16 == 0
    off, hw, span = split.img_off.cpu().numpy(), split.frame_hw.cpu().numpy(), split.rec_span.cpu().numpy()
    assert off.dtype == np.int64 and hw.dtype == np.int32 and span.dtype == np.int32 and (off % 16 == 0).all()
    assert split.rec.dtype == torch.float64 and split.P2.dtype == torch.float32 and tuple(split.P2.shape) == (N, 2, 12)
    rec, P2, row = split.rec.cpu().numpy(), split.P2.cpu().numpy(), 0
    for pos in range(N):
        W, H = wh(z, pos)
        assert tuple(hw[pos]) == (H, W) and (pos == 0 or off[pos] >= off[pos - 1] + hw[pos - 1].prod() * 3)
        lab = kitti.label_records(kitti.read_label(os.path.join(root, "training/label_2", f"{pos:06d}.txt")))
        assert tuple(span[pos]) == (row, len(lab)) and rec[row:row + len(lab)].tobytes() == lab.tobytes()
        row += len(lab)
        P = kitti.read_calib(os.path.join(root, "training/calib", f"{pos:06d}.txt"))
        assert P2[pos, 0].tobytes() == P.tobytes() and P2[pos, 1].tobytes() == kitti.flip_calib(P, (W, H)).tobytes()
        assert split.frame_info(pos) == ((P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(lab), (W, H))
        assert torch.equal(split.frame(pos).cpu(), torch.from_numpy(frame_pixels(pos, W, H)))
    assert row == rec.shape[0]
    ms = torch.tensor(kitti.CLS_MEAN_SIZE, dtype=torch.float64)
    assert torch.equal(split.mean_size.cpu(), ms)


# ------------------------------------------------------------------------------------------------------------ the plan kernel
def test_plan_single_image(z, split):
    got = check_plan(split, made_draws(z, [0], [-1], [0], [1.0]))
    assert got["src2"][0] == 0 and got["mixed"][0] == 0 and got["flip"][0] == 0 and got["src"][0] == split.arena.data_ptr()


def test_plan_partners_flips_and_repeated_frames(z, split):
    draws = recorded_draws(z, "default")
    items = argset(z, "default")[3]
    assert sorted(items)[:2] == [0, 0] and items.count(4) == 2 and items.count(9) == 2  # frames repeated
    assert (draws[:, 1] >= 0).any() and (draws[:, 1] < 0).any() and (draws[:, 2] == 1).any() and (draws[:, 2] == 0).any()
    assert len(items) > 1  # (one 64-thread block; B behind a block's end is covered by the guard rows)
    got = check_plan(split, draws)
    assert got["mixed"].tolist() == [int(p >= 0) for p in z["default/partner"]]


def test_plan_more_than_one_block(z, split):
    N = len(split)
    pos = [i % N for i in range(130)]
    same = {0: 5, 1: 4, 2: 3, 6: 8, 9: 11}  # partners of the primary's size
    par = [same.get(p, -1) if i % 3 else -1 for i, p in enumerate(pos)]
    check_plan(split, made_draws(z, pos, par, [i % 2 for i in range(130)], [1.0 + 0.001 * (i % 7) for i in range(130)]))


def test_plan_with_an_empty_label_file(z, blank):
    _, sb = blank
    span = sb.rec_span.cpu().numpy()
    assert span[BLANK, 1] == 0 and span[BLANK, 0] == span[BLANK + 1, 0] and sb.n_lines[BLANK] == 0
    draws = recorded_draws(z, "default")
    assert BLANK in draws[:, 0] and BLANK in draws[:, 1]
    got = check_plan(sb, draws)
    b = list(draws[:, 0]).index(BLANK)
    assert got["img_i"][b, 1] == 0 and got["img_i"][list(draws[:, 1]).index(BLANK), 3] == 0


def test_plan_frame_with_55_label_lines(z, split):
    pos = split.n_lines.index(55)
    got = check_plan(split, made_draws(z, [pos, 0, pos], [-1, pos, pos], [1, 0, 1], [0.9, 1.1, 1.0]))
    assert got["img_i"][0, 1] == 55 and got["img_i"][1, 3] == 55 and got["img_i"][2, 1] == got["img_i"][2, 3] == 55


def test_plan_last_frame_of_the_split(z, split):
    last = len(split) - 1
    got = check_plan(split, made_draws(z, [last, last - 1, last], [-1, last, last], [0, 1, 1], [1.0, 1.2, 0.8]))
    W, H = wh(z, last)
    off = int(split.img_off.cpu()[last])
    assert off == int(split.img_off.cpu().max()) and off + H * W * 3 <= split.arena.numel()
    assert got["src"][0] == got["src2"][1] == split.arena.data_ptr() + off
    assert got["img_i"][0, 0] + got["img_i"][0, 1] == split.rec.shape[0]  # its records are the last ones


def test_plan_refuses_bad_draws(z, split):
    N = len(split)
    ok = made_draws(z, [0, 1], [-1, 0], [0, 1], [1.0, 1.0])
    for col, value, what in ((0, N, "position"), (0, -1, "position"), (0, 0.5, "position"), (1, N, "partner"), (1, -2, "partner")):
        bad = ok.copy()
        bad[1, col] = value
        with pytest.raises(Y3DError, match=what):
            kitti.plan_batch(split, bad)
    with pytest.raises(Y3DError, match="B = 0"):
        kitti.plan_batch(split, np.zeros((0, 16), np.float64))
    with pytest.raises(Y3DError):
        kitti.plan_batch(split, ok.astype(np.float32))
    with pytest.raises(Y3DError, match="null"):
        y3d.lib().kitti_plan_batch(None, None, None, None, N, None, None, None, 1, None, None, None, None, None, None, None, None, None)
    check_plan(split, ok)  # and the table itself is fine


# ------------------------------------------------------------------------------------------------------------ the restatement's pin
@pytest.mark.parametrize("name", ARGSETS)
def test_restatement_matches_pack_labels_and_the_pixels(z, root, split, name):
    mode, args, seed, items = argset(z, name)
    draws = recorded_draws(z, name)
    base, off, hw, span, P2 = host_tables(split)
    p = R.plan(base, off, hw, span, P2, draws)
    lab = lambda i: kitti.read_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
    calib = lambda i: kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt"))
    partners = [int(v) for v in z[f"{name}/partner"]]
    flips = [bool(v) for v in z[f"{name}/flip"]]
    P2s = [kitti.flip_calib(calib(i), wh(z, i)) if f else calib(i) for i, f in zip(items, flips)]  # as build_batch computes them
    packed = kitti.pack_labels([lab(i) for i in items], [lab(q) if q >= 0 else None for q in partners], P2s, list(z[f"{name}/trans"]), flips,
                               list(z[f"{name}/scale"]), [wh(z, i) for i in items], DEV)
    img_i, img_f, prec = packed["img_i"].cpu().numpy(), packed["img_f"].cpu().numpy(), packed["rec"].cpu().numpy()
    assert np.array_equal(p["img_i"][:, [1, 3, 4, 5, 6]], img_i[:, [1, 3, 4, 5, 6]])
    assert p["img_f"].tobytes() == img_f.tobytes()
    rec, arena = split.rec.cpu().numpy(), split.arena.cpu().numpy()
    for b, (pos, q) in enumerate(zip(items, partners)):
        for first, n in ((0, 1), (2, 3)):
            mine = rec[p["img_i"][b, first]:p["img_i"][b, first] + p["img_i"][b, n]]
            theirs = prec[img_i[b, first]:img_i[b, first] + img_i[b, n]]
            assert mine.tobytes() == theirs.tobytes(), (name, b, first)
        W, H = wh(z, pos)
        assert tuple(p["hw"][b]) == (H, W)
        o = int(p["src"][b]) - base
        assert o % 16 == 0 and np.array_equal(arena[o:o + H * W * 3].reshape(H, W, 3), frame_pixels(pos, W, H))
        if q >= 0:
            o = int(p["src2"][b]) - base
            assert wh(z, q) == (W, H) and np.array_equal(arena[o:o + H * W * 3].reshape(H, W, 3), frame_pixels(q, W, H))
        else:
            assert p["src2"][b] == 0
        assert p["mixed"][b] == (q >= 0) and p["flip"][b] == flips[b]
        assert p["trans_inv"][b].tobytes() == np.asarray(z[f"{name}/trans_inv"][b], np.float64).tobytes()


# ------------------------------------------------------------------------------------------------------------ end to end
def same_batch(got, want):
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(g, w), k
    assert got["im_file"] == want["im_file"] and all(type(f) is str for f in got["im_file"])
    assert len(got["info"]) == len(want["info"]) == len(got["ori_shape"]) == len(want["ori_shape"])
    for gi, wi, gs, ws in zip(got["info"], want["info"], got["ori_shape"], want["ori_shape"]):
        assert list(gi) == list(wi) and gi["img_id"] == wi["img_id"] and type(gi["img_id"]) is type(wi["img_id"])
        for k in ("img_size", "trans_inv"):
            assert gi[k].dtype == wi[k].dtype and gi[k].shape == wi[k].shape and gi[k].tobytes() == wi[k].tobytes(), k
        assert gs.dtype == ws.dtype and gs.shape == ws.shape and gs.tobytes() == ws.tobytes()


def both(source, sp, items, args, mode, seed, **kw):
    np.random.seed(seed)
    want = kitti.build_batch(source, items, args, DEV, mode=mode, **kw)
    after = np.random.get_state()[1].copy()
    np.random.seed(seed)
    got = sp.build_batch(items, args, mode=mode, **kw)
    assert np.array_equal(np.random.get_state()[1], after)  # the same draws were consumed
    return got, want


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("img_mode", ["uint8", "float"])
@pytest.mark.parametrize("name", ARGSETS)
def test_cached_batch_equals_the_disk_batch(z, root, split, name, img_mode, compact):
    mode, args, seed, items = argset(z, name)
    got, want = both(root, split, items, args, mode, seed, img_mode=img_mode, compact=compact)
    same_batch(got, want)
    assert ("counts" in got) != compact and got["img"].dtype == (torch.uint8 if img_mode == "uint8" else torch.float32)
    if name == "default" and not compact:  # the draws are the recorded ones: partners and flips happened
        assert got["mixed"].cpu().tolist() == [int(p >= 0) for p in z["default/partner"]]


def test_build_batch_dispatches_on_a_device_split(z, root, split, blank):
    mode, args, seed, items = argset(z, "default")
    np.random.seed(seed)
    want = split.build_batch(items, args, mode=mode, compact=True, img_mode="float")
    np.random.seed(seed)
    same_batch(kitti.build_batch(split, items, args, DEV, mode=mode, compact=True, img_mode="float"), want)
    with pytest.raises(Y3DError):
        kitti.build_batch(split, items, args, "cpu", mode=mode)
    with pytest.raises(Y3DError, match="depth maps"):
        split.build_batch(items, kitti.data_args(load_depth_maps=True))
    with pytest.raises(Y3DError, match="test"):
        split.build_batch(items, args, mode="test")
    with pytest.raises(Y3DError, match="test"):
        kitti.DeviceSplit(root, mode="test", device=DEV)
    with pytest.raises(Y3DError):
        split.build_batch([len(split)], args)
    # the tree with an empty label file, as primary and as partner candidate
    rb, sb = blank
    same_batch(*both(rb, sb, items, args, mode, seed, compact=True))


def test_epoch_yields_every_frame_once(z, split):
    args = kitti.data_args()
    np.random.seed(1)
    seen = [f for b in split.epoch(5, args, mode="val", shuffle=True, seed=2) for f in b["im_file"]]
    assert sorted(seen) == [f"{i:06d}.txt" for i in range(len(split))]
    assert seen == [f"{i:06d}.txt" for idx in kitti.epoch_indices(len(split), 5, seed=2) for i in idx]
    sizes = [b["img"].shape[0] for b in split.epoch(5, args, mode="val", drop_last=True)]
    assert sizes == [5, 5]


def test_no_disk_after_load(tmp_path, z, root):
    r = os.path.join(str(tmp_path), "tree")
    shutil.copytree(root, r)
    mode, args, seed, items = argset(z, "default")
    vmode, vargs, vseed, vitems = argset(z, "val")
    wants = []
    for s in (seed, seed + 1):
        np.random.seed(s)
        wants.append(kitti.build_batch(r, items, args, DEV, mode=mode))
    want_val = kitti.build_batch(r, vitems, vargs, DEV, mode="val", compact=True)
    sp = kitti.DeviceSplit(os.path.join(r, "ImageSets", "train.txt"), device=DEV, workers=3)
    shutil.rmtree(r)
    assert not os.path.exists(r)
    for s, want in zip((seed, seed + 1), wants):
        np.random.seed(s)
        same_batch(sp.build_batch(items, args, mode=mode), want)
    same_batch(kitti.build_batch(sp, vitems, vargs, DEV, mode="val", compact=True), want_val)


def test_budget_is_checked_before_any_allocation(z, root):
    need = need_bytes(z)
    assert need == sum((w * h * 3 + 15) // 16 * 16 for w, h in [(1242, 375)] * 6 + [(1224, 370)] * 3 + [(1238, 374)] * 3) > 1 << 20
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(Y3DError, match=f"{need} bytes.*{1 << 20} bytes"):
        kitti.DeviceSplit(root, device=DEV, max_bytes=1 << 20)
    assert torch.cuda.memory_allocated() == before
    sp = kitti.DeviceSplit(root, device=DEV, max_bytes=need)  # exactly enough
    assert sp.nbytes == need and torch.cuda.memory_allocated() >= before + need


def test_ring_reuse_without_synchronising(z, root, split):
    mode, args, _, _ = argset(z, "default")
    items = [0, 4, 9, 6, 11]
    n = 2 * kitti.DeviceSplit.RING + 1
    got = []
    for k in range(n):  # more builds in flight than the ring has buffers, nothing waits in between
        np.random.seed(1000 + k)
        got.append(split.build_batch(items, args, mode=mode))
    distinct = {g["ratio_pad"].cpu().numpy().tobytes() + g["calib"].cpu().numpy().tobytes() + g["center_3d"].cpu().numpy().tobytes() for g in got}
    assert len(distinct) > kitti.DeviceSplit.RING  # the draws differ, so a stale table would show
    for k in range(n):
        np.random.seed(1000 + k)
        same_batch(got[k], kitti.build_batch(root, items, args, DEV, mode=mode))


# ------------------------------------------------------------------------------------------------------------ the validator
@pytest.fixture(scope="module")
def model_n3d():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml")).to(DEV)
    y3d.set_compute_dtype(before)
    return m.eval()


def test_validator3d_on_a_device_split(z, root, model_n3d):
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    try:
        sp = kitti.DeviceSplit(root, mode="val", device=DEV)
        idx = [0, 1, 2, 3]
        same_batch(val.Validator3d(model_n3d, sp, batch=4)._batch(idx), val.Validator3d(model_n3d, root, batch=4)._batch(idx))
        n, calib, data = val.Validator3d(model_n3d, sp)._dataset()
        n2, calib2, data2 = val.Validator3d(model_n3d, root)._dataset()
        assert n == n2 == len(sp) and data == data2 and all(calib(p) == calib2(p) for p in range(n))
        cached, disk = val.Validator3d(model_n3d, sp)(), val.Validator3d(model_n3d, root)()
        assert list(cached) == list(disk) and len(cached) >= 6
        assert all(np.isfinite(float(v)) for v in cached.values()) and all(np.isfinite(float(v)) for v in disk.values())
        with pytest.raises(Y3DError, match="KITTI"):
            val.Validator3d(model_n3d, sp, dataset="waymo")
    finally:
        y3d.set_compute_dtype(before)
