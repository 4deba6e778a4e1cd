"""GPU: the Waymo / Omni3D split resident in two tiers (json3d.DeviceSplit, csrc/json3d_cache.hip): HBM first, pinned host memory behind
it.  The split's tables and every frame's pixels in its tier; the plan kernel against its numpy restatement (tests/json3d_cache_ref.py)
bit for bit with guard rows, and that restatement's addresses against the frames' pixels; its refusals; the resident `build_batch`
against the path-based one, tensor for tensor, for every recorded run under three placements (all in HBM, the boundary behind position
4, all on the host), both image modes and both label layouts; a partner of another size; no file access after the load; both byte
budgets; the pinned ring under reuse; `epoch`; `val.Validator3d` on a resident split.  Every comparison is exact."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import json3d_cache_ref as R
from json3d_tree import DATASETS, RUNS, argset, fixture, frame_pixels, write_tree

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import json3d, kitti, val  # noqa: E402
from yolov10_3d_amd import ops as P_ops  # noqa: E402
from yolov10_3d_amd._lib import Y3DError  # noqa: E402

DEV = "cuda"
GUARD, SENTINEL = 3, 0xA5
BIG, SMALL = 480 * 320 * 3, 384 * 256 * 3  # the fixture's two frame sizes in bytes
TOTAL = 9 * BIG + 3 * SMALL
# placement -> (max_bytes, host_bytes, n_dev): all in HBM as kitti.DeviceSplit holds a split; positions 0-4 in HBM and 5-11 on the host;
# everything on the host
PLACEMENTS = {"hbm": (TOTAL, 0, 12), "boundary": (5 * BIG, 4 * BIG + 3 * SMALL, 5), "host": (0, TOTAL, 0)}
_TREES, _SPLITS, _WANT = {}, {}, {}


def wh(z, pos):
    return tuple(int(v) for v in z["frame_wh"][pos])


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    def tree(dataset):
        if dataset not in _TREES:
            z = fixture(dataset)
            assert [wh(z, p) for p in range(12)] == [(480, 320)] * 9 + [(384, 256)] * 3
            _TREES[dataset] = write_tree(str(tmp_path_factory.mktemp(f"json3d_cache_{dataset}")), z, dataset, images=True)
        return _TREES[dataset]

    yield tree
    _TREES.clear(), _SPLITS.clear(), _WANT.clear()


def split_of(trees, dataset, placement):
    if (dataset, placement) not in _SPLITS:
        max_bytes, host_bytes, n_dev = PLACEMENTS[placement]
        sp = json3d.DeviceSplit(trees(dataset), dataset, device=DEV, max_bytes=max_bytes, host_bytes=host_bytes)
        assert sp.n_dev == n_dev and sp.dataset == dataset
        _SPLITS[dataset, placement] = sp
    return _SPLITS[dataset, placement]


def disk_batch(trees, dataset, name, seed=None, **kw):
    """the path builder's batch of a recorded run, built once and shared (nobody writes to it)"""
    key = (dataset, name, seed, tuple(sorted(kw.items())))
    if key not in _WANT:
        mode, args, rseed, items = argset(fixture(dataset), name)
        np.random.seed(rseed if seed is None else seed)
        want = json3d.build_batch(trees(dataset), items, args, DEV, dataset=dataset, mode=mode, **kw)
        _WANT[key] = (want, np.random.get_state()[1].copy())
    return _WANT[key]


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


# ------------------------------------------------------------------------------------------------------------ the split's tables
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dataset", DATASETS)
def test_split_tables_and_pixels(trees, dataset, placement):
    z, sp = fixture(dataset), split_of(trees, dataset, placement)
    ref = json3d.read_split(trees(dataset), dataset)
    N, n_dev = 12, PLACEMENTS[placement][2]
    assert len(sp) == N and sp.ids == ref.ids == [int(i) for i in z["img_id"]] and sp.files == [ref.file(i) for i in ref.ids]
    want_n, want_dev, want_host, used, spilled = R.tiers([(h, w) for w, h in (wh(z, p) for p in range(N))], PLACEMENTS[placement][0])
    assert want_n == n_dev and sp.nbytes == used == sp.arena.numel() and sp.host_nbytes == spilled == sp.host_arena.numel()
    assert sp.arena.dtype == torch.uint8 and sp.arena.is_cuda and sp.host_arena.dtype == torch.uint8 and not sp.host_arena.is_cuda
    assert sp.host_arena.is_pinned() == (n_dev < N) and (n_dev == 0 or sp.arena.data_ptr() % 16 == 0)
    assert sp.host_arena.numel() == 0 or sp.host_arena.data_ptr() % 16 == 0
    off, hw, span = sp.img_off.cpu().numpy(), sp.frame_hw.cpu().numpy(), sp.rec_span.cpu().numpy()
    assert off.dtype == np.int64 and hw.dtype == np.int32 and span.dtype == np.int32 and off.shape == (N,) and hw.shape == span.shape == (N, 2)
    assert off.tolist() == want_dev.tolist() == sp.offsets.tolist() and sp.host_offsets.tolist() == want_host.tolist()
    assert [o == -1 for o in off.tolist()] == [p >= n_dev for p in range(N)]  # -1 exactly at the positions of the host tier
    assert sp.rec.dtype == torch.float64 and sp.P2.dtype == torch.float64 and tuple(sp.P2.shape) == (N, 2, 12)
    rec, P2, row = sp.rec.cpu().numpy(), sp.P2.cpu().numpy(), 0
    want_rec = np.concatenate([json3d.object_records(ref.anns.get(i, []), dataset) for i in ref.ids])
    assert rec.shape == want_rec.shape and rec.tobytes() == want_rec.tobytes()
    for pos, i in enumerate(ref.ids):
        W, H = wh(z, pos)
        n = len(ref.records(i))
        assert tuple(hw[pos]) == (H, W) and tuple(span[pos]) == (row, n) and sp.wh[pos] == (W, H) and sp.n_lines[pos] == n
        row += n
        P = ref.P2(i)
        assert P.dtype == np.float64 and P2[pos, 0].tobytes() == P.tobytes() and sp.P2_host[pos].tobytes() == P.tobytes()
        flipped = json3d.flip_calib(P, (W, H))
        assert flipped.dtype == np.float32 and P2[pos, 1].tobytes() == flipped.astype(np.float64).tobytes()
        cam = (P[0, 2], P[1, 2], P[0, 0], P[1, 1])
        assert sp.cam[pos] == cam and sp.frame_info(pos, primary=True) == (cam, n, (W, H)) and sp.frame_info(pos) == (cam, n, None)
        f = sp.frame(pos)
        assert f.is_cuda == (pos < n_dev) and tuple(f.shape) == (H, W, 3)
        if pos >= n_dev:  # a view of the pinned arena, not a copy
            assert f.data_ptr() == sp.host_arena.data_ptr() + int(want_host[pos])
        assert f.cpu().numpy().tobytes() == frame_pixels(pos, W, H).tobytes()
    assert row == rec.shape[0] and [sp.n_lines[p] for p in (2, 5, 11)] == [55, 0, 45] and span[5, 0] == span[6, 0]
    assert torch.equal(sp.mean_size.cpu(), torch.tensor(json3d.CLS_MEAN_SIZE[dataset], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------ the plan kernel
def made_draws(z, sp, positions, partners, flips, scales):
    """a draw table over the fixture's frames (a crop of the given scale, shifted off the centre) with the batch's staging buffer"""
    tr = []
    for pos, s in zip(positions, scales):
        size = np.array(wh(z, pos), np.float64)
        tr.append(kitti.get_affine_transform(size / 2 + np.array([7.0, -3.0]) * (s != 1.0), size * s, json3d.RESOLUTION, inv=True))
    staged, spill = sp._stage([p for pair in zip(positions, partners) for p in pair])
    want = R.staging(positions, partners, sp.n_dev, [(h, w) for w, h in sp.wh])
    assert (staged, 0 if spill is None else spill.numel()) == want and (spill is None) == (not staged)
    return R.draw_rows(positions, partners, flips, scales, [t[0] for t in tr], [t[1] for t in tr], staged), spill


def guarded_plan(sp, draws, spill):
    """the plan kernel into buffers with GUARD sentinel rows behind the B it may write -> the B rows of each output"""
    B = len(draws)
    bufs = {}
    for k, dt, s in kitti.PLAN_TABLES:
        bufs[k] = torch.empty(B + GUARD, *s, dtype=dt, device=DEV)
        bufs[k].view(torch.uint8).fill_(SENTINEL)
    out = json3d.plan_batch(sp, draws, out=bufs, spill=spill)
    assert all(out[k] is bufs[k] for k in bufs)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t[B:].contiguous().view(torch.uint8) == SENTINEL).all()), f"{k}: the rows behind the batch were written"
    return {k: t[:B].cpu().numpy() for k, t in bufs.items()}


def check_plan(z, sp, positions, partners, flips, scales):
    draws, spill = made_draws(z, sp, positions, partners, flips, scales)
    base, stage = (sp.arena.data_ptr() if sp.n_dev else 0), (spill.data_ptr() if spill is not None else 0)
    got = guarded_plan(sp, draws, spill)
    want = R.plan(base, stage, sp.img_off.cpu().numpy(), sp.frame_hw.cpu().numpy(), sp.rec_span.cpu().numpy(), sp.P2.cpu().numpy(), draws)
    assert [k for k, _, _ in kitti.PLAN_TABLES] == [k for k, _, _ in R.OUTPUTS]
    for k, dt, s in R.OUTPUTS:
        assert got[k].dtype == dt and got[k].shape == want[k].shape == (len(draws),) + s, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    # the restatement's pin: every address holds the frame's pixels, in the arena or in the staging buffer
    arena, staged = sp.arena.cpu().numpy(), (spill.cpu().numpy() if spill is not None else None)
    for b, (pos, par) in enumerate(zip(positions, partners)):
        for key, p in (("src", pos), ("src2", par)):
            if p < 0:
                assert got[key][b] == 0
                continue
            W, H = wh(z, p)
            a, n = int(got[key][b]), H * W * 3
            where, o = (arena, a - base) if p < sp.n_dev else (staged, a - stage)
            assert o % 16 == 0 and 0 <= o and o + n <= where.size and where[o:o + n].tobytes() == frame_pixels(p, W, H).tobytes(), (key, b, p)
    return got, draws, spill


SAME = {0: 5, 1: 4, 2: 3, 3: 0, 5: 1, 6: 8, 7: 6, 9: 11, 11: 10}  # partners of the primary's size (and camera)
PLAN_CASES = {
    "one_image": ([0], [-1], [0], [1.0]),
    "partners_flips_and_a_repeated_frame": ([6, 2, 6, 0, 7, 6], [8, -1, 6, 5, 6, -1], [1, 0, 1, 1, 0, 0], [0.9, 1.0, 1.1, 1.0, 1.2, 0.8]),
    "three_blocks": ([i % 12 for i in range(130)], [SAME.get(i % 12, -1) if i % 3 else -1 for i in range(130)], [i % 2 for i in range(130)],
                     [1.0 + 0.001 * (i % 7) for i in range(130)]),
    "frame_without_annotations": ([5, 0, 5], [-1, 5, 5], [1, 0, 0], [1.0, 0.9, 1.1]),
    "frame_with_55_objects": ([2, 0, 2], [-1, 2, 2], [1, 0, 1], [0.9, 1.1, 1.0]),
    "last_frame": ([11, 10, 11], [-1, 11, 11], [0, 1, 1], [1.0, 1.2, 0.8]),
    "hbm_primary_with_staged_partner_and_the_reverse": ([0, 5, 4, 8], [5, 0, 6, 3], [0, 1, 1, 0], [1.0, 0.9, 1.1, 1.0]),
}


@pytest.mark.parametrize("case", PLAN_CASES)
@pytest.mark.parametrize("placement", PLACEMENTS)  # n_dev = N, the boundary, n_dev = 0
@pytest.mark.parametrize("dataset", DATASETS)
def test_plan_kernel_against_the_restatement(trees, dataset, placement, case):
    z, sp = fixture(dataset), split_of(trees, dataset, placement)
    pos, par, fl, sc = PLAN_CASES[case]
    got, draws, spill = check_plan(z, sp, pos, par, fl, sc)
    n_dev = sp.n_dev
    assert got["mixed"].tolist() == [int(p >= 0) for p in par] and got["flip"].tolist() == list(fl)
    assert (draws[:, 16] >= 0).tolist() == [p >= n_dev for p in pos] and (draws[:, 17] >= 0).tolist() == [p >= 0 and p >= n_dev for p in par]
    if placement == "hbm":
        assert spill is None and (draws[:, 16:] == -1).all()
    if placement == "host":
        assert sp.arena.numel() == 0 and spill is not None
    if case == "frame_without_annotations":
        span = sp.rec_span.cpu().numpy()
        assert got["img_i"][0, 1] == 0 and got["img_i"][1, 3] == 0 and got["img_i"][0, 0] == span[6, 0] == got["img_i"][0, 2]
    if case == "frame_with_55_objects":
        assert got["img_i"][0, 1] == 55 and got["img_i"][1, 3] == 55 and got["img_i"][2, 1] == got["img_i"][2, 3] == 55
    if case == "last_frame":
        assert got["img_i"][0, 0] + got["img_i"][0, 1] == sp.rec.shape[0] and got["src"][0] == got["src2"][1] == got["src2"][2]
    if case == "hbm_primary_with_staged_partner_and_the_reverse" and placement == "boundary":
        assert draws[:, 16].tolist() == [-1, 0, -1, 2 * BIG] and draws[:, 17].tolist() == [0, -1, BIG, -1] and spill.numel() == 3 * BIG
        a, s = sp.arena.data_ptr(), spill.data_ptr()
        assert got["src"].tolist() == [a, s, a + 4 * BIG, s + 2 * BIG] and got["src2"].tolist() == [s, a, s + BIG, a + 3 * BIG]
    if case == "partners_flips_and_a_repeated_frame" and placement != "hbm":
        # frame 6, three times a primary and twice a partner, is staged once: 6, 8, 5, 7 behind the boundary; 2 and 0 too on the host
        assert spill.numel() == (4 if placement == "boundary" else 6) * BIG


@pytest.mark.parametrize("dataset", DATASETS)
def test_plan_refuses_bad_draws(trees, dataset):
    z, sp = fixture(dataset), split_of(trees, dataset, "boundary")
    N = len(sp)
    ok, spill = made_draws(z, sp, [0, 5, 6], [-1, 1, 8], [0, 1, 0], [1.0, 1.0, 0.9])
    assert ok[:, 16].tolist() == [-1, 0, BIG] and ok[:, 17].tolist() == [-1, -1, 2 * BIG] and spill.numel() == 3 * BIG
    bufs = {}
    for k, dt, s in kitti.PLAN_TABLES:
        bufs[k] = torch.empty(3, *s, dtype=dt, device=DEV)
        bufs[k].view(torch.uint8).fill_(SENTINEL)
    bad_tables = [
        (1, 0, N, "position"), (1, 0, -1, "position"), (1, 0, 2.5, "position"), (1, 1, N, "partner"), (1, 1, -2, "partner"),
        (0, 16, 0, "resident in the arena"),       # a staging offset on a resident position
        (1, 17, 16, "resident in the arena"),      # ... on a resident partner
        (1, 16, -1, "no staging offset"),          # none on a position of the host tier
        (2, 17, -1, "no staging offset"),          # ... on a partner of the host tier
        (0, 17, 0, "without a partner"),
        (1, 16, 8, "multiple of 16"), (2, 17, -16, "multiple of 16"), (2, 16, 16.5, "multiple of 16"),
        (2, 16, 3 * BIG, "outside the staging buffer"), (2, 17, 3 * BIG + 16, "outside the staging buffer"),
        (2, 17, 3 * BIG - 16, "ends outside"),      # starts inside, ends behind the buffer: refused from the host sizes
    ]
    for b, col, value, what in bad_tables:
        bad = ok.copy()
        bad[b, col] = value
        with pytest.raises(Y3DError, match=what):
            json3d.plan_batch(sp, bad, out=bufs, spill=spill)
    with pytest.raises(Y3DError, match="staging"):  # offsets without a buffer
        json3d.plan_batch(sp, ok, out=bufs)
    with pytest.raises(Y3DError, match="B = 0"):
        json3d.plan_batch(sp, np.zeros((0, 18), np.float64), out=bufs)
    with pytest.raises(Y3DError):
        json3d.plan_batch(sp, ok[:, :16].copy(), out=bufs, spill=spill)  # kitti's table
    with pytest.raises(Y3DError):
        json3d.plan_batch(sp, ok.astype(np.float32), out=bufs, spill=spill)
    with pytest.raises(Y3DError, match="staging buffer"):
        json3d.plan_batch(sp, ok, out=bufs, spill=spill.cpu())
    with pytest.raises(Y3DError, match="null"):
        y3d.lib().json3d_plan_batch(None, None, None, None, N, 0, None, None, 0, None, None, 1, None, None, None, None, None, None, None, None, None)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t.view(torch.uint8) == SENTINEL).all()), f"{k}: a refused batch wrote"
    json3d.plan_batch(sp, ok, out=bufs, spill=spill)  # and the table itself is fine
    torch.cuda.synchronize()
    assert not any(bool((t.view(torch.uint8) == SENTINEL).all()) for t in bufs.values())


# ------------------------------------------------------------------------------------------------------------ end to end
def resident_batch(sp, dataset, name, seed=None, **kw):
    mode, args, rseed, items = argset(fixture(dataset), name)
    np.random.seed(rseed if seed is None else seed)
    got = sp.build_batch(items, args, mode=mode, **kw)
    return got, np.random.get_state()[1].copy()


@pytest.mark.parametrize("name", RUNS)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dataset", DATASETS)
def test_resident_batch_equals_the_disk_batch(trees, dataset, placement, name):
    z = fixture(dataset)
    want, after = disk_batch(trees, dataset, name)
    got, state = resident_batch(split_of(trees, dataset, placement), dataset, name)
    assert np.array_equal(state, after)  # the same draws were consumed
    same_batch(got, want)
    assert "counts" in got and got["img"].dtype == torch.uint8
    assert got["mixed"].cpu().tolist() == [int(p >= 0) for p in z[f"{name}/partner"]]  # the draws are the recorded ones


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("img_mode", ["uint8", "float"])
@pytest.mark.parametrize("name", RUNS)
@pytest.mark.parametrize("dataset", DATASETS)
def test_image_modes_and_label_layouts_on_the_boundary(trees, dataset, name, img_mode, compact):
    want, after = disk_batch(trees, dataset, name, img_mode=img_mode, compact=compact)
    got, state = resident_batch(split_of(trees, dataset, "boundary"), dataset, name, img_mode=img_mode, compact=compact)
    assert np.array_equal(state, after)
    same_batch(got, want)
    assert ("counts" in got) != compact and got["img"].dtype == (torch.uint8 if img_mode == "uint8" else torch.float32)


@pytest.mark.parametrize("dataset", DATASETS)
def test_build_batch_dispatches_on_a_device_split(trees, dataset):
    sp = split_of(trees, dataset, "boundary")
    mode, args, seed, items = argset(fixture(dataset), "default")
    want, _ = disk_batch(trees, dataset, "default", img_mode="float", compact=True)
    np.random.seed(seed)
    same_batch(json3d.build_batch(sp, items, args, DEV, mode=mode, compact=True, img_mode="float"), want)
    with pytest.raises(Y3DError, match="lives on"):
        json3d.build_batch(sp, items, args, "cpu", mode=mode)
    with pytest.raises(Y3DError, match="test"):
        sp.build_batch(items, args, mode="test")
    with pytest.raises(Y3DError, match="test"):
        json3d.build_batch(sp, items, args, DEV, mode="test")
    with pytest.raises(Y3DError, match="test"):
        json3d.DeviceSplit(trees(dataset), dataset, mode="test", device=DEV)
    for bad in ([len(sp)], [0, -1], []):
        with pytest.raises(Y3DError, match="positions"):
            sp.build_batch(bad, args)


def two_sized_tree(root, dataset):
    """two frames of equal calibration and different sizes, without annotations -> the split JSON's path"""
    from PIL import Image
    K = [[500.0, 0.0, 100.0], [0.0, 500.0, 60.0], [0.0, 0.0, 1.0]]
    images = []
    for i, (W, H) in enumerate(((200, 120), (192, 120))):
        name = f"images/{i:04d}.png"
        os.makedirs(os.path.join(root, "images"), exist_ok=True)
        Image.fromarray(frame_pixels(i, W, H), "RGB").save(os.path.join(root, name))
        images.append({"id": i, "file_name": name, "calib": [r + [0.0] for r in K]} if dataset == "waymo" else {"id": i, "file_path": name, "K": K})
    raw = {"images": images, "annotations": [], "categories": [{"name": "car", "id": 0}]}
    path = os.path.join(root, "split.json")
    json.dump(raw, open(path, "w"))
    return path


@pytest.mark.parametrize("dataset", DATASETS)
def test_a_partner_of_another_size_is_refused_by_both_builders(tmp_path, dataset):
    path = two_sized_tree(str(tmp_path), dataset)
    args = kitti.data_args(mixup=1.0)
    cam = (100.0, 60.0, 500.0, 500.0)
    sizes = [(200, 120), (192, 120)]
    seed = None
    for s in range(200):  # the first seed under which frame 0 draws frame 1 as its partner (a dry run of the draws; no device work)
        np.random.seed(s)
        first = [True]

        def info(p):
            size, first[0] = (sizes[p] if first[0] else None), False
            return cam, 0, size

        if kitti.sample_augment(2, [0], info, args, "train", json3d.MAX_OBJS, json3d.RESOLUTION)[0]["partner"] == 1:
            seed = s
            break
    assert seed is not None
    np.random.seed(seed)
    with pytest.raises(Y3DError, match="partner"):
        json3d.build_batch(path, [0], args, DEV, dataset=dataset)
    after = np.random.get_state()[1].copy()
    for max_bytes, host_bytes in ((None, 0), (0, 1 << 20)):
        sp = json3d.DeviceSplit(path, dataset, device=DEV, max_bytes=max_bytes, host_bytes=host_bytes)
        assert sp.wh == sizes and sp.cam[0] == sp.cam[1] == cam
        np.random.seed(seed)
        with pytest.raises(Y3DError, match="partner 1 of position 0 has another size"):
            sp.build_batch([0], args)
        assert np.array_equal(np.random.get_state()[1], after)
        sp.build_batch([0], args, mode="val")  # and without the mixup the frame builds


@pytest.mark.parametrize("dataset", DATASETS)
def test_no_disk_after_load(tmp_path, trees, dataset):
    r = os.path.join(str(tmp_path), "tree")
    shutil.copytree(os.path.dirname(trees(dataset)), r)
    path = os.path.join(r, "split.json")
    z = fixture(dataset)
    mode, args, seed, items = argset(z, "camdis")
    vmode, vargs, vseed, vitems = argset(z, "val")
    wants = []
    for s in (seed, seed + 1):
        np.random.seed(s)
        wants.append(json3d.build_batch(path, items, args, DEV, dataset=dataset, mode=mode))
    want_val = json3d.build_batch(path, vitems, vargs, DEV, dataset=dataset, mode="val", compact=True)
    max_bytes, host_bytes, n_dev = PLACEMENTS["boundary"]
    sp = json3d.DeviceSplit(path, dataset, device=DEV, max_bytes=max_bytes, host_bytes=host_bytes, workers=3)
    assert sp.n_dev == n_dev
    shutil.rmtree(r)
    assert not os.path.exists(r)
    for s, want in zip((seed, seed + 1), wants):
        np.random.seed(s)
        same_batch(sp.build_batch(items, args, mode=mode), want)
    same_batch(json3d.build_batch(sp, vitems, vargs, DEV, mode="val", compact=True), want_val)


@pytest.mark.parametrize("dataset", DATASETS)
def test_both_budgets_are_checked_before_any_allocation(trees, dataset):
    path = trees(dataset)
    host = 4 * BIG + 3 * SMALL
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(Y3DError, match=f"{TOTAL} bytes.*{TOTAL - 1} bytes"):
        json3d.DeviceSplit(path, dataset, device=DEV, max_bytes=TOTAL - 1)  # no host tier: all in HBM, or refused
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(Y3DError, match=f"{host} bytes.*{host - 1} bytes"):
        json3d.DeviceSplit(path, dataset, device=DEV, max_bytes=5 * BIG, host_bytes=host - 1)
    assert torch.cuda.memory_allocated() == before
    sp = json3d.DeviceSplit(path, dataset, device=DEV, max_bytes=5 * BIG, host_bytes=host)  # exactly enough on both sides
    assert sp.n_dev == 5 and sp.nbytes == 5 * BIG and sp.host_nbytes == host and torch.cuda.memory_allocated() >= before + 5 * BIG
    assert sp.host_arena.is_pinned()


@pytest.mark.parametrize("dataset", DATASETS)
def test_ring_reuse_without_synchronising(trees, dataset):
    sp = split_of(trees, dataset, "boundary")
    mode, args, _, _ = argset(fixture(dataset), "default")
    items = [0, 4, 9, 6, 11]
    n = 2 * json3d.DeviceSplit.RING + 1
    got = []
    for k in range(n):  # more builds in flight than the ring has buffers, nothing waits in between
        np.random.seed(1000 + k)
        got.append(sp.build_batch(items, args, mode=mode))
    distinct = {g["ratio_pad"].cpu().numpy().tobytes() + g["calib"].cpu().numpy().tobytes() + g["center_3d"].cpu().numpy().tobytes() for g in got}
    assert len(distinct) > json3d.DeviceSplit.RING  # the draws differ, so a stale table would show
    for k in range(n):
        np.random.seed(1000 + k)
        same_batch(got[k], json3d.build_batch(trees(dataset), items, args, DEV, dataset=dataset, mode=mode))


@pytest.mark.parametrize("dataset", DATASETS)
def test_epoch_yields_every_position_once(trees, dataset):
    sp = split_of(trees, dataset, "boundary")
    args = kitti.data_args()
    np.random.seed(1)
    seen = [f for b in sp.epoch(5, args, mode="val", shuffle=True, seed=2) for f in b["im_file"]]
    assert sorted(seen) == sorted(f"{i:06d}.txt" for i in sp.ids)
    assert seen == [f"{sp.ids[p]:06d}.txt" for idx in kitti.epoch_indices(len(sp), 5, seed=2) for p in idx]
    assert [b["img"].shape[0] for b in sp.epoch(5, args, mode="val", drop_last=True)] == [5, 5]


# ------------------------------------------------------------------------------------------------------------ the validator
@pytest.fixture(scope="module")
def model_n3d():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml")).to(DEV)
    y3d.set_compute_dtype(before)
    return m.eval()


@pytest.mark.parametrize("dataset", DATASETS)
def test_validator3d_on_a_device_split(trees, dataset, model_n3d):
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    try:
        sp, path = split_of(trees, dataset, "boundary"), trees(dataset)
        on_split = val.Validator3d(model_n3d, sp, dataset=sp.dataset, batch=6, pictures=1)
        on_disk = val.Validator3d(model_n3d, path, dataset=dataset, batch=6, pictures=1)
        same_batch(on_split._batch([3, 4, 5, 6]), on_disk._batch([3, 4, 5, 6]))
        (n, calib, data), (n2, calib2, data2) = on_split._dataset(), on_disk._dataset()
        assert n == n2 == len(sp) and data is data2 is None and all(calib(p) == calib2(p) for p in range(n))
        assert all(on_split._projection()(p).tobytes() == on_disk._projection()(p).tobytes() for p in range(n))
        cached, disk = on_split(), on_disk()
        assert list(cached) == list(disk) and len(cached) >= 6
        for k in disk:
            assert np.array_equal(np.asarray(cached[k], np.float64), np.asarray(disk[k], np.float64), equal_nan=True), k
        assert list(on_split.results) == list(on_disk.results) == [f"{i:06d}.txt" for i in sp.ids]
        for f in on_disk.results:
            assert np.array_equal(np.array(on_split.results[f], np.float64), np.array(on_disk.results[f], np.float64), equal_nan=True), f
        assert sum(len(r) for r in on_split.results.values()) > 0 and on_split.seen == on_disk.seen == len(sp)
        assert len(on_split.pictures) == len(on_disk.pictures) == 1
        for k in ("labels", "preds", "bev"):
            assert on_split.pictures[0][k].dtype == np.uint8 and on_split.pictures[0][k].tobytes() == on_disk.pictures[0][k].tobytes(), k
        other = "omni3d" if dataset == "waymo" else "waymo"
        for wrong in (other, "kitti"):
            with pytest.raises(Y3DError, match=f"holds a {dataset} split"):
                val.Validator3d(model_n3d, sp, dataset=wrong)
    finally:
        y3d.set_compute_dtype(before)
