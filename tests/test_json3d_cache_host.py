"""CPU: the host side of the two-tier resident split of json3d (json3d.DeviceSplit, resident.tier_layout): where the boundary between
the device arena and the pinned host arena falls, both byte budgets, the 18 columns of the draw table, the staging of a batch's
host-tier frames, the restated plan's calibration columns against `json3d.pack_labels`, the refusals that need no device, and the plan
kernel's declaration."""
import os

import numpy as np
import pytest

import json3d_cache_ref as R
from json3d_tree import DATASETS, RUNS, argset, fixture, write_tree

from yolov10_3d_amd import _lib, json3d, kitti, resident
from yolov10_3d_amd._lib import Y3DError

BIG, SMALL = 480 * 320 * 3, 384 * 256 * 3  # the fixture's two frame sizes in bytes, both multiples of 16
HW = [(320, 480)] * 9 + [(256, 384)] * 3  # (h, w) of the fixture's twelve frames
TOTAL = 9 * BIG + 3 * SMALL


def layout(hw, max_bytes, host_bytes):
    return resident.tier_layout(hw, max_bytes, host_bytes, None, "Split")


def test_fixture_frames_are_the_sizes_assumed_here():
    for dataset in DATASETS:
        assert [(int(h), int(w)) for w, h in fixture(dataset)["frame_wh"]] == HW
    assert BIG == 460800 and BIG % 16 == 0 and SMALL % 16 == 0


@pytest.mark.parametrize("max_bytes", [0, 1, BIG - 1, BIG, 5 * BIG, 5 * BIG + 1, 6 * BIG - 1, 9 * BIG, 9 * BIG + SMALL, TOTAL - 1, TOTAL, TOTAL + 5])
def test_tier_layout_against_the_sequential_walk(max_bytes):
    n_dev, off, padded, nbytes, host_off, host_nbytes = layout(HW, max_bytes, TOTAL)
    want_n, want_dev, want_host, used, spilled = R.tiers(HW, max_bytes)
    assert n_dev == want_n and nbytes == used and host_nbytes == spilled and nbytes + host_nbytes == TOTAL
    assert off.dtype == np.int64 and host_off.dtype == np.int64 and padded.dtype == np.int64
    assert off.tolist() == want_dev.tolist() and host_off.tolist() == want_host.tolist()
    assert padded.tolist() == [R.pad16(h * w * 3) for h, w in HW]
    assert ((off >= 0) == (np.arange(12) < n_dev)).all() and ((host_off >= 0) == (np.arange(12) >= n_dev)).all()


def test_boundary_is_where_the_cumulative_bytes_first_exceed_the_budget():
    assert layout(HW, 5 * BIG, TOTAL)[0] == 5 and layout(HW, 5 * BIG - 1, TOTAL)[0] == 4 and layout(HW, 0, TOTAL)[0] == 0
    n_dev, off, _, nbytes, host_off, host_nbytes = layout(HW, 5 * BIG, TOTAL)
    assert off.tolist() == [0, BIG, 2 * BIG, 3 * BIG, 4 * BIG] + [-1] * 7 and nbytes == 5 * BIG
    assert host_off.tolist() == [-1] * 5 + [0, BIG, 2 * BIG, 3 * BIG, 4 * BIG, 4 * BIG + SMALL, 4 * BIG + 2 * SMALL]
    assert host_nbytes == 4 * BIG + 3 * SMALL


def test_a_smaller_later_frame_that_would_still_fit_goes_to_the_host():
    hw = [(10, 10), (100, 100), (10, 10), (4, 4)]  # 300 -> 304 bytes, 30000, 304, 48 -> 48
    n_dev, off, padded, nbytes, host_off, host_nbytes = layout(hw, 1000, 1 << 20)
    assert padded.tolist() == [304, 30000, 304, 48]
    assert n_dev == 1 and off.tolist() == [0, -1, -1, -1] and nbytes == 304  # frames 2 and 3 would fit the 696 bytes left
    assert host_off.tolist() == [-1, 0, 30000, 30304] and host_nbytes == 30352


def test_both_tiers_align_their_offsets_to_16():
    hw = [(3, 5), (7, 11), (1, 1), (13, 3), (2, 9), (5, 5)]  # 45, 231, 3, 117, 54, 75 bytes: none a multiple of 16
    n_dev, off, padded, nbytes, host_off, host_nbytes = layout(hw, 48 + 240 + 16, 1 << 20)
    assert n_dev == 3 and padded.tolist() == [48, 240, 16, 128, 64, 80]
    assert off.tolist() == [0, 48, 288, -1, -1, -1] and host_off.tolist() == [-1, -1, -1, 0, 128, 192]
    assert all(o % 16 == 0 for o in off[:3]) and all(o % 16 == 0 for o in host_off[3:]) and nbytes == 304 and host_nbytes == 272


def test_budgets_exactly_enough_and_one_byte_short():
    dev, host = 5 * BIG, 4 * BIG + 3 * SMALL
    assert layout(HW, dev, host)[0] == 5  # exactly enough on both sides
    assert layout(HW, TOTAL, 0)[0] == 12
    with pytest.raises(Y3DError, match=f"{host} bytes.*{host - 1} bytes"):  # one byte short on the host side
        layout(HW, dev, host - 1)
    with pytest.raises(Y3DError, match=f"{TOTAL} bytes.*{TOTAL - 1} bytes"):  # one byte short on the device side, no host tier
        layout(HW, TOTAL - 1, 0)
    # one byte short on the device side with a host tier: the frame that no longer fits, and every later one, must fit the host's
    with pytest.raises(Y3DError, match=f"{host + BIG} bytes.*{host} bytes"):
        layout(HW, dev - 1, host)
    assert layout(HW, dev - 1, host + BIG)[0] == 4


def test_without_a_host_tier_the_layout_is_arena_layout():
    for hw in (HW, [(3, 5), (7, 11), (1, 1)]):
        off, padded, nbytes = resident.arena_layout(hw, 1 << 30, None, "Split")
        n_dev, toff, tpadded, tnbytes, host_off, host_nbytes = layout(hw, 1 << 30, 0)
        assert n_dev == len(hw) and toff.tolist() == off.tolist() and tpadded.tolist() == padded.tolist() and tnbytes == nbytes
        assert toff.dtype == off.dtype and host_off.tolist() == [-1] * len(hw) and host_nbytes == 0
    with pytest.raises(Y3DError) as mine:
        layout(HW, 1000, 0)
    with pytest.raises(Y3DError) as theirs:
        resident.arena_layout(HW, 1000, None, "Split")
    assert str(mine.value) == str(theirs.value)


def test_staging_holds_a_frame_used_three_times_once():
    padded = np.array([R.pad16(h * w * 3) for h, w in HW])
    # rows (primary, partner): 7 as a primary, as a partner, as a primary again; 6 once; 2 and 0 live in the arena
    rows = [(7, -1), (2, 7), (7, 6), (0, -1)]
    at, nbytes = resident.stage_layout([p for r in rows for p in r], 5, padded)
    assert at == {7: 0, 6: BIG} and nbytes == 2 * BIG
    assert (at, nbytes) == R.staging([r[0] for r in rows], [r[1] for r in rows], 5, HW)
    assert resident.stage_layout([0, -1, 4, 3], 5, padded) == ({}, 0)  # nothing of the host tier: no buffer
    at, nbytes = resident.stage_layout([11, 9, 11, 5], 0, padded)  # all on the host, two sizes
    assert at == {11: 0, 9: SMALL, 5: 2 * SMALL} and nbytes == 2 * SMALL + BIG


def made_draws(positions, partners, flips, scales):
    out = []
    for pos, par, f, s in zip(positions, partners, flips, scales):
        size = np.array(HW[pos][::-1], np.float64)
        tr, inv = kitti.get_affine_transform(size / 2 + np.array([7.0, -3.0]) * (s != 1.0), size * s, json3d.RESOLUTION, inv=True)
        out.append(dict(partner=par, mixed=par >= 0, flip=bool(f), scale=s, trans=tr, trans_inv=inv))
    return out


def test_draw_table_has_kittis_sixteen_columns_and_two_staging_offsets():
    assert json3d._DRAW_W == R.DRAW_W == 18 and kitti._DRAW_W == 16
    pos, par, fl, sc = [7, 2, 7, 0, 11], [-1, 7, 6, -1, 10], [0, 1, 1, 0, 1], [1.0, 0.9, 1.1, 1.0, 1.2]
    draws = made_draws(pos, par, fl, sc)
    staged = {7: 0, 6: BIG, 11: 2 * BIG, 10: 2 * BIG + SMALL}
    t = json3d.draw_table(pos, draws, staged)
    assert t.dtype == np.float64 and t.shape == (5, 18) and t.flags["C_CONTIGUOUS"]
    assert t[:, :16].tobytes() == kitti.draw_table(pos, draws).tobytes()
    assert t[:, 16].tolist() == [0, -1, 0, -1, 2 * BIG] and t[:, 17].tolist() == [-1, 0, BIG, -1, 2 * BIG + SMALL]
    want = R.draw_rows(pos, par, fl, sc, [d["trans"] for d in draws], [d["trans_inv"] for d in draws], staged)
    assert t.tobytes() == want.tobytes()
    # without a host tier every offset is -1, the missing partner's too
    assert (json3d.draw_table(pos, draws, {})[:, 16:] == -1).all()


@pytest.mark.parametrize("dataset", DATASETS)
def test_restated_calibration_columns_equal_what_pack_labels_uploads(tmp_path, monkeypatch, dataset):
    """img_f of the restated plan over the split's P2 table (as read in float64; flip_calib's float32 widened) against img_f of
    `json3d.pack_labels` given what `json3d.build_batch` gives it, for every recorded run: flipped and unflipped rows"""
    z = fixture(dataset)
    sp = json3d.Split(write_tree(str(tmp_path), z, dataset), dataset)
    N = len(sp)
    wh = [tuple(int(v) for v in s) for s in z["frame_wh"]]
    P2 = np.stack([np.stack((sp.P2(i).reshape(12), json3d.flip_calib(sp.P2(i), wh[p]).astype(np.float64).reshape(12)))
                   for p, i in enumerate(sp.ids)])
    assert P2.dtype == np.float64 and P2.shape == (N, 2, 12)
    n_obj = [len(sp.records(i)) for i in sp.ids]
    span = resident.span_table(n_obj)
    assert n_obj[2] == 55 and n_obj[5] == 0 and n_obj[11] == 45 and tuple(span[5]) == (tuple(span[6])[0], 0)
    hw = np.array([(h, w) for w, h in wh], np.int32)
    monkeypatch.setattr(kitti, "upload", lambda a, device, dtype=None: np.ascontiguousarray(a))  # what would be uploaded, kept on the host
    seen = set()
    for name in RUNS:
        items = argset(z, name)[3]
        partners, flips = [int(p) for p in z[f"{name}/partner"]], [bool(f) for f in z[f"{name}/flip"]]
        seen |= set(flips)
        draws = R.draw_rows(items, partners, flips, z[f"{name}/scale"], z[f"{name}/trans"], z[f"{name}/trans_inv"], {})
        p = R.plan(0, 0, np.zeros(N, np.int64), hw, span, P2, draws)
        rec = lambda pos: sp.records(sp.ids[pos])
        P2s = [json3d.flip_calib(sp.P2(sp.ids[i]), wh[i]) if f else sp.P2(sp.ids[i]) for i, f in zip(items, flips)]  # as build_batch
        packed = json3d.pack_labels([rec(i) for i in items], [rec(q) if q >= 0 else None for q in partners], P2s, list(z[f"{name}/trans"]),
                                    flips, list(z[f"{name}/scale"]), [wh[i] for i in items], "cuda", dataset)
        assert packed["img_f"].dtype == np.float64 and p["img_f"][:, :12].tobytes() == packed["img_f"][:, :12].tobytes(), name
        assert p["img_f"].tobytes() == packed["img_f"].tobytes(), name
        assert np.array_equal(p["img_i"][:, [1, 3, 4, 5, 6]], packed["img_i"][:, [1, 3, 4, 5, 6]])
        split_rec = np.concatenate([rec(q) for q in range(N)])
        for b in range(len(items)):
            for first, n in ((0, 1), (2, 3)):
                mine = split_rec[p["img_i"][b, first]:p["img_i"][b, first] + p["img_i"][b, n]]
                theirs = packed["rec"][packed["img_i"][b, first]:packed["img_i"][b, first] + packed["img_i"][b, n]]
                assert mine.tobytes() == theirs.tobytes(), (name, b, first)
    assert seen == {False, True}


def test_refusals_that_need_no_device(tmp_path):
    nowhere = os.path.join(str(tmp_path), "no_such_tree", "split.json")
    for dataset in DATASETS:
        with pytest.raises(Y3DError, match="HIP device"):
            json3d.DeviceSplit(nowhere, dataset, device="cpu")
        with pytest.raises(Y3DError, match="test"):
            json3d.DeviceSplit(nowhere, dataset, mode="test", device="cuda")
    with pytest.raises(Y3DError, match="dataset"):
        json3d.DeviceSplit(nowhere, "kitti", device="cuda")
    with pytest.raises(Y3DError, match="host_bytes"):
        json3d.DeviceSplit(nowhere, "waymo", device="cuda", host_bytes=-1)
    assert not os.path.exists(os.path.dirname(nowhere))


def test_plan_kernel_is_declared():
    protos = _lib.parse_header()
    assert "y3d_json3d_plan_batch" in protos
    ret, argtypes = protos["y3d_json3d_plan_batch"]
    # 4 frame tables, N, n_dev, arena, staging buffer and its size, draws (host, device), B, 8 outputs, stream
    assert len(argtypes) == 21
    import ctypes
    assert argtypes[8] is ctypes.c_int64 and argtypes[4] is argtypes[5] is ctypes.c_int
    src = open(_lib.HEADER).read()
    assert "Y3D_JSON3D_DRAW_W = 18" in src
