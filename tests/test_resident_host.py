"""CPU: what the resident splits and the batch builders share (yolov10_3d_amd/resident.py and the helpers of kitti.py): the arena
layout and its byte budget, the span table, the re-exports, the refusals of a plan kernel's tables, KITTI's draw table, and the flip fit
behind both `flip_calib`s against the arrays recorded before the two were joined."""
import numpy as np
import pytest
import torch

import kitti_cache_ref as R
from kitti_labels_tree import fixture, frame_info_fn, write_tree

from yolov10_3d_amd import json3d, kitti, resident
from yolov10_3d_amd._lib import Y3DError

HW = [(375, 1242), (370, 1224), (1, 1), (5, 3)]  # 14, 0, 13 and 3 bytes short of a multiple of 16
PADDED = [(h * w * 3 + 15) // 16 * 16 for h, w in HW]


def test_arena_layout_pads_every_frame_to_16_bytes():
    offsets, padded, nbytes = resident.arena_layout(HW, sum(PADDED), torch.device("cpu"), "Some")  # the budget met exactly
    assert padded.tolist() == PADDED and nbytes == sum(PADDED)
    assert offsets.dtype == np.int64 and offsets.tolist() == [sum(PADDED[:i]) for i in range(len(HW))]
    assert [p - h * w * 3 for p, (h, w) in zip(PADDED, HW)] == [14, 0, 13, 3]


def test_arena_layout_refuses_one_byte_less():
    need = sum(PADDED)
    with pytest.raises(Y3DError, match=f"^Some: the 4 decoded frames need {need} bytes, {need - 1} bytes are allowed"):
        resident.arena_layout(HW, need - 1, torch.device("cpu"), "Some")


def test_span_table():
    span = resident.span_table([0, 3, 0, 55])
    assert span.dtype == np.int32 and span.tolist() == [[0, 0], [0, 3], [3, 0], [3, 55]]


def test_kitti_re_exports_the_shared_objects():
    assert kitti.epoch_indices is resident.epoch_indices and kitti.fill_arena is resident.fill_arena and kitti.DrawRing is resident.DrawRing
    assert issubclass(kitti.DeviceSplit, resident.ResidentSplit)


TABLES = (("a", torch.int32, (2,)), ("b", torch.float64, ()))
CPU = torch.device("cpu")


def test_check_plan_passes_a_good_table_through():
    draws = np.zeros((3, 16))
    host, dev, out = resident.check_plan(draws, 16, CPU, TABLES, None, None)
    assert host.data_ptr() == draws.ctypes.data and dev.shape == (3, 16)
    assert {k: (tuple(t.shape), t.dtype) for k, t in out.items()} == {"a": ((3, 2), torch.int32), "b": ((3,), torch.float64)}
    mine = {"a": torch.empty(5, 2, dtype=torch.int32), "b": torch.empty(3, dtype=torch.float64)}
    assert resident.check_plan(draws, 16, CPU, TABLES, dev, mine)[2] is mine  # longer outputs are taken as they are


@pytest.mark.parametrize("draws,match", [
    (np.zeros((3, 16), np.float32), r"contiguous \(B, 16\) float64 table on the host, got \(3, 16\) torch.float32"),
    (np.zeros((3, 15)), r"contiguous \(B, 16\) float64 table on the host, got \(3, 15\) torch.float64"),
    (np.zeros((3, 32))[:, ::2], r"contiguous \(B, 16\) float64 table on the host, got \(3, 16\) torch.float64"),
])
def test_check_plan_refuses_a_bad_draw_table(draws, match):
    with pytest.raises(Y3DError, match="^plan_batch: the draws are a " + match):
        resident.check_plan(draws, 16, CPU, TABLES, None, None)


def test_check_plan_refuses_a_short_output():
    out = {"a": torch.empty(2, 2, dtype=torch.int32), "b": torch.empty(3, dtype=torch.float64)}
    with pytest.raises(Y3DError, match=r"^plan_batch: output a must be a contiguous \(3\+, 2\) torch.int32 tensor on cpu"):
        resident.check_plan(np.zeros((3, 16)), 16, CPU, TABLES, None, out)
    with pytest.raises(Y3DError, match="^plan_batch: the device copy of the draws must match the host table"):
        resident.check_plan(np.zeros((3, 16)), 16, CPU, TABLES, torch.zeros(2, 16, dtype=torch.float64), None)


def test_kitti_draw_table_equals_the_restated_rows(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    n = len(z["label_text"])
    items = [i % n for i in range(2 * n)]
    np.random.seed(11)
    draws = kitti.sample_augment(n, items, frame_info_fn(root, z), kitti.data_args())
    assert any(d["mixed"] for d in draws) and any(d["flip"] for d in draws) and any(d["crop"] for d in draws)
    got = kitti.draw_table(items, draws)
    want = R.draw_rows(items, [d["partner"] for d in draws], [d["flip"] for d in draws], [d["scale"] for d in draws],
                       [d["trans"] for d in draws], [d["trans_inv"] for d in draws])
    assert got.dtype == np.float64 and got.shape == (2 * n, 16) and got.tobytes() == want.tobytes()


# recorded with kitti.flip_calib / json3d.flip_calib before the two shared one fit: a KITTI P2 over a 1242 x 375 image, and a float64
# Waymo-style P2 (with a translation column) over a 1920 x 1280 image
KITTI_P2 = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]
KITTI_FLIPPED = [[721.5377197265625, 0.0, 632.440673828125, -44.85728073120117], [0.0, 721.5377197265625, 172.85400390625, 0.2163791060447693],
                 [0.0, 0.0, 0.0, 0.0027458840049803257]]
WAYMO_P2 = [[2055.556149, 0.0, 939.657469, 12.5], [0.0, 2055.556149, 641.072182, -3.25], [0.0, 0.0, 1.0, 0.001]]
WAYMO_FLIPPED = [[2055.55615234375, 0.0, 980.342529296875, -12.5], [0.0, 2055.55615234375, 641.0722045898438, -3.25],
                 [0.0, 0.0, 0.0, 0.0010000000474974513]]


def test_both_flip_calibs_return_the_recorded_arrays():
    got = kitti.flip_calib(np.array(KITTI_P2, np.float32), (1242, 375))
    assert got.dtype == np.float32 and got.shape == (3, 4) and got.tobytes() == np.array(KITTI_FLIPPED, np.float32).tobytes()
    got = json3d.flip_calib(np.array(WAYMO_P2, np.float64), (1920, 1280))
    assert got.dtype == np.float32 and got.shape == (3, 4) and got.tobytes() == np.array(WAYMO_FLIPPED, np.float32).tobytes()
