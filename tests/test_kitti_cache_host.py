"""CPU: the host side of the resident KITTI split (kitti.DeviceSplit): the epoch's index lists, the refusal of a host device before any
file is read, and the plan kernel's declaration."""
import os

import pytest

from yolov10_3d_amd import _lib, kitti
from yolov10_3d_amd._lib import Y3DError


@pytest.mark.parametrize("n,batch", [(12, 4), (13, 4), (7481, 32), (3, 8), (1, 1)])
def test_epoch_covers_every_position_once(n, batch):
    ep = kitti.epoch_indices(n, batch)
    assert sorted(i for b in ep for i in b) == list(range(n))
    assert all(len(b) == batch for b in ep[:-1]) and 1 <= len(ep[-1]) <= batch
    assert len(ep) == -(-n // batch)
    assert all(type(i) is int for b in ep for i in b)


def test_epoch_is_reproducible_and_seeded():
    a, b, c = kitti.epoch_indices(100, 8, seed=3), kitti.epoch_indices(100, 8, seed=3), kitti.epoch_indices(100, 8, seed=4)
    assert a == b and a != c
    assert kitti.epoch_indices(100, 8) == kitti.epoch_indices(100, 8, seed=0)
    assert a != kitti.epoch_indices(100, 8, shuffle=False)


def test_epoch_leaves_the_global_generator_alone():
    import numpy as np
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    kitti.epoch_indices(50, 4, seed=9)
    assert np.array_equal(np.random.get_state()[1], state)


def test_epoch_drop_last():
    full, cut = kitti.epoch_indices(13, 4, seed=1), kitti.epoch_indices(13, 4, seed=1, drop_last=True)
    assert len(full) == 4 and len(full[-1]) == 1 and cut == full[:3]
    assert kitti.epoch_indices(12, 4, drop_last=True) == kitti.epoch_indices(12, 4)  # nothing short to drop
    assert kitti.epoch_indices(3, 8, drop_last=True) == []
    assert kitti.epoch_indices(0, 8) == []


def test_epoch_without_shuffle_is_consecutive():
    assert kitti.epoch_indices(10, 4, shuffle=False) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert kitti.epoch_indices(10, 4, shuffle=False, seed=7, drop_last=True) == [[0, 1, 2, 3], [4, 5, 6, 7]]


@pytest.mark.parametrize("batch", [0, -1])
def test_epoch_refuses_an_empty_batch(batch):
    with pytest.raises(Y3DError, match="batch"):
        kitti.epoch_indices(10, batch)


def test_device_split_refuses_a_host_device_before_reading(tmp_path):
    nowhere = os.path.join(str(tmp_path), "no_such_tree")
    assert not os.path.exists(nowhere)
    with pytest.raises(Y3DError, match="HIP device"):
        kitti.DeviceSplit(nowhere, device="cpu")
    with pytest.raises(Y3DError, match="HIP device"):
        kitti.DeviceSplit(os.path.join(nowhere, "ImageSets", "val.txt"), mode="val", device="cpu", max_bytes=1)
    assert not os.path.exists(nowhere)


def test_plan_kernel_is_declared():
    protos = _lib.parse_header()
    assert "y3d_kitti_plan_batch" in protos
    ret, argtypes = protos["y3d_kitti_plan_batch"]
    assert len(argtypes) == 18  # 4 frame tables, N, arena, draws (host, device), B, 8 outputs, stream
