"""CPU: the host side of the KITTI label encoder — KITTI text parsing, the flipped calibration, the replayed random draws and the
refusals — against the reference's own records (tests/golden/kitti_labels.npz, minted by tools/make_golden_kitti_labels.py)."""
import os

import numpy as np
import pytest
import torch

from kitti_labels_tree import argset, fixture, frame_info_fn, write_tree

from yolov10_3d_amd import _lib
from yolov10_3d_amd import kitti
from yolov10_3d_amd._lib import Y3DError


def test_prototype_declared():
    assert "y3d_kitti_encode_labels" in _lib.parse_header()


def test_read_label_and_calib_match_the_reference_records(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    off = np.concatenate(([0], np.cumsum(z["rec_n"])))
    for i in range(len(z["rec_n"])):
        lab = kitti.read_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
        s = slice(off[i], off[i + 1])
        assert lab["type"] == list(z["rec_cls"][s]) and lab["level"] == list(z["rec_level"][s])
        assert lab["box2d"].dtype == np.float32 and lab["pos"].dtype == np.float32
        assert np.array_equal(lab["box2d"], z["rec_box"][s]) and np.array_equal(lab["pos"], z["rec_pos"][s])
        f64 = np.stack([lab[k] for k in ("truncation", "occlusion", "alpha", "h", "w", "l", "ry")], 1)
        assert f64.dtype == np.float64 and np.array_equal(f64, z["rec_f64"][s])
        P = kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt"))
        assert P.dtype == np.float32 and P.shape == (3, 4)
    # the unflipped P2 the reference projected with in its val run
    for b, item in enumerate(argset(z, "val")[3]):
        P = kitti.read_calib(os.path.join(root, "training/calib", f"{item:06d}.txt"))
        assert np.array_equal(P, z["val/P2"][b])


def test_flip_calib_matches_the_reference(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    for i, wh in enumerate(z["frame_wh"]):
        P = kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt"))
        got = kitti.flip_calib(P, wh)
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, z["flip_P2"][i], rtol=1e-9, atol=0, err_msg=f"frame {i}")
        np.testing.assert_allclose(kitti.calib_params(got), z["flip_c6"][i], rtol=1e-9, atol=0, err_msg=f"frame {i}")
    # and the flipped P2 of every recorded flipped sample
    for name in z["argsets"]:
        items = argset(z, str(name))[3]
        for b, item in enumerate(items):
            if z[f"{name}/flip"][b]:
                np.testing.assert_allclose(kitti.flip_calib(kitti.read_calib(os.path.join(root, "training/calib", f"{item:06d}.txt")),
                                                            z["frame_wh"][item]), z[f"{name}/P2"][b], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", ["default", "camdis", "val", "nomix"])
def test_sample_augment_replays_the_reference_draws(tmp_path, name):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    mode, args, seed, items = argset(z, name)
    np.random.seed(seed)
    draws = kitti.sample_augment(len(z["label_text"]), items, frame_info_fn(root, z), args, mode)
    for b, d in enumerate(draws):
        for k in ("mixed", "flip", "crop", "partner"):
            assert int(d[k]) == int(z[f"{name}/{k}"][b]), (name, b, k)
        assert d["scale"] == z[f"{name}/scale"][b]
        np.testing.assert_array_equal(d["center"], z[f"{name}/center"][b])
        np.testing.assert_allclose(d["trans"], z[f"{name}/trans"][b], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(d["trans_inv"], z[f"{name}/trans_inv"][b], rtol=1e-12, atol=1e-12)
    if name in ("default", "camdis"):
        assert any(d["mixed"] for d in draws) and any(d["crop"] for d in draws) and any(d["flip"] for d in draws)


def test_refusals(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    with pytest.raises(Y3DError):
        kitti.build_batch(root, [0, 1], kitti.data_args(load_depth_maps=True), "cuda")
    with pytest.raises(Y3DError):
        kitti.build_batch(root, [0, 1], kitti.data_args(), "cpu")
    lab = kitti.read_label(os.path.join(root, "training/label_2", "000000.txt"))
    P = kitti.read_calib(os.path.join(root, "training/calib", "000000.txt"))
    with pytest.raises(Y3DError):
        kitti.pack_labels([lab], [None], [P], [np.eye(2, 3)], [False], [1.0], [(1242, 375)], "cpu")
    cpu = {"rec": torch.zeros(1, 16, dtype=torch.float64), "img_i": torch.zeros(1, 7, dtype=torch.int32),
           "img_f": torch.zeros(1, 19, dtype=torch.float64), "mean_size": torch.zeros(3, 3, dtype=torch.float64)}
    with pytest.raises(Y3DError):
        kitti.encode_labels(cpu)


def test_label_records_layout():
    lab = {"type": ["Car", "Van", "Cyclist"], "truncation": np.array([0.0, 0.1, 0.2]), "occlusion": np.array([0.0, 1.0, 2.0]),
           "alpha": np.zeros(3), "h": np.array([1.5, 2.0, 1.7]), "w": np.ones(3), "l": np.full(3, 3.0), "ry": np.array([0.1, 0.2, 0.3]),
           "box2d": np.arange(12, dtype=np.float32).reshape(3, 4), "pos": np.arange(9, dtype=np.float32).reshape(3, 3)}
    r = kitti.label_records(lab)
    assert r.shape == (3, 16) and list(r[:, 0]) == [0, -1, 2]
    assert np.array_equal(r[:, 3:7], lab["box2d"]) and np.array_equal(r[:, 10:13], lab["pos"]) and np.array_equal(r[:, 13], lab["ry"])


def test_compact_dtype_rules():
    """collate_fn's torch.cat promotion: an empty image turns the batch's keys float64; depth is float32 only without crop / cam_dis"""
    M = 4
    st = {"cls": torch.zeros(2 * M, 1, dtype=torch.int64), "bboxes": torch.zeros(2 * M, 4, dtype=torch.float64),
          "center_2d": torch.zeros(2 * M, 2), "size_2d": torch.zeros(2 * M, 2), "center_3d": torch.zeros(2 * M, 2, dtype=torch.float64),
          "size_3d": torch.zeros(2 * M, 3, dtype=torch.float64), "depth": torch.zeros(2 * M, dtype=torch.float64),
          "heading_bin": torch.zeros(2 * M, dtype=torch.int64), "heading_res": torch.zeros(2 * M, dtype=torch.float64),
          "batch_idx": torch.zeros(2 * M)}
    c = kitti.compact_labels(st, [2, 1], [False, False], max_objs=M)
    assert c["cls"].dtype == torch.int64 and c["cls"].shape == (3, 1) and c["depth"].dtype == torch.float32
    assert c["heading_res"].dtype == torch.float32 and c["heading_bin"].dtype == torch.int64
    c = kitti.compact_labels(st, [2, 1], [True, False], max_objs=M)
    assert c["depth"].dtype == torch.float64
    c = kitti.compact_labels(st, [2, 0], [False, False], max_objs=M)
    assert c["cls"].dtype == torch.float64 and c["center_2d"].dtype == torch.float64 and c["batch_idx"].dtype == torch.float32
    c = kitti.compact_labels(st, [0, 0], [False, False], max_objs=M)
    assert c["bboxes"].shape == (0,) and c["bboxes"].dtype == torch.float32 and c["cls"].shape == (0,)
