"""CPU: the host side of json3d (Waymo / Omni3D batches): the JSON readers against the reference's parse of the same split
(tests/golden/waymo_labels.npz, omni3d_labels.npz), the mirrored calibration, the replay of the recorded random draws, the yaw of an
Omni3D rotation matrix against scipy, and the refusal to build a batch anywhere but on a HIP device."""
import json

import numpy as np
import pytest

from json3d_tree import DATASETS, RUNS, argset, fixture, write_tree

import yolov10_3d_amd as y3d
from yolov10_3d_amd import json3d, kitti


@pytest.mark.parametrize("dataset", DATASETS)
def test_reader_parses_as_the_reference(tmp_path, dataset):
    z = fixture(dataset)
    sp = json3d.read_split(write_tree(str(tmp_path), z, dataset), dataset)
    assert sp.ids == [int(i) for i in z["img_id"]] == sorted(sp.ids) and len(sp) == 12
    raw = json.loads(str(z["json_text"]))
    assert [im["id"] for im in raw["images"]] != sp.ids  # the JSON lists them out of order
    rows = np.concatenate([sp.records(i) for i in sp.ids])
    assert rows.dtype == np.float64 and rows.shape == (int(z["rec_n"].sum()), json3d.REC_W)
    assert [len(sp.records(i)) for i in sp.ids] == list(z["rec_n"]) and 0 in z["rec_n"] and z["rec_n"].max() > 50
    want = z["rec"]
    ry = 11
    cols = [c for c in range(18) if c != ry]
    assert np.array_equal(rows[:, cols], want[:, cols])  # class map, float32 box, float64 dims / position, the flags
    assert np.array_equal(rows[:, 1:5], rows[:, 1:5].astype(np.float32)) and not np.array_equal(rows[:, 8:11], rows[:, 8:11].astype(np.float32))
    np.testing.assert_allclose(rows[:, ry], want[:, ry], rtol=0, atol=0 if dataset == "waymo" else 1e-13)
    assert not rows[:, 18:].any() and set(np.unique(rows[:, 0])) == {-1.0, 0.0, 1.0, 2.0}
    for pos, i in enumerate(sp.ids):
        P = sp.P2(i)
        assert P.dtype == np.float64 and P.shape == (3, 4) and np.array_equal(P, z["P2"][pos])
        if dataset == "omni3d":
            assert not P[:, 3].any()
        assert sp.file(i).startswith(str(tmp_path)) and "waymo/images" not in sp.file(i)
    if dataset == "omni3d":
        assert sp.id2cls == {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Traffic Cone"}
    else:
        assert sp.id2cls == json3d.WAYMO_DATA_ID2CLS


def test_overfit_keeps_the_ids_below_50(tmp_path):
    z = fixture("waymo")
    sp = json3d.Split(write_tree(str(tmp_path), z, "waymo"), "waymo", overfit=True)
    assert sp.ids == [int(i) for i in z["img_id"] if i < 50] and 0 < len(sp) < 12
    assert all(a["image_id"] < 50 for anns in sp.anns.values() for a in anns)


@pytest.mark.parametrize("dataset", DATASETS)
def test_flip_calib_of_a_float64_calibration(dataset):
    z = fixture(dataset)
    for pos in range(12):
        got = json3d.flip_calib(z["P2"][pos], z["frame_wh"][pos])
        assert got.dtype == np.float32
        np.testing.assert_allclose(got, z["flip_P2"][pos], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", RUNS)
@pytest.mark.parametrize("dataset", DATASETS)
def test_sample_augment_replays_the_recorded_draws(tmp_path, dataset, name):
    z = fixture(dataset)
    sp = json3d.read_split(write_tree(str(tmp_path), z, dataset), dataset)
    mode, args, seed, items = argset(z, name)
    np.random.seed(seed)
    state = np.random.get_state()[1].copy()
    draws = []
    for pos in items:
        first = [True]

        def info(p, _first=first, _size=tuple(int(v) for v in z["frame_wh"][pos])):
            size, _first[0] = (_size if _first[0] else None), False
            P = sp.P2(sp.ids[p])
            return (P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(sp.records(sp.ids[p])), size

        draws += kitti.sample_augment(len(sp), [pos], info, args, mode, json3d.MAX_OBJS, json3d.RESOLUTION)
    for k in ("mixed", "flip", "crop", "partner"):
        assert [int(d[k]) for d in draws] == list(z[f"{name}/{k}"]), k
    np.testing.assert_allclose([d["scale"] for d in draws], z[f"{name}/scale"], rtol=0, atol=0)
    for k in ("center", "trans", "trans_inv"):
        np.testing.assert_allclose(np.stack([d[k] for d in draws]), z[f"{name}/{k}"], rtol=1e-12, atol=1e-12, err_msg=k)
    assert np.array_equal(np.random.get_state()[1], state) == (mode == "val")


def test_yaw_from_matrix_against_scipy():
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(5)
    mats = list(Rot.random(200, random_state=7).as_matrix())
    mats += [Rot.from_euler("xyz", [0.3, s * (np.pi / 2 - 1e-5), -0.2]).as_matrix() for s in (-1, 1)]  # next to the gimbal lock
    mats += [m + rng.normal(0, 1e-6, (3, 3)) for m in mats[:50]]  # not quite orthonormal, as a JSON's rounded digits
    z = fixture("omni3d")
    mats += [np.array(a["R_cam"]) for a in json.loads(str(z["json_text"]))["annotations"][:60]]
    for m in mats:
        want = Rot.from_matrix(m).as_euler("xyz")[1]
        assert abs(json3d.yaw_from_matrix(m) - want) < 1e-12, (m, want)


def test_constants_and_errors(tmp_path):
    assert json3d.RESOLUTION == (960, 640) and json3d.MAX_OBJS == 50
    assert np.asarray(json3d.WAYMO_CLS_MEAN_SIZE).shape == (3, 3) and json3d.OMNI3D_CLS_MEAN_SIZE == kitti.CLS_MEAN_SIZE
    z = fixture("waymo")
    path = write_tree(str(tmp_path), z, "waymo")
    args = kitti.data_args()
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        json3d.build_batch(path, [0, 1], args, "cpu", dataset="waymo")
    with pytest.raises(y3d.Y3DError, match="test split"):
        json3d.build_batch(path, [0, 1], args, "cuda", dataset="waymo", mode="test")
    with pytest.raises(y3d.Y3DError, match="dataset"):
        json3d.build_batch(path, [0, 1], args, "cuda", dataset="nuscenes")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        json3d.pack_labels([np.zeros((0, json3d.REC_W))], [None], [np.eye(3, 4)], [np.eye(2, 3)], [0], [1.0], [(480, 320)], "cpu", "waymo")
    assert "y3d_json3d_encode_labels" in y3d.lib().protos
