"""CPU: the label decode (`kitti.decode_batch_device`, `y3d_decode_labels`) without a device — the float64 restatement of
tests/decode_batch_ref.py against the reference's own `decode_batch` (tests/golden/decode_batch.npz, minted by
tools/make_golden_decode_batch.py), the conditions that fixture was minted under, every refusal of the wrappers and of the C entry
(which checks before it launches, so no device is needed to be refused), and the validator's `pictures` argument.

The restatement equals the reference to the bit in every run but KITTI's `camdis`: `camera_dis_to_rect` squares the float32 `fu` in
float32 (kitti_utils.py:295, `self.fu ** 2`), the one place where decode_batch's arithmetic leaves float64, and the restatement (like
the kernels) squares it in float64.  That run is held to the bound the reference comparison on the device uses."""
import inspect

import numpy as np
import pytest
import torch

import decode_batch_ref as D

import yolov10_3d_amd as y3d
from yolov10_3d_amd import json3d, kitti, plot, val

CASES = [(ds, run, undo) for ds, runs in D.RUNS.items() for run in runs for undo in (True, False)]


@pytest.mark.parametrize("dataset,run,undo", CASES)
def test_restatement_reproduces_the_reference(dataset, run, undo):
    I = D.fixture_inputs(dataset, run)
    rows, c3, ci, counts = D.decode(I["lab"], None, I["ori_shape"], I["calib6"], I["ratio_pad"], I["trans_inv"], I["P2"], I["mean_size"], undo,
                                    I["cam_dis"], 50)
    want, want_counts = D.fixture_rows(dataset, run, undo)
    assert counts.tolist() == want_counts.tolist() and counts.max() <= 50
    got = D.ragged(rows, counts)
    assert np.array_equal(got[:, 0], want[:, 0]) and (got[:, 13] == 1).all()
    print(f"{dataset}/{run} undo={undo}: max |restatement - reference| per column {np.abs(got - want).max(0)}")
    if I["cam_dis"]:  # the float32 fu ** 2 of camera_dis_to_rect: the device comparison's bound
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
        other = [c for c in range(14) if c not in (9, 10, 11)]
        np.testing.assert_allclose(got[:, other], want[:, other], rtol=0, atol=1e-9)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    if run == "val" and undo:
        g = D.fixture()
        pick = g[f"{dataset}/val/corner_rows"]
        assert len(pick) >= 10
        np.testing.assert_allclose(D.ragged(c3, counts)[pick], g[f"{dataset}/val/corners3d"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(D.ragged(ci, counts)[pick], g[f"{dataset}/val/corners_img"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dataset", list(D.RUNS))
def test_fixture_meets_the_conditions_it_was_minted_under(dataset):
    z = D.label_fixture(dataset)
    lines = [len(str(t).splitlines()) for t in z["label_text"]] if dataset == "kitti" else [int(n) for n in z["rec_n"]]
    fullest = int(np.argmax(lines))
    empty, classes, angle_wraps, high, low, margin = 0, set(), 0, 0, 0, np.inf
    for run in D.RUNS[dataset]:
        I = D.fixture_inputs(dataset, run)
        rows, counts = D.fixture_rows(dataset, run, True)
        assert len(rows) == counts.sum() == len(I["lab"]["cls"])
        if run in ("val", "default"):
            assert fullest in I["items"] and counts[I["items"].index(fullest)] == counts.max()
        empty += int((counts == 0).sum())
        classes |= set(rows[:, 0].astype(int).tolist())
        img = I["lab"]["batch_idx"].astype(np.int64)
        ang = I["lab"]["heading_bin"].astype(np.float64) * (2 * np.pi / 12) + I["lab"]["heading_res"].astype(np.float64)
        alpha = np.where(ang > np.pi, ang - 2 * np.pi, ang)
        ry = alpha + np.arctan2(I["lab"]["bboxes"].astype(np.float64)[:, 0] * I["ori_shape"][img, 1] - I["calib6"][img, 0], I["calib6"][img, 2])
        angle_wraps, high, low = angle_wraps + int((ang > np.pi).sum()), high + int((ry > np.pi).sum()), low + int((ry < -np.pi).sum())
        margin = min([margin] + np.abs(ang - np.pi).tolist() + np.abs(ry - np.pi).tolist() + np.abs(ry + np.pi).tolist())
        # the recorded rows wrapped where these numbers say
        np.testing.assert_allclose(rows[:, 1], alpha, rtol=0, atol=1e-12)
        wrapped = np.where(ry > np.pi, ry - 2 * np.pi, np.where(ry < -np.pi, ry + 2 * np.pi, ry))
        np.testing.assert_allclose(rows[:, 12], wrapped, rtol=0, atol=1e-9)
    assert empty >= 1 and classes == {0, 1, 2} and angle_wraps >= 1 and high >= 1 and low >= 1, (empty, classes, angle_wraps, high, low)
    assert margin >= 1e-6, margin


def test_crafted_rows_wrap_where_they_should():
    lab, ori, c6, P2, rp, inv, names, want_ry = D.crafted()
    rows, c3, ci, counts = D.decode(lab, None, ori, c6, rp, inv, P2, D.KITTI_MEAN, False, False, 16)
    assert counts.tolist() == [len(names)]
    r = dict(zip(names, rows[0]))
    assert r["bin11_wraps"][1] == (11 * (2 * np.pi / 12) + 0.2) - 2 * np.pi and r["bin5_below"][1] == 5 * (2 * np.pi / 12) + 0.25
    for name, ry in want_ry.items():
        assert r[name][12] == ry, (name, r[name][12], ry)
    assert set(want_ry) == {"ry_pi", "ry_below_pi", "ry_above_pi", "ry_minus_pi", "ry_above_minus_pi", "ry_below_minus_pi"}
    assert r["behind_camera"][11] == -7.5 and r["on_camera_plane"][11] == 0.0


# ---------------------------------------------------------------------------------------------------------------- refusals
def _host_batch(n=2):
    lab, ori, c6, P2, rp, inv = D.synth((n, 1), 5)
    b = {k: torch.from_numpy(v) for k, v in lab.items()}
    b.update(ori_shape=[np.array(o) for o in ori], ratio_pad=torch.from_numpy(rp), info=[{"trans_inv": t} for t in inv], im_file=["a.txt", "b.txt"],
             img=torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
    return b, [tuple(c) for c in c6], P2


def test_wrappers_refuse_host_tensors_and_broken_batches():
    b, c6, P2 = _host_batch()
    for fn in (kitti.decode_batch_device, kitti.decode_batch, lambda *a: json3d.decode_batch_device(*a, dataset="waymo"),
               lambda *a: json3d.decode_batch(*a, dataset="omni3d")):
        with pytest.raises(y3d.Y3DError, match="HIP device"):
            fn(b, c6)
    for k in ("cls", "depth", "heading_res", "batch_idx"):
        with pytest.raises(y3d.Y3DError, match="per-box keys"):
            kitti.decode_batch_device({q: v for q, v in b.items() if q != k}, c6)
    for k in ("ori_shape", "ratio_pad", "info"):
        with pytest.raises(y3d.Y3DError, match="lacks"):
            kitti.decode_batch_device({q: v for q, v in b.items() if q != k}, c6)
    with pytest.raises(y3d.Y3DError, match="one of"):
        json3d.decode_batch_device(b, c6, dataset="nuscenes")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        plot.label_pictures(b, c6, P2)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        plot.draw_labels3d(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 1, 14, dtype=torch.float64), torch.zeros(1, 1, 8, 3, dtype=torch.float64),
                           torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4, dtype=torch.float64))
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        plot.box2d_segments(torch.zeros(1, 1, 14, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
    # decode_labels, the capturable core: host tensors, missing keys
    lab = {k: b[k] for k in D.KEYS}
    ori, calib, rp = torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 6, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float64)
    ms = torch.ones(3, 3, dtype=torch.float64)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        kitti.decode_labels(lab, None, ori, calib, rp, None, None, ms, undo_augment=False)
    with pytest.raises(y3d.Y3DError, match="per-box keys"):
        kitti.decode_labels({k: v for k, v in lab.items() if k != "size_3d"}, None, ori, calib, rp, None, None, ms, undo_augment=False)
    with pytest.raises(y3d.Y3DError, match=r"\(B, 2\)"):
        kitti.decode_labels(lab, None, torch.zeros(2, 3, dtype=torch.float64), calib, rp, None, None, ms, undo_augment=False)


# the C entry checks everything before it launches: addresses are compared and tested for alignment, never read, so made-up ones do
_A = dict(cls=0x10000, bboxes=0x20000, center_3d=0x30000, size_3d=0x40000, depth=0x50000, heading_bin=0x60000, heading_res=0x70000,
          batch_idx=0x80000, counts_in=None, N=4, max_objs=0, B=2, ori_shape=0x90000, calib=0xA0000, ratio=0xB0000, ratio_pitch=4,
          trans_inv=0xC0000, P2=0xD0000, mean_size=0xE0000, nc=3, use_camera_dis=0, undo_augment=1, R=4, rows=0x100000, corners3d=0x110000,
          corners_img=0x120000, counts=0x130000, stream=None)


def _entry(**over):
    a = dict(_A, **over)
    return y3d.lib().decode_labels(*[a[k] for k in _A])


@pytest.mark.parametrize("over,match", [
    (dict(rows=None), "null output"), (dict(corners3d=None), "null output"), (dict(counts=None), "null output"),
    (dict(corners_img=None), "goes with P2"), (dict(P2=None), "goes with P2"),
    (dict(rows=0x100008), "aligned"), (dict(corners3d=0x110008), "aligned"), (dict(corners_img=0x120004), "aligned"), (dict(counts=0x130002), "aligned"),
    (dict(R=0), "R = 0"), (dict(R=-3), "R = -3"), (dict(B=0), "bad sizes"), (dict(nc=0), "bad sizes"), (dict(N=-1), "bad sizes"),
    (dict(ratio_pitch=3), "ratio_pitch"), (dict(trans_inv=None), "needs trans_inv"), (dict(bboxes=None), "null per-box"),
    (dict(batch_idx=None), "needs batch_idx"), (dict(counts_in=0xF0000, max_objs=3), "static layout"), (dict(calib=None), "null per-image"),
    (dict(rows=0x20000 + 16), "overlaps an input"),            # inside bboxes
    (dict(counts=0xA0000 + 8), "overlaps an input"),           # inside calib
    (dict(corners3d=0x100000 + 14 * 8 * 4), "overlap each other"),  # inside rows (2 x 4 x 14 doubles)
    (dict(rows=0x110000 - 2 * 4 * 14 * 8 + 16), "overlap each other"),  # rows ends 16 bytes inside corners3d
])
def test_entry_refuses_before_anything_is_launched(over, match):
    with pytest.raises(y3d.Y3DError, match=match):
        _entry(**over)


def test_validator_takes_pictures_and_defaults_to_none():
    assert inspect.signature(val.Validator3d).parameters["pictures"].default == 0
    assert inspect.signature(kitti.decode_batch_device).parameters["undo_augment"].default is True
    m3 = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml"))
    for bad in (-1, 1.5):
        with pytest.raises(y3d.Y3DError, match="pictures"):
            val.Validator3d(m3, "/nowhere", pictures=bad)
    # pictures=0 is accepted as an argument: on a host the constructor then stops at the device check, as it does without it
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        val.Validator3d(m3, "/nowhere", pictures=0)
    if torch.cuda.is_available():
        v = val.Validator3d(m3.to("cuda"), "/nowhere", pictures=0)
        assert v.n_pictures == 0 and v.pictures == []
