"""GPU: the KITTI AP evaluator (csrc/kitti_eval.hip) against the reference's own tables (tests/golden/kitti_eval.npz, minted by
tools/make_golden_kitti_eval.py) and against an independent fp64 polygon-clipping restatement of the rotated overlaps."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from kitti_eval_ref import bev_iou, iou3d   # the independent fp64 polygon clipping, shared with test_hip_kitti_eval_edges.py
from test_kitti_eval_host import _line, fixture_annos

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import kitti_eval as KE  # noqa: E402


def golden():
    return np.load(os.path.join(GOLDEN, "kitti_eval.npz"))


def assert_detail(got, z, prefix):
    keys = [k[len(prefix):] for k in z.files if k.startswith(prefix)]
    assert keys and set(keys) == set(got), (prefix, set(keys) ^ set(got))
    for k in keys:
        want = z[prefix + k]
        g = np.asarray(got[k], np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(want)), (prefix, k, g, want)
        assert np.allclose(g, want, rtol=0, atol=1e-9, equal_nan=True), (prefix, k, g, want)


def test_overlaps_match_the_reference():
    gts, dts = fixture_annos()
    z = golden()
    for metric in range(3):
        got = torch.cat([o.reshape(-1) for o in KE.box_overlaps(gts, dts, metric)]).cpu().numpy()
        want = z[f"ov{metric}"]
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, err_msg=f"metric {metric}")


@pytest.mark.parametrize("mode", [40, 11])
def test_detail_tables_match_the_reference(mode):
    gts, dts = fixture_annos()
    z = golden()
    for cls in ("Car", "Pedestrian", "Cyclist"):
        got = KE.get_official_eval_result(gts, dts, cls, ap_mode=mode)["detail"][cls]
        assert_detail(got, z, f"detail{mode}|{cls}|")


def test_fewer_than_50_images():
    """7 images: the reference's 50-part split fails on them; its table for them padded by 43 empty images is the answer"""
    gts, dts = fixture_annos()
    got = KE.get_official_eval_result(gts[:7], dts[:7], "Car")["detail"]["Car"]
    assert_detail(got, golden(), "subset40|Car|")


def test_repeated_runs_are_bit_identical():
    gts, dts = fixture_annos()
    mo = np.stack([np.full((3, 3), 0.7), np.full((3, 3), 0.5)])
    for metric in range(3):
        a = KE.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], metric, mo, compute_aos=True)
        b = KE.eval_class(gts, dts, [0, 1, 2], [0, 1, 2], metric, mo, compute_aos=True)
        for k in ("precision", "orientation", "thresholds"):
            assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), (metric, k)
        assert not a["recall"].any()


def annos_of(boxes, score=False):
    b = np.asarray(boxes, np.float32).reshape(-1, 7)
    n = b.shape[0]
    a = {"name": np.array(["Car"] * n), "bbox": np.tile(np.float32([0, 0, 10, 50]), (n, 1)), "alpha": np.zeros(n, np.float32),
         "occluded": np.zeros(n, np.float32), "truncated": np.zeros(n, np.float32), "location": b[:, 0:3], "dimensions": b[:, 3:6],
         "rotation_y": b[:, 6]}
    if score:
        a["score"] = np.full(n, 0.5, np.float32)
    return a


def device_pairs(gt_boxes, dt_boxes, metric):
    """one image per (gt, dt) pair -> the device overlaps, fp64"""
    gts = [annos_of([g]) for g in gt_boxes]
    dts = [annos_of([d], True) for d in dt_boxes]
    return np.array([float(o.reshape(-1)[0]) for o in KE.box_overlaps(gts, dts, metric)])


def test_rotated_overlaps_against_fp64_clipping():
    car = (1.0, 1.6, 20.0, 3.9, 1.5, 1.6, 0.3)
    sq = (-2.0, 1.5, 12.0, 2.0, 1.5, 2.0, 0.4)
    far = (30.0, 1.6, 60.0, 3.9, 1.5, 1.6, -1.1)
    sq90 = sq[:6] + (sq[6] + math.pi / 2,)
    got_bev = device_pairs([car, sq, car], [car, sq90, far], 1)
    got_3d = device_pairs([car, sq, car], [car, sq90, far], 2)
    np.testing.assert_allclose(got_bev, [1.0, 1.0, 0.0], atol=1e-5)   # identical / 90-degree square twin / disjoint
    np.testing.assert_allclose(got_3d, [1.0, 1.0, 0.0], atol=1e-5)
    # fp32 corners carry ~ulp(|coordinate|) of rounding, which the IoU of a small box divides by its area: pairs within 14 m agree with
    # fp64 within 1e-5; across the KITTI range (40 m) the reference's own fp32 geometry is 2.7e-5 from fp64 on these pairs, and so is this
    for (zr, xr), tol in (((2, 14), 6), 1e-5), (((5, 40), 10), 5e-5):
        rng = np.random.default_rng(11)
        gt, dt = [], []
        for _ in range(300):
            g = (rng.uniform(-xr, xr), rng.uniform(1, 2), rng.uniform(*zr), rng.uniform(0.5, 5), rng.uniform(1, 2), rng.uniform(0.5, 2.5),
                 rng.uniform(-math.pi, math.pi))
            d = tuple(np.asarray(g) + rng.normal(0, [0.6, 0.2, 0.8, 0.3, 0.2, 0.2, 0.5]))
            d = d[:3] + tuple(abs(v) + 0.1 for v in d[3:6]) + d[6:]
            gt.append(tuple(float(np.float32(v)) for v in g))
            dt.append(tuple(float(np.float32(v)) for v in d))
        want_bev = [bev_iou((g[0], g[2], g[3], g[5], g[6]), (d[0], d[2], d[3], d[5], d[6])) for g, d in zip(gt, dt)]
        want_3d = [iou3d(g, d) for g, d in zip(gt, dt)]
        np.testing.assert_allclose(device_pairs(gt, dt, 1), want_bev, rtol=0, atol=tol)
        np.testing.assert_allclose(device_pairs(gt, dt, 2), want_3d, rtol=0, atol=tol)
        assert 0.2 < np.mean(np.asarray(want_bev) > 0) < 1.0   # the random pairs overlap partly, and some not at all


def test_get_stats_equals_eval_from_scratch_on_saved_files(tmp_path):
    """validator path: decode_preds_eval rows -> get_stats in memory == eval_from_scratch on the files save_results would write"""
    from conftest import load_golden
    from yolov10_3d_amd import kitti
    g = load_golden("kitti_decode")
    preds = g["preds"].to("cuda")
    files = [f"{i:06d}.txt" for i in range(preds.shape[0])]
    results = kitti.decode_preds_eval(preds, g["calib"], files, g["ratio"], g["inv_trans"])
    names = ("Car", "Pedestrian", "Cyclist")
    label_dir, pred_dir = tmp_path / "label_2", tmp_path / "preds"
    label_dir.mkdir()
    pred_dir.mkdir()
    rng = np.random.default_rng(5)
    for f in files:
        with open(pred_dir / f, "w") as fh:   # save_results (kitti.py:452-464)
            for row in results[f]:
                fh.write("{} 0.0 0".format(names[int(row[0])]))
                for v in row[1:]:
                    fh.write(" {:.2f}".format(v))
                fh.write("\n")
        # labels: the detections moved a little, so that every metric sees matches and misses
        det = KE.read_label_file(str(pred_dir / f), det=True)
        n = len(det["name"])
        det["bbox"] = det["bbox"] + rng.normal(0, 2, (n, 4)).astype(np.float32)
        det["location"] = det["location"] + rng.normal(0, 0.1, (n, 3)).astype(np.float32)
        det["truncated"] = np.zeros(n, np.float32)
        (label_dir / f).write_text("".join(_line(det, j, False) + "\n" for j in range(n)))
    want = KE.eval_from_scratch(str(label_dir), str(pred_dir))["3d@0.70"][1]
    got = KE.get_stats(results, str(label_dir))
    assert got == want
    got_all = KE.eval_from_scratch(str(label_dir), str(pred_dir), ["Car"])
    assert all(np.isfinite(v).all() for v in got_all.values())
