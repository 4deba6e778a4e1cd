"""CPU: the KITTI evaluator's host side — ABI declarations, KITTI text parsing, the in-memory rounding of get_stats, the recall
threshold scan, and the refusals (no GPU needed)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib


def fixture_annos():
    z = np.load(os.path.join(GOLDEN, "kitti_eval.npz"))
    out = []
    for side in ("gt_", "dt_"):
        n = z[side + "n"]
        off = np.concatenate(([0], np.cumsum(n)))
        keys = [k[len(side):] for k in z.files if k.startswith(side) and k != side + "n"]
        out.append([{k: z[side + k][off[i]:off[i + 1]] for k in keys} for i in range(len(n))])
    return out


def test_prototypes_declared_and_module_imports():
    protos = _lib.parse_header()
    for name in ("y3d_kitti_eval_max_boxes", "y3d_kitti_box_overlaps", "y3d_kitti_eval_thresholds", "y3d_kitti_eval_counts"):
        assert name in protos, name
    from yolov10_3d_amd import kitti_eval
    assert kitti_eval.eval_from_scrach is kitti_eval.eval_from_scratch
    assert y3d.lib().kitti_eval_max_boxes() >= 256


def _line(a, i, det):
    f = lambda v: f"{float(v):.2f}"
    h, w, l = a["dimensions"][i][1], a["dimensions"][i][2], a["dimensions"][i][0]
    vals = [a["alpha"][i], *a["bbox"][i], h, w, l, *a["location"][i], a["rotation_y"][i]] + ([a["score"][i]] if det else [])
    return " ".join([str(a["name"][i]), f(a["truncated"][i]), str(int(a["occluded"][i]))] + [f(v) for v in vals])


def test_text_files_parse_to_the_fixture_annos_bitwise(tmp_path):
    from yolov10_3d_amd import kitti_eval as KE
    gts, dts = fixture_annos()
    for side, annos, det in (("gt", gts, False), ("dt", dts, True)):
        for i, a in enumerate(annos[:40]):
            p = tmp_path / f"{side}{i:06d}.txt"
            p.write_text("".join(_line(a, j, det) + "\n" for j in range(len(a["name"]))))
            b = KE.read_label_file(str(p), det=det)
            assert set(b) == set(a)
            for k in a:
                assert b[k].shape == a[k].shape, (i, k)
                if k == "name":
                    assert b[k].tolist() == a[k].tolist(), i
                else:
                    assert b[k].dtype == a[k].dtype == np.float32 and np.array_equal(b[k].view(np.int32), a[k].view(np.int32)), (i, k)


def test_get_stats_rounding_equals_a_file_round_trip(tmp_path):
    """save_results (kitti.py:452-464) writes '{:.2f}' text that eval_from_scrach reads back as float32; the in-memory path rounds alike"""
    from yolov10_3d_amd import kitti_eval as KE
    rng = np.random.default_rng(3)
    names = ("Car", "Pedestrian", "Cyclist")
    results = {}
    for i in range(6):
        n = int(rng.integers(0, 7))
        r = rng.normal(0, 30, (n, 14))
        r[:, 0] = rng.integers(0, 3, n)
        r[:, 1:5] = np.round(r[:, 1:5], 3) + 0.005   # halfway cases of the 2-decimal rounding (as binary fractions)
        r[:, 13] = rng.random(n)
        results[f"{i:06d}.txt"] = r.tolist()
    files, annos = KE.results_to_annos(results, names)
    assert files == sorted(results)
    for f, a in zip(files, annos):
        with open(tmp_path / f, "w") as fh:   # save_results' format
            for row in results[f]:
                fh.write("{} 0.0 0".format(names[int(row[0])]))
                for v in row[1:]:
                    fh.write(" {:.2f}".format(v))
                fh.write("\n")
        b = KE.read_label_file(str(tmp_path / f), det=True)
        for k in b:
            assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, (f, k)


def _thresholds_literal(scores, num_gt, num_sample_pts=41):
    """get_thresholds (kitti_eval.py:347-366) restated as the plain sequential scan"""
    scores = np.sort(np.asarray(scores, np.float64))[::-1]
    cur, out = 0, []
    for i, s in enumerate(scores):
        lr = (i + 1) / num_gt
        rr = (i + 2) / num_gt if i < len(scores) - 1 else lr
        if (rr - cur) < (cur - lr) and i < len(scores) - 1:
            continue
        out.append(s)
        cur += 1 / (num_sample_pts - 1.0)
    return out


def test_threshold_scan_matches_the_sequential_scan():
    from yolov10_3d_amd import kitti_eval as KE
    rng = np.random.default_rng(7)
    for n, ng in ((0, 5), (1, 1), (3, 3), (40, 40), (41, 80), (150, 200), (777, 900), (2000, 2100), (57, 57)):
        s = np.round(rng.random(n), 2).astype(np.float32).astype(np.float64)
        want = _thresholds_literal(s, ng)
        got = KE.get_thresholds(np.sort(s)[::-1], ng)
        assert got == want, (n, ng)


def test_refusals():
    from yolov10_3d_amd import kitti_eval as KE
    gts, dts = fixture_annos()
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        KE.box_overlaps(gts[:3], dts[:3], 1, device="cpu")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        KE.eval_class(gts[:3], dts[:3], [0], [0, 1, 2], 0, np.full((1, 3, 1), 0.7), device="cpu")
    cap = y3d.lib().kitti_eval_max_boxes()
    big = {k: np.repeat(v[:1], cap + 1, axis=0) for k, v in next(a for a in dts if len(a["name"])).items()}
    with pytest.raises(y3d.Y3DError, match="at most"):
        KE.box_overlaps(gts[:1], [big], 0)
    with pytest.raises(y3d.Y3DError, match="z_center"):
        KE.get_official_eval_result(gts, dts, "Car", z_center=0.5)
    with pytest.raises(y3d.Y3DError, match="z_axis"):
        KE.get_official_eval_result(gts, dts, "Car", z_axis=2)
