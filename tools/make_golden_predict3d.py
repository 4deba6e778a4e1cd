"""Mints tests/golden/predict3d.npz from the REFERENCE's KITTI decode, box corners, projection, result writer and unaugmented-sample
arithmetic, run on the CPU.

    python tools/make_golden_predict3d.py      # needs the reference checkout (oracle.ref_shim.import_reference)

Inputs are those of oracle/make_golden_kitti.py's recipe: tests/golden/kitti_decode.npz's `preds` (3, 12, 37), `ratio` and `inv_trans`
are reused, and the recipe's three float32 P2 matrices (P2[2, 3] = 0.004981016, so the projection's denominator is not the plain depth)
are rebuilt and recorded; the tool asserts that their six calibration constants are the ones that fixture holds.

Recorded from the reference:
  * `KITTIDataset.decode_preds` (with the inverse affine, pinhole depth) at thresholds 0.001 and 0.25: rows padded to (B, K, 14), counts;
  * the predictor's filter for the class lists None, [0], [1, 2], [2]: `YOLOv10_3DDetectionPredictor.postprocess`
    (models/yolov10_3D/predict.py:8-38) is called unbound on a namespace carrying args.conf / args.classes / args.max_det, batch and
    model.names, with six-wide rows built from a confidence and the label column and blank original images of the canvas's size
    (scale_boxes is then the identity); recorded is which rows survive, over every row of the decode fixture and over the 0.25 set;
  * `Object3d.generate_corners3d` and `Calibration.corners3d_to_img_boxes` (its `boxes_corner`) on every kept row, called unbound on a
    namespace carrying h, w, l, ry, pos / P2;
  * the text `KITTIDataset.save_results` writes for the 0.25 set;
  * for the sizes (1242, 375), (1224, 370), (97, 61), (310, 94) at resolutions (1280, 384) and (320, 256): `get_affine_transform`'s
    `trans` / `trans_inv` as kitti.py:187 calls it, and `resolution / img_size`.

OpenCV is absent: `cv2.getAffineTransform` is supplied as the exact float64 three-point solve (tools/make_golden_kitti_labels.py).  The
tool asserts what the tests rely on: at 0.25 every image keeps and drops a row; the class list [0] empties image 0; every kept corner
lies at least 1 m in front of the camera.  The fixture holds data only: recorded numbers and text.
"""
from __future__ import annotations

import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "predict3d.npz")
THRESHOLDS = {"t001": 0.001, "t25": 0.25}
CLASS_LISTS = {"none": None, "c0": [0], "c12": [1, 2], "c2": [2]}
SIZES = [(1242, 375), (1224, 370), (97, 61), (310, 94)]  # (W, H)
RESOLUTIONS = [(1280, 384), (320, 256)]
CLS_MEAN_SIZE = [[1.52563191462, 1.62856739989, 3.88311640418], [1.76255119, 0.66068622, 0.84422524], [1.73698127, 0.59706367, 1.76282397]]


def affine_from_points(src, dst):
    """cv2.getAffineTransform: the exact 2x3 map through three point pairs, in float64"""
    A = np.hstack((np.asarray(src, np.float64), np.ones((3, 1))))
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T.copy()


def recipe_p2(B):
    """the float32 P2 matrices of oracle/make_golden_kitti.py"""
    out = []
    for i in range(B):
        f = 707.0493 + 10 * i
        out.append(np.array([[f, 0, 604.0814 + 3 * i, 45.75831 - i], [0, f, 180.5066 - 2 * i, -0.3454157 + 0.1 * i], [0, 0, 1, 0.004981016]],
                            dtype=np.float32))
    return out


def survivors(Predictor, labels, conf, threshold, classes, batch):
    """`YOLOv10_3DDetectionPredictor.postprocess` unbound on six-wide rows [box, conf, label] built from `conf` and `labels` (B, K) -> (B, K) array
    holding, at each surviving row's position, the confidence it came back with (0 elsewhere)"""
    import torch
    B, K = labels.shape
    pos = torch.arange(K, dtype=torch.float32).repeat(B, 1)
    # x1 = x2 = the row's position, y = 2 .. 4: inside the 8 x K image below, which scale_boxes leaves unscaled and unclipped
    rows = torch.stack([pos, torch.full((B, K), 2.0), pos, torch.full((B, K), 4.0), conf.float(), labels.float()], -1)
    ns = types.SimpleNamespace(args=types.SimpleNamespace(conf=threshold, classes=classes, max_det=K), batch=batch,
                               model=types.SimpleNamespace(names={0: "Car", 1: "Pedestrian", 2: "Cyclist"}))
    res = Predictor.postprocess(ns, rows, torch.zeros(B, 3, 8, K), [np.zeros((8, K, 3), np.uint8)] * B)
    out = np.zeros((B, K))
    for b, r in enumerate(res):
        d = r.boxes.data.numpy()
        pos = d[:, 0].astype(np.int64)
        assert np.array_equal(pos, np.sort(pos)) and np.array_equal(d[:, 5], labels[b].numpy()[pos]) and (d[:, 4] > threshold).all()
        out[b, pos] = d[:, 4]
    return out


def main():
    import torch
    R.import_reference()
    from ultralytics.data.datasets import kitti_utils as KU
    from ultralytics.data.datasets.kitti import KITTIDataset
    from ultralytics.data.datasets.kitti_utils import Calibration, Object3d
    from ultralytics.models.yolov10_3D.predict import YOLOv10_3DDetectionPredictor as Predictor
    sys.modules["cv2"].getAffineTransform = affine_from_points
    KU.cv2 = sys.modules["cv2"]

    g = np.load(os.path.join(ROOT, "tests", "golden", "kitti_decode.npz"))
    preds = torch.from_numpy(g["preds"])
    B, K = preds.shape[:2]
    P2s = recipe_p2(B)
    calibs = [Calibration({"P2": P, "R0": np.eye(3, dtype=np.float32), "Tr_velo2cam": np.eye(3, 4, dtype=np.float32)}) for P in P2s]
    calib6 = np.array([[float(c.cu), float(c.cv), float(c.fu), float(c.fv), float(c.tx), float(c.ty)] for c in calibs], np.float64)
    assert np.array_equal(calib6, g["calib"]), "the recipe's P2 no longer give kitti_decode.npz's calibration constants"
    ratio_pad = torch.from_numpy(np.stack([g["ratio"], np.zeros_like(g["ratio"])], 1))
    inv_trans = [np.asarray(t, np.float64) for t in g["inv_trans"]]
    files = [f"{i:06d}.txt" for i in range(B)]
    ds = types.SimpleNamespace(cls_mean_size=np.array(CLS_MEAN_SIZE), use_camera_dis=False, class_name=["Car", "Pedestrian", "Cyclist"])
    out = {"P2": np.stack(P2s), "thresholds": np.array(list(THRESHOLDS.values())), "threshold_tags": np.array(list(THRESHOLDS)),
           "class_tags": np.array(list(CLASS_LISTS)), "files": np.array(files)}

    min_depth = np.inf
    results = {}
    for tag, thr in THRESHOLDS.items():
        res = KITTIDataset.decode_preds(ds, preds.clone(), calibs, files, ratio_pad, inv_trans, undo_augment=True, threshold=thr)
        results[tag] = res
        rows, counts = np.zeros((B, K, 14)), np.zeros(B, np.int64)
        c3, ci = np.zeros((B, K, 8, 3)), np.zeros((B, K, 8, 2))
        for i, f in enumerate(files):
            counts[i] = len(res[f])
            for j, r in enumerate(res[f]):
                rows[i, j] = [float(np.asarray(v).reshape(-1)[0]) for v in r]
                _, _, _, _, _, _, h, w, l, x, y, z, ry, _ = rows[i, j]
                obj = types.SimpleNamespace(h=h, w=w, l=l, ry=ry, pos=np.array([x, y, z]))
                c3[i, j] = Object3d.generate_corners3d(obj)
                ci[i, j] = Calibration.corners3d_to_img_boxes(types.SimpleNamespace(P2=P2s[i]), c3[i, j][None])[1][0]
                min_depth = min(min_depth, float(c3[i, j, :, 2].min()))
        out[f"{tag}/rows"], out[f"{tag}/counts"], out[f"{tag}/corners3d"], out[f"{tag}/corners_img"] = rows, counts, c3, ci

    # the predictor's filter (models/yolov10_3D/predict.py:23-25), executed: postprocess takes six-wide rows as they are
    files_b = [[f"{i}.png" for i in range(B)]]
    for tag, classes in CLASS_LISTS.items():
        if classes is not None:
            out[f"classes/{tag}"] = np.array(classes, np.int64)
        # every row of the decode fixture: only the class list decides (the confidence column carries the row's index + 1)
        mask = survivors(Predictor, preds[..., 36], torch.arange(1, K + 1, dtype=torch.float32).repeat(B, 1), 0.0, classes, files_b) > 0
        out[f"class_mask/{tag}"] = mask
        # the 0.25 set: its rows' own classes and scores, padding rows at confidence -1
        lab, conf = torch.zeros(B, K), -torch.ones(B, K)
        for i, f in enumerate(files):
            n = len(results["t25"][f])
            lab[i, :n] = torch.tensor([float(r[0]) for r in results["t25"][f]])
            conf[i, :n] = torch.tensor([float(np.asarray(r[13]).reshape(-1)[0]) for r in results["t25"][f]])
        kept = survivors(Predictor, lab, conf, 0.0, classes, files_b) > 0
        assert not any(kept[i, len(results["t25"][f]):].any() for i, f in enumerate(files))
        out[f"class_keep_t25/{tag}"] = kept
        out[f"class_counts_t25/{tag}"] = kept.sum(1).astype(np.int64)
    assert out["class_mask/none"].all() and out["class_counts_t25/none"].tolist() == [len(results["t25"][f]) for f in files]

    tmp = tempfile.mkdtemp(prefix="y3d_p3d_")
    try:
        KITTIDataset.save_results(ds, results["t25"], output_dir=tmp)
        assert sorted(os.listdir(os.path.join(tmp, "preds"))) == files
        out["save_text"] = np.array([open(os.path.join(tmp, "preds", f)).read() for f in files])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    for W, H in RESOLUTIONS:
        tr, ti, rt = [], [], []
        for size in SIZES:
            img_size = np.array(size)  # kitti.py:121, :130-131, :187, :404
            trans, trans_inv = KU.get_affine_transform(np.array(img_size) / 2, img_size, 0, np.array([W, H]), inv=1)
            tr.append(trans)
            ti.append(trans_inv)
            rt.append(np.array([W, H]) / img_size)
        out[f"plan_{W}x{H}/trans"], out[f"plan_{W}x{H}/trans_inv"], out[f"plan_{W}x{H}/ratio"] = np.stack(tr), np.stack(ti), np.stack(rt)
    out["plan_sizes"] = np.array(SIZES, np.int64)
    out["plan_resolutions"] = np.array(RESOLUTIONS, np.int64)

    # what the tests rely on
    c25, c001 = out["t25/counts"], out["t001/counts"]
    assert (c25 >= 1).all() and (c25 < K).all(), c25
    assert (c001 >= c25).all() and (c001 < K).all(), c001
    assert out["class_counts_t25/c0"][0] == 0 and out["class_counts_t25/c0"].sum() > 0, out["class_counts_t25/c0"]
    assert min_depth >= 1.0, min_depth
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100 * 1024, size
    print(f"wrote {OUT} ({size} bytes): kept at 0.25 {c25.tolist()} of {K}, at 0.001 {c001.tolist()}, class [0] at 0.25 "
          f"{out['class_counts_t25/c0'].tolist()}, nearest kept corner {min_depth:.2f} m")


if __name__ == "__main__":
    main()
