"""Mints tests/golden/decode_batch.npz from the REFERENCE's `decode_batch` (data/datasets/kitti.py:469-513 and its copies in waymo.py and
omni3d.py), run on the CPU.

    python tools/make_golden_decode_batch.py      # needs the reference checkout (oracle.ref_shim.import_reference)

The batches are those of the label fixtures: the synthetic trees of tests/kitti_labels_tree.py and tests/json3d_tree.py are rebuilt from
tests/golden/{kitti,waymo,omni3d}_labels.npz, and for each dataset the recorded runs `val` (a validation batch) and `default` (a seeded
train batch with flips, crops and mixup), for KITTI also `camdis` (cam_dis=True, which sets use_camera_dis on the dataset object) and for
Omni3D also `nomix` (see RUNS), are minted again from the reference's own `__getitem__` + `collate_fn`.  The tool asserts that every
per-box tensor equals the one the label fixture holds, so the tests take the INPUTS from those fixtures and only the decoded boxes are
stored here:

  <dataset>/calib6 (frames, 6), <dataset>/P2 (frames, 3, 4)   the original calibrations, by dataset position (`get_calib`)
  <dataset>/<run>/counts (B,)                                  boxes per image
  <dataset>/<run>/rows (n, 14)                                 decode_batch(undo_augment=True), images back to back
  <dataset>/<run>/loc0 (n, 3)                                  the location columns of decode_batch(undo_augment=False); every other
                                                               column equals undo_augment=True's (asserted)
  <dataset>/val/corner_rows (m,), corners3d (m, 8, 3),         `Object3d.generate_corners3d` and `Calibration.corners3d_to_img_boxes`
  corners_img (m, 8, 2)                                        (its boxes_corner) of every fourth val row, called unbound as
                                                               tools/make_golden_predict3d.py does

Asserted on the reference's output alone: an image without boxes and the frame with the most label lines are present, every class is
present, class2angle wraps (an angle above pi) and alpha2ry wraps at both ends at least once, and no wrap decision lies closer than
1e-6 rad to its edge.  OpenCV is absent: `cv2.getAffineTransform` is supplied as the exact float64 three-point solve.  The fixture
holds numbers only."""
from __future__ import annotations

import os
import shutil
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "decode_batch.npz")
# Omni3D's yaw lies in [-pi/2, pi/2], so only its mirrored frames can wrap alpha2ry: `val` and `default` never do, `nomix` (a seeded train
# batch with flips and crops) wraps at both ends and is recorded for that
RUNS = {"kitti": ("val", "default", "camdis"), "waymo": ("val", "default"), "omni3d": ("val", "default", "nomix")}
CORNER_STEP = 4  # corners are recorded for every fourth val row (320 bytes each)
KEYS = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx")
MARGIN = 1e-6


def affine_from_points(src, dst):
    """cv2.getAffineTransform: the exact 2x3 map through three point pairs, in float64"""
    A = np.hstack((np.asarray(src, np.float64), np.ones((3, 1))))
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T.copy()


def scalar(v):
    return float(np.asarray(v).reshape(-1)[0])


def mint_batch(ds, collate, seed, items):
    """the run as the label tools draw it: one seed, then the items in order"""
    np.random.seed(seed)
    outs = [ds[i] for i in items]
    for o in outs:
        o.pop("ori_img", None)
    return collate(outs)


def decode(ds, KU, batch, z, run, out, tag, stats):
    """both decodes of one batch, recorded under `tag`; the wrap statistics of its boxes go to `stats`"""
    calibs = [ds.get_calib(i["img_id"]) for i in batch["info"]]
    for k in KEYS:  # the inputs are the label fixture's
        a, b = batch[k].numpy(), z[f"{run}/c/{k}"]
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{tag}: {k} differs from the label fixture"
    assert np.array_equal(np.stack([np.asarray(i["trans_inv"], np.float64) for i in batch["info"]]), z[f"{run}/trans_inv"]), tag
    # decode_batch keys its result by im_file, and a train run draws some frames twice: number the names so that no image is lost
    batch["im_file"] = files = [f"{n:02d}_{f}" for n, f in enumerate(batch["im_file"])]
    res = {u: type(ds).decode_batch(ds, batch, calibs, undo_augment=bool(u)) for u in (1, 0)}
    assert list(res[1]) == files and list(res[0]) == files
    rows = {u: np.array([[scalar(v) for v in r] for f in files for r in res[u][f]], np.float64).reshape(-1, 14) for u in (1, 0)}
    counts = np.array([len(res[1][f]) for f in files], np.int64)
    other = [c for c in range(14) if c not in (9, 10, 11)]
    assert np.array_equal(rows[1][:, other], rows[0][:, other]) and counts.tolist() == [len(res[0][f]) for f in files]
    assert (rows[1][:, 13] == 1).all()
    out[f"{tag}/counts"], out[f"{tag}/rows"], out[f"{tag}/loc0"] = counts, rows[1], rows[0][:, 9:12]
    if run == "val":
        pick = np.arange(0, len(rows[1]), CORNER_STEP)
        c3, ci = np.zeros((len(pick), 8, 3)), np.zeros((len(pick), 8, 2))
        img = np.repeat(np.arange(len(files)), counts)[pick]
        for j, r in enumerate(rows[1][pick]):
            obj = types.SimpleNamespace(h=r[6], w=r[7], l=r[8], ry=r[12], pos=np.array(r[9:12]))
            c3[j] = KU.Object3d.generate_corners3d(obj)
            ci[j] = KU.Calibration.corners3d_to_img_boxes(types.SimpleNamespace(P2=calibs[img[j]].P2), c3[j][None])[1][0]
        out[f"{tag}/corner_rows"], out[f"{tag}/corners3d"], out[f"{tag}/corners_img"] = pick, c3, ci
        stats["min_depth"] = min(stats["min_depth"], float(c3[..., 2].min()) if len(c3) else np.inf)
    # wrap statistics, from the batch's own numbers in float64
    img = batch["batch_idx"].numpy().astype(np.int64)
    ang = batch["heading_bin"].numpy().astype(np.float64) * (2 * np.pi / 12) + batch["heading_res"].numpy().astype(np.float64)
    alpha = np.where(ang > np.pi, ang - 2 * np.pi, ang)
    W = np.array([float(batch["ori_shape"][i][1]) for i in img])
    cu = np.array([float(calibs[i].cu) for i in img])
    fu = np.array([float(calibs[i].fu) for i in img])
    ry = alpha + np.arctan2(batch["bboxes"].numpy().astype(np.float64).reshape(-1, 4)[:, 0] * W - cu, fu)
    stats["angle_wraps"] += int((ang > np.pi).sum())
    stats["ry_high"] += int((ry > np.pi).sum())
    stats["ry_low"] += int((ry < -np.pi).sum())
    stats["margin"] = min([stats["margin"]] + np.abs(ang - np.pi).tolist() + np.abs(ry - np.pi).tolist() + np.abs(ry + np.pi).tolist())
    stats["classes"] |= set(rows[1][:, 0].astype(int).tolist())
    stats["empty"] += int((counts == 0).sum())
    np.testing.assert_allclose(rows[1][:, 1], alpha, rtol=0, atol=1e-12)
    return counts


def main():
    R.import_reference()
    from ultralytics.data.datasets import kitti as K
    from ultralytics.data.datasets import kitti_utils as KU
    from ultralytics.data.datasets import omni3d as O
    from ultralytics.data.datasets import waymo as Wm
    import json3d_tree
    import kitti_labels_tree
    cv2 = sys.modules["cv2"]
    cv2.getAffineTransform = affine_from_points
    K.cv2 = KU.cv2 = cv2

    out = {}
    summary = []
    for dataset in ("kitti", "waymo", "omni3d"):
        z = kitti_labels_tree.fixture() if dataset == "kitti" else json3d_tree.fixture(dataset)
        root = tempfile.mkdtemp(prefix=f"y3d_decode_batch_{dataset}_")
        stats = dict(angle_wraps=0, ry_high=0, ry_low=0, margin=np.inf, classes=set(), empty=0, min_depth=np.inf)
        try:
            if dataset == "kitti":
                kitti_labels_tree.write_tree(root, z, images=True)
                lines = [len(str(t).splitlines()) for t in z["label_text"]]
            else:
                path = json3d_tree.write_tree(root, z, dataset, images=True)
                lines = [int(n) for n in z["rec_n"]]
            fullest = int(np.argmax(lines))
            calib6 = P2 = None
            for run in RUNS[dataset]:
                mode, seed, items = str(z[f"{run}/mode"]), int(z[f"{run}/seed"]), [int(i) for i in z[f"{run}/items"]]
                over = dict(cam_dis=bool(int(z[f"{run}/cam_dis"])), mixup=float(z[f"{run}/mixup"]))
                if dataset == "kitti":
                    args = R.model_args(seed=0, load_depth_maps=False, **over)
                    ds = K.KITTIDataset(os.path.join(root, "ImageSets", f"{'val' if mode == 'val' else 'train'}.txt"), mode, args)
                    ids = list(range(len(lines)))
                else:
                    args = R.model_args(seed=0, load_depth_maps=False, overfit=False, **over)
                    ds = (Wm.WaymoDataset if dataset == "waymo" else O.Omni3Dataset)(path, mode, args)
                    ds.use_camera_dis = over["cam_dis"]
                    ids = list(ds.imgs)
                assert bool(ds.use_camera_dis) == over["cam_dis"]
                if calib6 is None:
                    cal = [ds.get_calib(i) for i in ids]
                    calib6 = np.array([[float(c.cu), float(c.cv), float(c.fu), float(c.fv), float(c.tx), float(c.ty)] for c in cal], np.float64)
                    P2 = np.stack([np.asarray(c.P2, np.float64).reshape(3, 4) for c in cal])
                    out[f"{dataset}/calib6"], out[f"{dataset}/P2"] = calib6, P2
                batch = mint_batch(ds, type(ds).collate_fn, seed, items)
                counts = decode(ds, KU, batch, z, run, out, f"{dataset}/{run}", stats)
                if run in ("val", "default"):
                    assert fullest in items, f"{dataset}/{run}: the frame with the most label lines ({fullest}) is not in the batch"
                    assert counts[items.index(fullest)] == counts.max(), (dataset, run, counts)
                summary.append(f"{dataset}/{run}: {len(items)} images, {int(counts.sum())} boxes (most {int(counts.max())})")
        finally:
            shutil.rmtree(root, ignore_errors=True)
        # what the tests rely on, from the reference's output alone
        assert stats["empty"] >= 1, f"{dataset}: no image without boxes"
        assert stats["classes"] == {0, 1, 2}, f"{dataset}: classes {stats['classes']}"
        assert stats["angle_wraps"] >= 1, f"{dataset}: class2angle never wraps"
        assert stats["ry_high"] >= 1 and stats["ry_low"] >= 1, f"{dataset}: alpha2ry wraps {stats['ry_high']} / {stats['ry_low']}"
        assert stats["margin"] >= MARGIN, f"{dataset}: a wrap decision lies {stats['margin']:.3g} rad from its edge"
        summary.append(f"{dataset}: class2angle wraps {stats['angle_wraps']}, alpha2ry wraps +{stats['ry_high']} / -{stats['ry_low']}, nearest "
                       f"decision {stats['margin']:.3g} rad, images without boxes {stats['empty']}, nearest val corner {stats['min_depth']:.2f} m")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 100 * 1024, size
    print("\n".join(summary))
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
