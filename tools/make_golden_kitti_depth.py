"""Mints tests/golden/kitti_depth_map.npz from the REFERENCE's `KITTIDataset.__getitem__` with `load_depth_maps=True`
(data/datasets/kitti.py), run on the CPU in a process of its own.

    python tools/make_golden_kitti_depth.py      # needs the reference checkout (oracle.ref_shim.import_reference)

The tree is the one of tests/golden/kitti_labels.npz (tests/kitti_labels_tree.py: 12 frames at real KITTI sizes, a 55-line frame, a
frame where nothing survives) plus one segmentation mask per frame, `depth_map_ref.synthetic_mask`: every label line's box painted
with its line index, stripes of ids no line can carry, 8- and 16-bit files alternating.  Three runs are recorded, each over a seeded
sequence of items the way a `workers=0` DataLoader draws them: `train` with mixup, `train` without, `val`.  Per run the fixture holds
the seed, the items, the draws this package's `sample_augment` replays from that seed (checked here against the reference's own
`trans_inv` and `mixed`) and the reference's `depth_map` of every item as float64 (an image without kept objects gives an integer
map of zeros there).

OpenCV is absent: `cv2.imread(path, -1)` is served by Pillow (the file's own array, unchanged) and `cv2.getAffineTransform` by the exact
float64 three-point solve, for the duration of the run.  The fixture holds data only.
"""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402
import depth_map_ref as DR  # noqa: E402
from kitti_labels_tree import fixture, frame_info_fn, write_tree  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kitti_depth_map.npz")
RUNS = {  # name -> (dataset mode, argument overrides, seed, items)
    "mix": ("train", dict(), 511, [0, 2, 5, 7, 9, 4]),
    "nomix": ("train", dict(mixup=0.0), 622, [1, 2, 5, 6, 10]),
    "val": ("val", dict(), 733, [0, 2, 5, 8]),
}


def write_masks(root, z):
    from PIL import Image
    for i in range(len(z["label_text"])):
        W, H = (int(v) for v in z["frame_wh"][i])
        m = DR.synthetic_mask(DR.parse_label(str(z["label_text"][i])), i, W, H, DR.mask_bits(i))
        Image.fromarray(m).save(os.path.join(root, "training/image_2", f"{i:06d}_seg.png"))


def affine_from_points(src, dst):
    """cv2.getAffineTransform: the exact 2x3 map through three point pairs, in float64"""
    A = np.hstack((np.asarray(src, np.float64), np.ones((3, 1))))
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T.copy()


def imread(path, flags=-1):
    """cv2.imread(path, -1) for a single-channel PNG: the file's array, unchanged"""
    from PIL import Image
    assert flags == -1
    with Image.open(path) as im:
        return np.array(im)


def main():
    R.import_reference()
    from ultralytics.data.datasets import kitti as K
    from ultralytics.data.datasets import kitti_utils as KU
    from yolov10_3d_amd import kitti
    cv2 = sys.modules["cv2"]
    cv2.getAffineTransform, cv2.imread = affine_from_points, imread
    K.cv2 = KU.cv2 = cv2
    z = fixture()
    root = tempfile.mkdtemp(prefix="y3d_kitti_depth_")
    try:
        write_tree(root, z, images=True)
        write_masks(root, z)
        info = frame_info_fn(root, z)
        out = {"runs": np.array(list(RUNS)), "resolution": np.array(kitti.RESOLUTION, np.int64)}
        for name, (mode, over, seed, items) in RUNS.items():
            args = R.model_args(seed=0, load_depth_maps=True, **over)
            ds = K.KITTIDataset(os.path.join(root, "ImageSets", f"{'val' if mode == 'val' else 'train'}.txt"), mode, args)
            np.random.seed(seed)
            got = [ds[i] for i in items]
            np.random.seed(seed)
            draws = kitti.sample_augment(len(ds), items, info, kitti.data_args(mixup=args.mixup), mode)
            maps, integer = [], []
            for o, d in zip(got, draws):
                assert np.array_equal(o["info"]["trans_inv"], d["trans_inv"]) and int(o["mixed"]) == int(d["mixed"]), name
                m = o["depth_map"].numpy()
                assert m.shape == (kitti.RESOLUTION[1], kitti.RESOLUTION[0]), m.shape
                integer.append(int(m.dtype.kind in "iu"))
                maps.append(m.astype(np.float64))
            out[f"{name}/mode"], out[f"{name}/seed"], out[f"{name}/mixup"] = np.array(mode), np.array(seed), np.array(float(args.mixup))
            out[f"{name}/items"] = np.array(items, np.int64)
            out[f"{name}/depth_map"] = np.stack(maps)
            out[f"{name}/integer_map"] = np.array(integer, np.int64)
            for k in ("mixed", "flip", "crop", "partner"):
                out[f"{name}/{k}"] = np.array([int(d[k]) for d in draws], np.int64)
            out[f"{name}/scale"] = np.array([d["scale"] for d in draws], np.float64)
            out[f"{name}/trans"] = np.stack([d["trans"] for d in draws])
            out[f"{name}/trans_inv"] = np.stack([d["trans_inv"] for d in draws])
            fg = [float((m > 0).mean()) for m in maps]
            print(f"{name}: items {items}, mixed {[int(d['mixed']) for d in draws]}, flip {[int(d['flip']) for d in draws]}, "
                  f"foreground share {[round(v, 3) for v in fg]}")
        np.savez_compressed(OUT, **out)
        print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
