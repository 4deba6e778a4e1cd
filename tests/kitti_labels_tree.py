"""The synthetic KITTI tree of tests/golden/kitti_labels.npz (minted by tools/make_golden_kitti_labels.py): frame pixels, the tree
rebuilt from the fixture's label / calibration text, and the argument sets of its recorded runs."""
import os

import numpy as np

from conftest import GOLDEN


def frame_pixels(i, W, H):
    """the deterministic RGB content of frame i (H, W, 3) uint8"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(xx * (3 + c) + yy * (5 + 2 * c) + 37 * i + 85 * c) % 256 for c in range(3)], -1).astype(np.uint8)


def fixture():
    return np.load(os.path.join(GOLDEN, "kitti_labels.npz"))


def write_tree(root, z, images=False):
    """the fixture's frames as a KITTI directory under root (ImageSets/train.txt and val.txt list all of them)"""
    for sub in ("training/image_2", "training/calib", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    n = len(z["label_text"])
    for i in range(n):
        open(os.path.join(root, "training/label_2", f"{i:06d}.txt"), "w").write(str(z["label_text"][i]))
        open(os.path.join(root, "training/calib", f"{i:06d}.txt"), "w").write(str(z["calib_text"][i]))
        if images:
            from PIL import Image
            W, H = (int(v) for v in z["frame_wh"][i])
            Image.fromarray(frame_pixels(i, W, H), "RGB").save(os.path.join(root, "training/image_2", f"{i:06d}.png"))
    for split in ("train", "val"):
        open(os.path.join(root, "ImageSets", f"{split}.txt"), "w").write("".join(f"{i:06d}\n" for i in range(n)))
    return root


def argset(z, name):
    """(mode, data_args namespace, seed, items) of a recorded run"""
    from yolov10_3d_amd import kitti
    args = kitti.data_args(cam_dis=bool(int(z[f"{name}/cam_dis"])), mixup=float(z[f"{name}/mixup"]))
    return str(z[f"{name}/mode"]), args, int(z[f"{name}/seed"]), [int(i) for i in z[f"{name}/items"]]


def frame_info_fn(root, z):
    """sample_augment's frame_info over the rebuilt tree"""
    from yolov10_3d_amd import kitti

    def info(pos):
        P = kitti.read_calib(os.path.join(root, "training/calib", f"{pos:06d}.txt"))
        lab = kitti.read_label(os.path.join(root, "training/label_2", f"{pos:06d}.txt"))
        return (P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(lab["type"]), tuple(int(v) for v in z["frame_wh"][pos])

    return info


def per_image(z, name, key):
    """the reference-collated per-box key of a run, split back into its images"""
    bi = z[f"{name}/c/batch_idx"].astype(np.int64)
    v = z[f"{name}/c/{key}"]
    return [v[bi == b] for b in range(len(z[f"{name}/items"]))]
