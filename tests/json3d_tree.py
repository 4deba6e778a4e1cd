"""The synthetic Waymo / Omni3D splits of tests/golden/waymo_labels.npz and omni3d_labels.npz (minted by
tools/make_golden_json3d_labels.py): frame pixels, the split rebuilt from the fixture's JSON text, and the argument sets of its
recorded runs."""
import json
import os

import numpy as np

from conftest import GOLDEN

DATASETS = ("waymo", "omni3d")
RUNS = ("default", "more", "camdis", "val", "nomix")
KEYS = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res")


def frame_pixels(i, W, H):
    """the deterministic RGB content of the frame at dataset position i (H, W, 3) uint8"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(xx * (5 + c) + yy * (3 + 2 * c) + 41 * i + 67 * c) % 256 for c in range(3)], -1).astype(np.uint8)


_Z = {}


def fixture(dataset):
    if dataset not in _Z:
        _Z[dataset] = dict(np.load(os.path.join(GOLDEN, f"{dataset}_labels.npz")))
    return _Z[dataset]


def image_relpath(dataset, im):
    """where the dataset's get_image looks for a frame, relative to the split file's directory"""
    return im["file_name"] if dataset == "waymo" else im["file_path"].replace("waymo/images/", "")


def write_tree(root, z, dataset, images=False):
    """the fixture's split JSON under root (and its frames' PNGs) -> the JSON's path"""
    path = os.path.join(root, "split.json")
    text = str(z["json_text"])
    open(path, "w").write(text)
    if images:
        from PIL import Image
        raw = json.loads(text)
        for pos, im in enumerate(sorted(raw["images"], key=lambda im: im["id"])):
            p = os.path.join(root, image_relpath(dataset, im))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            W, H = (int(v) for v in z["frame_wh"][pos])
            Image.fromarray(frame_pixels(pos, W, H), "RGB").save(p)
    return path


def argset(z, name):
    """(mode, data_args namespace, seed, items) of a recorded run"""
    from yolov10_3d_amd import kitti
    args = kitti.data_args(cam_dis=bool(int(z[f"{name}/cam_dis"])), mixup=float(z[f"{name}/mixup"]))
    return str(z[f"{name}/mode"]), args, int(z[f"{name}/seed"]), [int(i) for i in z[f"{name}/items"]]


def per_image(z, name, key):
    """the reference-collated per-box key of a run, split back into its images"""
    bi = z[f"{name}/c/batch_idx"].astype(np.int64)
    v = z[f"{name}/c/{key}"]
    return [v[bi == b] for b in range(len(z[f"{name}/items"]))]
