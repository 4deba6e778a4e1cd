"""Support for the 3D predictor's tests: a float64 numpy restatement of the box corners and their projection
(kitti_utils.py Object3d.generate_corners3d :98-114, Calibration.corners3d_to_img_boxes :266-284), the `synth` recipe for post-processed
predictions, and the synthetic KITTI tree's frames copied into an unlabelled `testing/` split."""
import os
import shutil

import numpy as np
import torch

from conftest import GOLDEN


def fixture():
    return dict(np.load(os.path.join(GOLDEN, "predict3d.npz")))


def decode_fixture():
    return dict(np.load(os.path.join(GOLDEN, "kitti_decode.npz")))


def corners(rows, P2):
    """rows (n, 14) [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score], P2 (3, 4) -> corners3d (n, 8, 3), corners_img (n, 8, 2),
    float64: R_y(ry) applied to the box template, + the position (y is the bottom face), then the full 3 x 4 projection"""
    rows = np.asarray(rows, np.float64).reshape(-1, 14)
    P = np.asarray(P2, np.float64).reshape(3, 4)
    h, w, l, ry = rows[:, 6], rows[:, 7], rows[:, 8], rows[:, 12]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64)
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64)
    top = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.float64)
    xc, zc, yc = sx[None] * (l / 2)[:, None], sz[None] * (w / 2)[:, None], -top[None] * h[:, None]
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    X = c * xc + s * zc + rows[:, 9:10]
    Y = yc + rows[:, 10:11]
    Z = -s * xc + c * zc + rows[:, 11:12]
    c3 = np.stack([X, Y, Z], -1)
    hom = np.concatenate([c3, np.ones(c3.shape[:2] + (1,))], -1) @ P.T
    return c3, hom[..., :2] / hom[..., 2:3]


def synth(gen, B, K):
    """post-processed rows (B, K, 37) float32: boxes inside a 1280 x 384 canvas, depth 3 .. 63 m, labels 0 .. 2 (the recipe of the
    decode fixture)"""
    u = lambda *s: torch.rand(*s, generator=gen)
    n = lambda *s: torch.randn(*s, generator=gen)
    x1, y1 = u(B, K) * 1000, u(B, K) * 250
    w, h = 20 + u(B, K) * 250, 20 + u(B, K) * 120
    c3 = torch.stack((x1 + w / 2 + n(B, K) * 3, y1 + h / 2 + n(B, K) * 3), -1)
    preds = torch.cat((torch.stack((x1, y1, x1 + w, y1 + h), -1), c3, n(B, K, 3) * 0.2, n(B, K, 24), 3 + u(B, K, 1) * 60, n(B, K, 1),
                       n(B, K, 1) * 4, torch.randint(0, 3, (B, K, 1), generator=gen).float()), -1)
    return preds.float().contiguous()


def synth_camera(B):
    """(calib6 (B, 6), P2 (B, 3, 4) float32, ratio (B, 2), inv_trans (B, 2, 3)) in the style of the decode fixture, for any B"""
    from yolov10_3d_amd import kitti
    P2 = np.zeros((B, 3, 4), np.float32)
    for i in range(B):
        f = 707.0493 + 10 * i
        P2[i] = [[f, 0, 604.0814 + 3 * i, 45.75831 - i], [0, f, 180.5066 - 2 * i, -0.3454157 + 0.1 * i], [0, 0, 1, 0.004981016]]
    calib6 = np.array([kitti.calib_params(p) for p in P2], np.float64)
    ratio = np.array([[1280 / (1242.0 - 2 * i), 384 / (375.0 - i)] for i in range(B)], np.float64)
    inv = np.array([[[0.97 + 0.01 * i, 0.0, 1.5 * i], [0.0, 0.976 - 0.01 * i, -0.75 * i]] for i in range(B)], np.float64)
    return calib6, P2, ratio, inv


def add_testing_split(root, ids):
    """copies training/{image_2, calib} of the frames `ids` into testing/ and lists them in ImageSets/test.txt"""
    for sub in ("image_2", "calib"):
        os.makedirs(os.path.join(root, "testing", sub), exist_ok=True)
    for i in ids:
        shutil.copy(os.path.join(root, "training/image_2", f"{i:06d}.png"), os.path.join(root, "testing/image_2", f"{i:06d}.png"))
        shutil.copy(os.path.join(root, "training/calib", f"{i:06d}.txt"), os.path.join(root, "testing/calib", f"{i:06d}.txt"))
    open(os.path.join(root, "ImageSets", "test.txt"), "w").write("".join(f"{i:06d}\n" for i in ids))
    return root
