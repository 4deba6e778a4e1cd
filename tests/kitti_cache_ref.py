"""Numpy restatement of `y3d_kitti_plan_batch` (csrc/kitti_cache.hip): the per-image tables of the image augmentation and the label
encoder from a resident split's frame tables and one table of draws.  Copies and one exact float32 -> float64 widening, so the kernel
must agree bit for bit.  test_hip_kitti_cache.py pins this restatement to `kitti.pack_labels` and to the frames' pixels."""
import numpy as np

OUTPUTS = (("src", np.int64, ()), ("src2", np.int64, ()), ("hw", np.int32, (2,)), ("flip", np.int32, ()), ("trans_inv", np.float64, (6,)),
           ("img_i", np.int32, (7,)), ("img_f", np.float64, (19,)), ("mixed", np.uint8, ()))


def draw_rows(positions, partners, flips, scales, trans, trans_inv):
    """the (B, 16) float64 draw table: [position, partner or -1, flip, scale, trans (6), trans_inv (6)]"""
    B = len(positions)
    d = np.zeros((B, 16), np.float64)
    d[:, 0], d[:, 1], d[:, 2], d[:, 3] = positions, partners, [int(bool(f)) for f in flips], scales
    d[:, 4:10] = np.asarray(trans, np.float64).reshape(B, 6)
    d[:, 10:16] = np.asarray(trans_inv, np.float64).reshape(B, 6)
    return d


def plan(base, img_off, frame_hw, rec_span, P2, draws):
    """base: the arena's address; img_off (N) int64, frame_hw (N, 2) int32 (H, W), rec_span (N, 2) int32 (first row, lines), P2 (N, 2, 12)
    float32 (as read, mirrored), draws (B, 16) float64 -> {name: array} of the kernel's eight outputs"""
    B = len(draws)
    o = {k: np.zeros((B,) + s, dt) for k, dt, s in OUTPUTS}
    for b, d in enumerate(draws):
        pos, par, fl = int(d[0]), int(d[1]), int(d[2] != 0)
        H, W = (int(v) for v in frame_hw[pos])
        o["src"][b] = base + int(img_off[pos])
        o["src2"][b] = base + int(img_off[par]) if par >= 0 else 0
        o["hw"][b] = (H, W)
        o["flip"][b] = fl
        o["trans_inv"][b] = d[10:16]
        row0, n0 = (int(v) for v in rec_span[pos])
        row1, n1 = (int(v) for v in rec_span[par]) if par >= 0 else (row0 + n0, 0)  # no partner: an empty span behind the primary's
        o["img_i"][b] = (row0, n0, row1, n1, fl, W, H)
        o["img_f"][b, :12] = P2[pos, fl].astype(np.float64)
        o["img_f"][b, 12:18] = d[4:10]
        o["img_f"][b, 18] = d[3]
        o["mixed"][b] = par >= 0
    return o
