"""Support for the label-decode tests: a float64 NumPy restatement of `KITTIDataset.decode_batch` (data/datasets/kitti.py:469-513) in the
output layout of `y3d_decode_labels`, the inputs of the reference fixture tests/golden/decode_batch.npz (taken from the label fixtures
it was minted next to), and the crafted rows of the GPU tests.  The corners and their projection are tests/predict3d_ref.py's."""
import os

import numpy as np

import json3d_tree
import kitti_labels_tree
import predict3d_ref as PR
from conftest import GOLDEN

KEYS = ("cls", "bboxes", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx")
WIDTH = {"cls": 1, "bboxes": 4, "center_3d": 2, "size_3d": 3, "depth": 1, "heading_bin": 1, "heading_res": 1, "batch_idx": 1}
DTYPES = {"cls": np.int64, "bboxes": np.float64, "center_3d": np.float64, "size_3d": np.float64, "depth": np.float64,
          "heading_bin": np.int64, "heading_res": np.float64, "batch_idx": np.float32}
RUNS = {"kitti": ("val", "default", "camdis"), "waymo": ("val", "default"), "omni3d": ("val", "default", "nomix")}
KITTI_MEAN = ((1.52563191462, 1.62856739989, 3.88311640418), (1.76255119, 0.66068622, 0.84422524), (1.73698127, 0.59706367, 1.76282397))
WAYMO_MEAN = ((1.7974, 2.106, 4.8117), (1.751, 0.85498, 0.90977), (1.7697, 0.83474, 1.769))
MEAN = {"kitti": KITTI_MEAN, "waymo": WAYMO_MEAN, "omni3d": KITTI_MEAN}
SIX_MEAN = KITTI_MEAN + WAYMO_MEAN  # a table of six classes
PI = np.pi


def owners(lab, counts_in, B):
    """per image the indices of its rows, in order: the static layout's leading counts_in[b] rows of its block, or the ragged layout's
    rows with batch_idx == b"""
    N = len(np.asarray(lab["cls"]).reshape(-1))
    if counts_in is not None:
        M = N // B
        return [np.arange(b * M, b * M + min(max(int(counts_in[b]), 0), M)) for b in range(B)]
    bi = np.asarray(lab["batch_idx"]).reshape(-1)
    return [np.nonzero(bi == np.float32(b))[0] for b in range(B)]


def decode_rows(lab, idx, ori_hw, calib6, ratio, trans_inv, mean_size, undo_augment, use_camera_dis):
    """the rows `idx` of one image -> (n, 14) float64, decode_batch line by line"""
    f = lambda k: np.asarray(lab[k]).reshape(-1, WIDTH[k])[idx].astype(np.float64)
    n = len(idx)
    ms = np.asarray(mean_size, np.float64).reshape(-1, 3)
    cls = np.asarray(lab["cls"]).reshape(-1)[idx].astype(np.int64)
    box, c3d, depth = f("bboxes"), f("center_3d"), f("depth")[:, 0]
    H, W = float(ori_hw[0]), float(ori_hw[1])
    cu, cv, fu, fv, tx, ty = (float(v) for v in calib6)
    x = box[:, 0] * W
    dw, dh = box[:, 2] / 2, box[:, 3] / 2
    xyxy = np.stack([(box[:, 0] - dw) * W, (box[:, 1] - dh) * H, (box[:, 0] + dw) * W, (box[:, 1] + dh) * H], 1)
    dims = f("size_3d") + ms[np.clip(cls, 0, len(ms) - 1)]  # outside the table: the nearest entry (the reference raises)
    if undo_augment:  # affine_transform builds its point in float32 (kitti_utils.py:467-470)
        t = np.asarray(trans_inv, np.float64).reshape(6)
        px, py = c3d[:, 0].astype(np.float32).astype(np.float64), c3d[:, 1].astype(np.float32).astype(np.float64)
        u, v = (t[0] * px + t[1] * py) + t[2], (t[3] * px + t[4] * py) + t[5]
    else:
        u, v = c3d[:, 0] / float(ratio[0]), c3d[:, 1] / float(ratio[1])
    with np.errstate(all="ignore"):
        if use_camera_dis:
            fd = np.sqrt((u - cu) * (u - cu) + (v - cv) * (v - cv) + fu * fu)
            lx = ((u - cu) * depth) / fd + tx
            ly = ((v - cv) * depth) / fd + ty
            lz = np.sqrt(depth * depth - lx * lx - ly * ly)
        else:
            lx = ((u - cu) * depth) / fu + tx
            ly = ((v - cv) * depth) / fv + ty
            lz = depth
    ly = ly + dims[:, 0] / 2
    alpha = f("heading_bin")[:, 0] * (2 * PI / 12.0) + f("heading_res")[:, 0]
    alpha = np.where(alpha > PI, alpha - 2 * PI, alpha)
    ry = alpha + np.arctan2(x - cu, fu)
    ry = np.where(ry > PI, ry - 2 * PI, ry)
    ry = np.where(ry < -PI, ry + 2 * PI, ry)
    return np.concatenate([cls[:, None].astype(np.float64), alpha[:, None], xyxy, dims, np.stack([lx, ly, lz, ry], 1), np.ones((n, 1))], 1)


def decode(lab, counts_in, ori_shape, calib6, ratio_pad, trans_inv, P2, mean_size, undo_augment, use_camera_dis, R):
    """-> rows (B, R, 14), corners3d (B, R, 8, 3), corners_img (B, R, 8, 2) or None, counts (B,) int32 as y3d_decode_labels lays them out"""
    B = len(ori_shape)
    rp = np.asarray(ratio_pad, np.float64)
    ratio = rp[:, 0] if rp.ndim == 3 else rp
    rows, c3, counts = np.zeros((B, R, 14)), np.zeros((B, R, 8, 3)), np.zeros(B, np.int32)
    ci = None if P2 is None else np.zeros((B, R, 8, 2))
    for b, idx in enumerate(owners(lab, counts_in, B)):
        idx = idx[:R]
        n = counts[b] = len(idx)
        if not n:
            continue
        rows[b, :n] = decode_rows(lab, idx, ori_shape[b], calib6[b], ratio[b], None if trans_inv is None else trans_inv[b], mean_size,
                                  undo_augment, use_camera_dis)
        with np.errstate(all="ignore"):
            w3, wi = PR.corners(rows[b, :n], np.eye(3, 4) if P2 is None else P2[b])
        c3[b, :n] = w3
        if ci is not None:
            ci[b, :n] = wi
    return rows, c3, ci, counts


# ---------------------------------------------------------------------------------------------------------------- the reference fixture
_G = {}


def fixture():
    if not _G:
        _G.update(np.load(os.path.join(GOLDEN, "decode_batch.npz")))
    return _G


def label_fixture(dataset):
    return kitti_labels_tree.fixture() if dataset == "kitti" else json3d_tree.fixture(dataset)


def fixture_inputs(dataset, run):
    """the reference-collated batch of a recorded run -> dict: `lab` (the per-box arrays in the reference's own dtypes), `B`, `items`,
    `ori_shape` (B, 2) (height, width), `calib6`, `P2` (the ORIGINAL calibrations), `ratio_pad` (B, 2, 2), `trans_inv` (B, 2, 3),
    `mean_size`, `cam_dis`"""
    z, g = label_fixture(dataset), fixture()
    items = [int(i) for i in z[f"{run}/items"]]
    lab = {k: z[f"{run}/c/{k}"] for k in KEYS}
    return dict(lab=lab, B=len(items), items=items, ori_shape=z["frame_wh"][items][:, ::-1].astype(np.float64), calib6=g[f"{dataset}/calib6"][items],
                P2=g[f"{dataset}/P2"][items], ratio_pad=z[f"{run}/c/ratio_pad"].astype(np.float64), trans_inv=z[f"{run}/trans_inv"].astype(np.float64),
                mean_size=MEAN[dataset], cam_dis=bool(int(z[f"{run}/cam_dis"])))


def fixture_rows(dataset, run, undo_augment):
    """the reference's rows of a run, images back to back -> (n, 14), counts (B,)"""
    g = fixture()
    rows = g[f"{dataset}/{run}/rows"].copy()
    if not undo_augment:
        rows[:, 9:12] = g[f"{dataset}/{run}/loc0"]
    return rows, g[f"{dataset}/{run}/counts"]


def ragged(rows, counts):
    """(B, R, ..) with counts -> the kept rows back to back"""
    return np.concatenate([rows[b, :n] for b, n in enumerate(counts)]) if len(counts) else rows[:0, 0]


def typed(lab):
    """the per-box arrays in y3d_decode_labels' dtypes and shapes (exact widenings of the reference's collated dtypes)"""
    return {k: np.ascontiguousarray(np.asarray(lab[k]).reshape(-1, WIDTH[k]) if WIDTH[k] > 1 else np.asarray(lab[k]).reshape(-1)).astype(DTYPES[k])
            for k in KEYS}


def to_static(lab, B, max_objs):
    """ragged per-box arrays -> (static arrays of B * max_objs rows with batch_idx = -1 padding, counts (B,) int32)"""
    t = typed(lab)
    out = {k: np.zeros((B * max_objs,) + t[k].shape[1:], DTYPES[k]) for k in KEYS}
    out["batch_idx"][:] = -1
    counts = np.zeros(B, np.int32)
    for b, idx in enumerate(owners(t, None, B)):
        idx = idx[:max_objs]
        counts[b] = len(idx)
        for k in KEYS:
            out[k][b * max_objs:b * max_objs + len(idx)] = t[k][idx]
    return out, counts


# ---------------------------------------------------------------------------------------------------------------- synthetic batches
def synth(counts, seed, nc=3, shuffle=False):
    """a ragged batch with counts[b] boxes in image b -> (lab, ori_shape, calib6, P2 float64, ratio_pad (B, 2, 2), trans_inv) in the
    style of tests/predict3d_ref.py's camera.  shuffle: the images' rows interleaved (collate_fn never does; the compaction must cope)"""
    rng = np.random.default_rng(seed)
    B = len(counts)
    calib6, P2, ratio, inv = PR.synth_camera(B)
    n = int(sum(counts))
    bi = np.repeat(np.arange(B), counts).astype(np.float32)
    if shuffle:
        bi = bi[rng.permutation(n)]
    w, h = rng.uniform(0.02, 0.3, n), rng.uniform(0.05, 0.4, n)
    cx, cy = rng.uniform(0.15, 0.85, n), rng.uniform(0.25, 0.75, n)
    lab = {"cls": rng.integers(0, nc, (n, 1)), "bboxes": np.stack([cx, cy, w, h], 1),
           "center_3d": np.stack([cx * 1280 + rng.normal(0, 3, n), cy * 384 + rng.normal(0, 3, n)], 1), "size_3d": rng.normal(0, 0.2, (n, 3)),
           "depth": rng.uniform(3, 63, n), "heading_bin": rng.integers(0, 12, n), "heading_res": rng.uniform(-PI / 12, PI / 12, n), "batch_idx": bi}
    ori = np.array([[375.0 - i, 1242.0 - 2 * i] for i in range(B)])
    rp = np.stack([ratio, np.zeros_like(ratio)], 1)
    return typed(lab), ori, calib6, P2.astype(np.float64), rp, inv


def _residual(hbin, target):
    """the residual for which class2angle(hbin, residual, to_label_format=True) is `target` to the bit"""
    apc = 2 * PI / 12
    res = (target if target > 0 else target + 2 * PI) - hbin * apc
    for _ in range(64):
        ang = hbin * apc + res
        got = ang - 2 * PI if ang > PI else ang
        if got == target:
            return res
        res = np.nextafter(res, np.inf if got < target else -np.inf)
    raise AssertionError(f"no residual reaches {target!r} from bin {hbin}")


def _column(alpha, target, W, cu, fu):
    """the box centre bx (a few ulps from 0.5, the principal column of an image 2 cu wide) for which alpha + atan2(bx W - cu, fu) is
    `target` to the bit, before alpha2ry's wrap"""
    for k in range(-64, 65):
        bx = 0.5 + k * 2.0 ** -53 if k < 0 else 0.5 + k * 2.0 ** -52
        if alpha + np.arctan2(bx * W - cu, fu) == target:
            return bx
    raise AssertionError(f"no column reaches {target!r} from {alpha!r}")


def crafted():
    """one image of hand-made rows -> (lab, ori_shape, calib6, P2, ratio_pad, trans_inv, names, want_ry): a heading at bin 11 whose
    residual carries the angle past pi (class2angle wraps) next to one that stays; rotation_y at +-pi exactly (stays) and one ulp on
    either side of each (alpha2ry wraps strictly beyond), steered by box centres a few ulps off the principal column of an image 2 cu
    wide; a box centre behind the camera and one on its plane.  `want_ry` maps those rows' names to their exact rotation_y."""
    calib6, P2, ratio, inv = PR.synth_camera(1)
    cu, fu = calib6[0, 0], calib6[0, 2]
    W = 2.0 * cu
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    names, rows, want_ry = [], [], {}

    def add(name, hbin, res, bx=0.5, depth=20.0):
        names.append(name)
        rows.append((hbin, res, bx, depth))

    add("bin11_wraps", 11, 0.2, bx=0.3)   # 11 * apc + 0.2 > pi -> - 2 pi
    add("bin5_below", 5, 0.25, bx=0.7)
    top, bottom = PI, up(-PI)  # class2angle's range is (-pi, pi]: the largest alpha and the smallest
    for name, alpha, pre, ry in (("ry_pi", top, PI, PI), ("ry_below_pi", down(PI), down(PI), down(PI)), ("ry_above_pi", top, up(PI), up(PI) - 2 * PI),
                                 ("ry_minus_pi", bottom, -PI, -PI), ("ry_above_minus_pi", bottom, up(-PI), up(-PI)),
                                 ("ry_below_minus_pi", bottom, down(-PI), down(-PI) + 2 * PI)):
        hbin = 3 if alpha > 0 else 9
        add(name, hbin, _residual(hbin, alpha), bx=_column(alpha, pre, W, cu, fu))
        want_ry[name] = ry
    add("behind_camera", 2, 0.1, bx=0.4, depth=-7.5)
    add("on_camera_plane", 2, 0.1, bx=0.6, depth=0.0)
    n = len(rows)
    lab = {"cls": np.arange(n).reshape(n, 1) % 3, "bboxes": np.array([[r[2], 0.5, 0.1, 0.2] for r in rows]),
           "center_3d": np.array([[r[2] * 1280, 190.0] for r in rows]), "size_3d": np.zeros((n, 3)), "depth": np.array([r[3] for r in rows]),
           "heading_bin": np.array([r[0] for r in rows]), "heading_res": np.array([r[1] for r in rows]), "batch_idx": np.zeros(n, np.float32)}
    ori = np.array([[375.0, W]])
    return typed(lab), ori, calib6, P2.astype(np.float64), np.stack([ratio, np.zeros_like(ratio)], 1), inv, names, want_ry
