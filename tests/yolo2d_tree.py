"""The synthetic 2D dataset of tests/golden/yolo2d_labels.npz (minted by tools/make_golden_yolo2d.py): twelve small frames
(landscape, portrait, square; smaller and larger than imgsz = 64), their deterministic pixels, the tree written from the fixture's
label text, and the fixture's recorded samples as the plain records `yolo2d.sample_augment` returns."""
import os

import numpy as np

IMGSZ = 64
BATCH = 16
# (W, H) of the twelve frames
FRAME_WH = [(100, 60), (60, 100), (64, 64), (48, 32), (32, 48), (80, 80), (96, 40), (40, 96), (64, 48), (50, 50), (90, 70), (72, 100)]
ARGSETS = {  # name -> (mode, argument overrides, seed, items)
    "default": ("train", dict(), 33, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0, 5]),
    "nomixup": ("train", dict(mixup=0.0), 22, [3, 1, 4, 1, 5, 9, 2, 6]),
    "nomosaic": ("train", dict(mosaic=0.0), 33, [0, 1, 2, 3, 5, 8, 10, 11]),
    "rotshear": ("train", dict(degrees=10.0, shear=2.0), 44, [11, 10, 9, 8, 7, 6]),
    "flipud": ("train", dict(flipud=0.5), 55, [2, 7, 1, 8, 2, 8]),
    "val": ("val", dict(), 66, [0, 3, 5, 6, 9, 11]),
}


def frame_pixels(i, W, H):
    """the deterministic RGB content of frame i (H, W, 3) uint8: smooth ramps plus a coarse checker, so interpolation matters"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(xx * (3 + c) + yy * (2 + 3 * c) + 37 * i + 71 * c + 40 * (((xx // 7) + (yy // 5) + c) % 2)) % 256 for c in range(3)],
                    -1).astype(np.uint8)


def write_tree(root, label_text, frame_wh=FRAME_WH):
    """root/images/NNNNNN.png + root/labels/NNNNNN.txt -> the images directory"""
    from PIL import Image
    img_dir, lab_dir = os.path.join(root, "images"), os.path.join(root, "labels")
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(lab_dir, exist_ok=True)
    for i, (W, H) in enumerate(frame_wh):
        p = os.path.join(img_dir, f"{i:06d}.png")
        if not os.path.exists(p):
            Image.fromarray(frame_pixels(i, W, H), "RGB").save(p)
        text = str(label_text[i])
        if text:
            open(os.path.join(lab_dir, f"{i:06d}.txt"), "w").write(text)
    return img_dir


_Z = {}


def fixture():
    if "z" not in _Z:
        from conftest import GOLDEN
        _Z["z"] = dict(np.load(os.path.join(GOLDEN, "yolo2d_labels.npz")))
    return _Z["z"]


_TILE_KEYS = ("frame", "h0", "w0", "h", "w", "x1a", "y1a", "x2a", "y2a", "padw", "padh")
_LAYER_I, _LAYER_F = 55, 29  # ints / floats per layer in the fixture's two flat arrays per sample


def pack_sample(s):
    """a `yolo2d.sample_augment` record -> {"i": int64 (117,), "f": float64 (69,)} (the fixture's storage; float32 M is exact in float64)"""
    hsv = s["hsv_u"] is not None
    i = [s["index"], int(s["mix"]), s["partner"], int(s["flipud"]), int(s["fliplr"]), int(s["rgb"]), int(hsv)]
    f = [s["p_mixup"], s["r"], s["p_flipud"], s["p_fliplr"], s["p_bgr"]] + list(s["hsv_u"] if hsv else np.zeros(3)) + list(s["hsv_gain"] if hsv else np.zeros(3))
    for pre in (s["pre"], s["pre2"]):
        li, lf = np.zeros(_LAYER_I, np.int64), np.zeros(_LAYER_F, np.float64)
        if pre is not None:
            li[:7] = (1, pre["index"], int(pre["mosaic"]), pre["yc"], pre["xc"], pre["canvas"], int(pre["warp"]))
            li[7:7 + len(pre["others"])] = pre["others"]
            li[10] = len(pre["tiles"])
            for k, t in enumerate(pre["tiles"]):
                li[11 + 11 * k:22 + 11 * k] = [t[q] for q in _TILE_KEYS]
                lf[21 + 2 * k:23 + 2 * k] = (t["lab_padw"], t["lab_padh"])
            lf[:4] = (pre["p_mosaic"], pre["scale"], pre.get("yc_u", -1.0), pre.get("xc_u", -1.0))
            lf[4:4 + len(pre["affine"])] = pre["affine"]
            lf[12:21] = np.asarray(pre["M"], np.float32).reshape(9)
        i += list(li)
        f += list(lf)
    return {"i": np.array(i, np.int64), "f": np.array(f, np.float64)}


def _unpack_pre(li, lf, train):
    from yolov10_3d_amd import yolo2d
    if not li[0]:
        return None
    tiles = [dict(zip(_TILE_KEYS, (int(v) for v in li[11 + 11 * k:22 + 11 * k])), lab_padw=float(lf[21 + 2 * k]), lab_padh=float(lf[22 + 2 * k]))
             for k in range(int(li[10]))]
    mosaic, warp = bool(li[2]), bool(li[6])
    M = lf[12:21].astype(np.float32).reshape(3, 3)
    return dict(index=int(li[1]), mosaic=mosaic, yc=int(li[3]), xc=int(li[4]), canvas=int(li[5]), warp=warp,
                others=[int(v) for v in li[7:10]] if mosaic else [], tiles=tiles, p_mosaic=float(lf[0]), scale=float(lf[1]), yc_u=float(lf[2]),
                xc_u=float(lf[3]), affine=[float(v) for v in lf[4:12]] if train else [], M=M,
                M_inv=yolo2d.invert_affine(M) if warp else np.array([1.0, 0, 0, 0, 1.0, 0]))


def sample(name, n, z=None):
    """sample n of argument set `name` as a `yolo2d.sample_augment` record"""
    z = fixture() if z is None else z
    i, f = z[f"{name}/s{n}/i"], z[f"{name}/s{n}/f"]
    hsv, train = bool(i[6]), ARGSETS[name][0] == "train"
    return dict(mode=ARGSETS[name][0], index=int(i[0]), mix=bool(i[1]), partner=int(i[2]), flipud=bool(i[3]), fliplr=bool(i[4]), rgb=bool(i[5]),
                p_mixup=float(f[0]), r=float(f[1]), p_flipud=float(f[2]), p_fliplr=float(f[3]), p_bgr=float(f[4]),
                hsv_u=f[5:8].copy() if hsv else None, hsv_gain=f[8:11].copy() if hsv else None,
                pre=_unpack_pre(i[7:7 + _LAYER_I], f[11:11 + _LAYER_F], train),
                pre2=_unpack_pre(i[7 + _LAYER_I:], f[11 + _LAYER_F:], train))


def flat_draws(s):
    """the draws of a sample record in the reference's order, as (generator function, value) pairs"""
    def pre(p):
        d = [("uniform", p["p_mosaic"])]
        if p["mosaic"]:
            d += [("choices", list(p["others"])), ("uniform", p["yc_u"]), ("uniform", p["xc_u"])]
        return d + [("uniform", v) for v in p["affine"]]

    d = []
    if s["mode"] == "train":
        d += pre(s["pre"]) + [("uniform", s["p_mixup"])]
        if s["mix"]:
            d += [("randint", s["partner"])] + pre(s["pre2"]) + [("beta", s["r"])]
        if s["hsv_u"] is not None:
            d += [("np.uniform", [float(v) for v in s["hsv_u"]])]
        d += [("random", s["p_flipud"]), ("random", s["p_fliplr"])]
    return d + [("uniform", s["p_bgr"])]


def label_rows(z=None):
    """the twelve frames' (n, 5) float32 label rows, parsed from the fixture's label text as the reader parses a file"""
    z = fixture() if z is None else z
    out = []
    for text in z["label_text"]:
        rows = [ln.split() for ln in str(text).strip().splitlines() if len(ln)]
        out.append(np.array(rows, np.float32).reshape(-1, 5))
    return out


def images():
    return {i: frame_pixels(i, W, H) for i, (W, H) in enumerate(FRAME_WH)}
