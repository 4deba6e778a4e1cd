"""2D training batches on the device — the data path of the six `v10` models.

Mirrors `YOLODataset.__getitem__` + `collate_fn` of the reference for detection: `load_image` and its mosaic buffer
(data/base.py:147-182, 251-266), `v8_transforms` (data/augment.py:973-1007: Mosaic, RandomPerspective, MixUp, RandomHSV, the two
RandomFlip), `Format` (:915-957) and `collate_fn` (data/dataset.py:206-223).  The plan is that of `kitti.py` / `json3d.py`: the host
reads the files and replays every random draw in the reference's order (`sample_augment`), one launch builds the images
(`y3d_yolo2d_image_aug`) and one the labels (`y3d_yolo2d_encode_labels`, csrc/yolo2d_batch.hip), in a static layout of
`max_boxes or 64` rows per image that `v10DetectLoss.targets` and `GraphedTrainStep` take unchanged.

Labels follow the reference's float32 arithmetic box by box.  Images follow the arithmetic stated in the kernel's header and in
tests/yolo2d_ref.py (float64 bilinear resize / warp, a float HSV round trip); that is not OpenCV's fixed-point interpolation nor its
integer HSV tables, and how far the two lie apart has not been measured (tools/make_golden_yolo2d.py --cv2).

Rectangular validation batches (the validator's `rect=True` dataset: `set_rectangle`, data/base.py:226-249, and `LetterBox` with
`rect_shape`, data/augment.py:696-750) are a class of their own, `RectSplit`: `build_batch(rect_split, ...)` letter-boxes each batch into
its own stride-multiple (H, W) canvas (`y3d_letterbox_image`, `y3d_letterbox_labels`, csrc/letterbox.hip) and returns the `ratio_pad`
that `metrics.BoxStats.update_2d` reads.  `Split(rect=True)` itself keeps raising.

`DeviceSplit` and `DeviceRectSplit` are the same two splits decoded once and held on the device (the reference's `cache="ram"`, one step
further): a batch from them is the draws, one small pinned upload and three launches (`y3d_yolo2d_plan_batch`, csrc/yolo2d_cache.hip,
writes the records of the two kernels from the draws and the split's frame tables), or for a rect batch two launches over records
computed at load — the same batch bit for bit, without opening a file.

Not covered (each raises Y3DError where it can be asked for): rect training batches, segments / keypoints / obb, copy_paste > 0,
perspective != 0, Albumentations, the RNG streams of multi-worker loaders, the mosaic 3 / 9 grids.
"""
from __future__ import annotations

import math
import random

import torch

from . import loss as _loss
from . import ops
from ._lib import Y3DError, lib
from .resident import ResidentSplit, check_plan, span_table
from .resident import upload as _up

IMG_FORMATS = {"bmp", "dng", "jpeg", "jpg", "mpo", "png", "tif", "tiff", "webp", "pfm"}  # data/utils.py
# the 2D data hyper-parameters of cfg/default.yaml
DATA_ARGS = dict(mosaic=1.0, mixup=0.5, degrees=0.0, translate=0.1, scale=0.4, shear=0.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7,
                 hsv_v=0.4, flipud=0.0, fliplr=0.5, bgr=0.0, copy_paste=0.0)
# Refusal-only arguments.  They are no hyper-parameters of default.yaml: they name what a caller of the reference can ask for elsewhere
# (Mosaic(n=...), an installed albumentations, DataLoader(num_workers=...)) and this module does not do.  Any other value raises.
_UNSUPPORTED = dict(mosaic_grid=4, albumentations=False, workers=0)
BASE_CAP = 64
# record widths of the two kernels (include/y3d.h)
_TILE, _LAYER, _REC_I, _REC_F, _LAB_I, _LAB_F = 12, 50, 112, 16, 20, 48
_LB_REC = 8  # y3d_letterbox_image: src, h0, w0, new_h, new_w, top, left, swap_rb


def data_args(**over):
    """DATA_ARGS with overrides, as the attribute namespace sample_augment / build_batch read.  Besides the fourteen hyper-parameters it
    carries three refusal-only arguments, `mosaic_grid=4`, `albumentations=False` and `workers=0`: they exist so that a request for a
    3 / 9 mosaic, for Albumentations or for a multi-worker loader's RNG streams is refused with Y3DError and not silently ignored."""
    from types import SimpleNamespace
    bad = set(over) - set(DATA_ARGS) - set(_UNSUPPORTED)
    if bad:
        raise ValueError(f"data_args: unknown argument(s) {sorted(bad)}")
    return SimpleNamespace(**{**DATA_ARGS, **_UNSUPPORTED, **over})


def _check_args(args):
    if getattr(args, "copy_paste", 0.0):
        raise Y3DError("yolo2d: copy_paste > 0 needs segments, which are not supported")
    if getattr(args, "perspective", 0.0):
        raise Y3DError("yolo2d: perspective != 0 (warpPerspective) is not supported")
    if getattr(args, "mosaic_grid", 4) != 4:
        raise Y3DError("yolo2d: only the 2 x 2 mosaic is supported (no 3 / 9 grids)")
    if getattr(args, "albumentations", False):
        raise Y3DError("yolo2d: Albumentations transforms are not supported")
    if getattr(args, "workers", 0):
        raise Y3DError("yolo2d: the draws replay a workers=0 loader; multi-worker RNG streams are not supported")


def img2label_path(path):
    """data/utils.py img2label_paths: the last /images/ becomes /labels/, the extension .txt"""
    import os
    sa, sb = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    return sb.join(path.rsplit(sa, 1)).rsplit(".", 1)[0] + ".txt"


def read_labels(path):
    """A YOLO txt label file -> (n, 5) float32 rows [cls, x, y, w, h] (normalised xywh); a missing or empty file is a background image"""
    import os
    import numpy as np
    if not os.path.isfile(path):
        return np.zeros((0, 5), np.float32)
    rows = [ln.split() for ln in open(path).read().strip().splitlines() if len(ln)]
    if not rows:
        return np.zeros((0, 5), np.float32)
    if any(len(r) != 5 for r in rows):
        raise Y3DError(f"yolo2d: {path}: rows of {sorted({len(r) for r in rows})} columns; segments / keypoints / obb labels are not supported")
    lb = np.array(rows, dtype=np.float32)
    if lb.min() < 0 or lb[:, 1:].max() > 1:
        raise Y3DError(f"yolo2d: {path}: negative or non-normalised label values")
    return lb


class Split:
    """The images of a directory (recursive) or of list files, sorted as the reference sorts them, with their label rows, their sizes
    and the reference's `buffer` of recently loaded indices (`load_image`: append on load, drop the oldest at
    min(ni, batch * 8, 1000)), from which Mosaic picks its three other tiles."""

    def __init__(self, img_dir_or_list, imgsz=640, batch=16, augment=True, rect=False, task="detect"):
        import glob
        import os
        from pathlib import Path
        if rect:
            raise Y3DError("yolo2d: rect=True (rectangular batches) is not supported")
        if task != "detect":
            raise Y3DError(f"yolo2d: task {task!r}: segments / keypoints / obb are not supported")
        if int(imgsz) % 4 or int(imgsz) < 4:
            raise Y3DError(f"yolo2d: imgsz {imgsz} must be a multiple of 4")
        f = []
        for p in img_dir_or_list if isinstance(img_dir_or_list, (list, tuple)) else [img_dir_or_list]:
            p = Path(p)
            if p.is_dir():
                f += glob.glob(str(p / "**" / "*.*"), recursive=True)
            elif p.is_file():
                parent = str(p.parent) + os.sep
                f += [x.replace("./", parent) if x.startswith("./") else x for x in open(p).read().strip().splitlines()]
            else:
                raise FileNotFoundError(f"{p} does not exist")
        self.im_files = sorted(x.replace("/", os.sep) for x in f if x.split(".")[-1].lower() in IMG_FORMATS)
        if not self.im_files:
            raise FileNotFoundError(f"No images found in {img_dir_or_list}")
        self.label_files = [img2label_path(x) for x in self.im_files]
        self.labels = [read_labels(x) for x in self.label_files]
        self.ni = len(self.im_files)
        self.imgsz, self.batch, self.augment = int(imgsz), int(batch), bool(augment)
        self.buffer = []
        self.max_buffer_length = min((self.ni, self.batch * 8, 1000)) if self.augment else 0
        self._held = set()  # indices whose resized image the reference holds in `ims`: loading them again does not touch the buffer
        self._hw0 = {}

    def __len__(self):
        return self.ni

    def size(self, i):
        """(h0, w0) of image i, from the file header"""
        if i not in self._hw0:
            from PIL import Image
            with Image.open(self.im_files[i]) as im:
                w, h = im.size
                if im.getexif().get(0x0112, 1) in (5, 6, 7, 8):  # EXIF orientations that transpose: cv2.imread applies them
                    w, h = h, w
                self._hw0[i] = (h, w)
        return self._hw0[i]

    def load(self, i):
        """`load_image` without the pixels: ((h0, w0), (h, w) after the resize to long side imgsz), and the buffer update"""
        h0, w0 = self.size(i)
        r = self.imgsz / max(h0, w0)
        h, w = (h0, w0) if r == 1 else (min(math.ceil(h0 * r), self.imgsz), min(math.ceil(w0 * r), self.imgsz))
        if i not in self._held and self.augment:
            self._held.add(i)
            self.buffer.append(i)
            if len(self.buffer) >= self.max_buffer_length:
                self._held.discard(self.buffer.pop(0))
        return (h0, w0), (h, w)

    def decode(self, i, device):
        """image i as a (h0, w0, 3) uint8 RGB tensor on `device`, its EXIF orientation applied as cv2.imread applies it"""
        import numpy as np
        from PIL import Image, ImageOps
        with Image.open(self.im_files[i]) as im:
            return torch.from_numpy(np.array(ImageOps.exif_transpose(im).convert("RGB"))).to(device)


def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(angle=angle, center=(0, 0), scale=scale) in its closed form -> (2, 3) float64"""
    import numpy as np
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * 0.0 - beta * 0.0], [-beta, alpha, beta * 0.0 + (1 - alpha) * 0.0]], np.float64)


def invert_affine(M):
    """The inverse cv2.warpAffine computes of a forward 2x3 map, in float64 -> (6,) output -> source"""
    import numpy as np
    m = np.asarray(M, np.float64)[:2].reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def _pre_transform(split, index, hw, args):
    """`pre_transform` of v8_transforms for an image already loaded: Mosaic (or, when its draw misses, RandomPerspective's LetterBox),
    then the eight `random.uniform` of `affine_transform` (all drawn, also at zero range) and M = T @ S @ R @ P @ C in float32"""
    import numpy as np
    s = split.imgsz
    rec = {"index": int(index), "p_mosaic": random.uniform(0, 1)}
    rec["mosaic"] = not (rec["p_mosaic"] > args.mosaic)
    tiles = []
    if rec["mosaic"]:
        others = random.choices(list(split.buffer), k=3)
        frames = [index] + others
        sizes = [hw] + [split.load(i) for i in others]
        border = (-s // 2, -s // 2)
        yc_u, xc_u = (random.uniform(-x, 2 * s + x) for x in border)  # y first, as the reference's generator draws them
        yc, xc = int(yc_u), int(xc_u)
        for i, (fi, ((h0, w0), (h, w))) in enumerate(zip(frames, sizes)):
            if i == 0:
                x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
                x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
            elif i == 1:
                x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
                x1b, y1b = 0, h - (y2a - y1a)
            elif i == 2:
                x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
                x1b, y1b = w - (x2a - x1a), 0
            else:
                x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
                x1b, y1b = 0, 0
            padw, padh = x1a - x1b, y1a - y1b
            tiles.append(dict(frame=int(fi), h0=h0, w0=w0, h=h, w=w, x1a=x1a, y1a=y1a, x2a=x2a, y2a=y2a, padw=padw, padh=padh,
                              lab_padw=float(padw), lab_padh=float(padh)))
        rec.update(others=[int(i) for i in others], yc=yc, xc=xc, yc_u=yc_u, xc_u=xc_u, canvas=2 * s)
    else:
        (h0, w0), (h, w) = hw
        r = min(s / h, s / w)
        if r != 1.0:
            raise Y3DError(f"yolo2d: letter-box ratio {r} after load_image's resize (expected 1)")
        dw, dh = (s - w) / 2, (s - h) / 2
        top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
        tiles.append(dict(frame=int(index), h0=h0, w0=w0, h=h, w=w, x1a=left, y1a=top, x2a=left + w, y2a=top + h, padw=left, padh=top,
                          lab_padw=float(dw), lab_padh=float(dh)))
        rec.update(others=[], yc=-1, xc=-1, yc_u=-1.0, xc_u=-1.0, canvas=s)
    rec["tiles"] = tiles
    C = np.eye(3, dtype=np.float32)
    C[0, 2] = -rec["canvas"] / 2
    C[1, 2] = -rec["canvas"] / 2
    P = np.eye(3, dtype=np.float32)
    d = [random.uniform(-args.perspective, args.perspective), random.uniform(-args.perspective, args.perspective)]
    P[2, 0], P[2, 1] = d[0], d[1]
    R = np.eye(3, dtype=np.float32)
    a = random.uniform(-args.degrees, args.degrees)
    sc = random.uniform(1 - args.scale, 1 + args.scale)
    R[:2] = rotation_matrix_2d(a, sc)
    S = np.eye(3, dtype=np.float32)
    d += [a, sc, random.uniform(-args.shear, args.shear), random.uniform(-args.shear, args.shear)]
    S[0, 1] = math.tan(d[4] * math.pi / 180)
    S[1, 0] = math.tan(d[5] * math.pi / 180)
    T = np.eye(3, dtype=np.float32)
    d += [random.uniform(0.5 - args.translate, 0.5 + args.translate), random.uniform(0.5 - args.translate, 0.5 + args.translate)]
    T[0, 2] = d[6] * s
    T[1, 2] = d[7] * s
    M = T @ S @ R @ P @ C
    rec.update(affine=[float(v) for v in d], scale=float(sc), M=M, M_inv=invert_affine(M), warp=True)
    return rec


def _letterbox_only(split, index, hw):
    """the `val` transform: LetterBox(scaleup=False), no warp"""
    import numpy as np
    s = split.imgsz
    (h0, w0), (h, w) = hw
    r = min(min(s / h, s / w), 1.0)
    if r != 1.0:
        raise Y3DError(f"yolo2d: letter-box ratio {r} after load_image's resize (expected 1)")
    dw, dh = (s - w) / 2, (s - h) / 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    tile = dict(frame=int(index), h0=h0, w0=w0, h=h, w=w, x1a=left, y1a=top, x2a=left + w, y2a=top + h, padw=left, padh=top,
                lab_padw=float(dw), lab_padh=float(dh))
    return dict(index=int(index), p_mosaic=-1.0, mosaic=False, others=[], yc=-1, xc=-1, yc_u=-1.0, xc_u=-1.0, canvas=s, tiles=[tile], affine=[], scale=1.0,
                M=np.eye(3, dtype=np.float32), M_inv=np.array([1.0, 0, 0, 0, 1.0, 0]), warp=False)


def sample_augment(split, index, args, mode="train"):
    """Every random decision of `dataset[index]` in the reference's order, for a `workers=0` loader seeded through `random.seed` and
    `np.random.seed`.  From `random`: the mosaic probability, `choices(buffer, k=3)`, yc, xc, the eight uniforms of `affine_transform`
    (two perspective, angle, scale, two shear, two translate), the MixUp probability and its `randint`, then — after the partner's own
    `pre_transform` — the two flips and Format's bgr draw; from `np.random`: `beta(32, 32)` and the HSV `uniform(-1, 1, 3)`.
    -> a plain dict: `pre` (and `pre2` for the MixUp partner): index, p_mosaic, mosaic, others, yc, xc, canvas, tiles (frame, sizes,
    canvas rectangle, pads), affine (the eight draws), scale, M (3, 3) float32, M_inv (6,) float64; p_mixup, mix, partner, r; hsv_u
    (3,), hsv_gain (3,) or None; p_flipud, flipud, p_fliplr, fliplr; p_bgr, rgb."""
    import numpy as np
    _check_args(args)
    if mode not in ("train", "val"):
        raise ValueError("mode must be 'train' or 'val'")
    index = int(index)
    if not 0 <= index < split.ni:
        raise IndexError(f"yolo2d: index {index} of {split.ni} images")
    if (mode == "train") != split.augment:
        raise Y3DError(f"yolo2d: mode {mode!r} needs a Split built with augment={mode == 'train'}")
    hw = split.load(index)
    out = dict(mode=mode, index=index, pre2=None, p_mixup=-1.0, mix=False, partner=-1, r=1.0, hsv_u=None, hsv_gain=None, p_flipud=-1.0,
               flipud=False, p_fliplr=-1.0, fliplr=False)
    if mode == "val":
        out["pre"] = _letterbox_only(split, index, hw)
    else:
        out["pre"] = _pre_transform(split, index, hw, args)
        out["p_mixup"] = random.uniform(0, 1)
        out["mix"] = not (out["p_mixup"] > args.mixup)
        if out["mix"]:
            out["partner"] = random.randint(0, split.ni - 1)
            out["pre2"] = _pre_transform(split, out["partner"], split.load(out["partner"]), args)
            out["r"] = float(np.random.beta(32.0, 32.0))
        if args.hsv_h or args.hsv_s or args.hsv_v:
            out["hsv_u"] = np.random.uniform(-1, 1, 3)
            out["hsv_gain"] = out["hsv_u"] * [args.hsv_h, args.hsv_s, args.hsv_v] + 1
        out["p_flipud"] = random.random()
        out["flipud"] = out["p_flipud"] < args.flipud
        out["p_fliplr"] = random.random()
        out["fliplr"] = out["p_fliplr"] < args.fliplr
    out["p_bgr"] = random.uniform(0, 1)
    out["rgb"] = out["p_bgr"] > (args.bgr if mode == "train" else 0.0)
    return out


def hsv_luts(gain):
    """The three tables of RandomHSV (augment.py:617-620) for gains r (3,) float64 -> (3, 256) uint8"""
    import numpy as np
    r = np.asarray(gain, np.float64)
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def image_records(samples, slot):
    """sample_augment's records -> (rec_i (B, 112) int32, rec_f (B, 16) float64, lut (B, 3, 256) uint8) of y3d_yolo2d_image_aug;
    slot: frame index -> position in the pointer table"""
    import numpy as np
    B = len(samples)
    ri, rf, lut = np.zeros((B, _REC_I), np.int32), np.zeros((B, _REC_F), np.float64), np.zeros((B, 3, 256), np.uint8)
    for b, s in enumerate(samples):
        for l, pre in enumerate((s["pre"], s["pre2"])):
            if pre is None:
                continue
            o = l * _LAYER
            ri[b, o], ri[b, o + 1] = len(pre["tiles"]), pre["canvas"]
            for k, t in enumerate(pre["tiles"]):
                ri[b, o + 2 + k * _TILE:o + 2 + k * _TILE + 11] = (slot[t["frame"]], t["h0"], t["w0"], t["h"], t["w"], t["x1a"], t["y1a"],
                                                                   t["x2a"], t["y2a"], t["padw"], t["padh"])
            rf[b, l * 6:l * 6 + 6] = pre["M_inv"]
        hsv = s["hsv_gain"] is not None
        ri[b, 100:105] = (int(s["flipud"]), int(s["fliplr"]), int(not s["rgb"]), int(hsv), int(s["pre2"] is not None))
        rf[b, 12] = s["r"]
        if hsv:
            lut[b] = hsv_luts(s["hsv_gain"])
    return ri, rf, lut


def label_records(split, samples, rec_start):
    """sample_augment's records -> (lab_i (B, 20) int32, lab_f (B, 48) float32) of y3d_yolo2d_encode_labels; rec_start[frame] = first
    row of the frame's labels in the uploaded label table"""
    import numpy as np
    B = len(samples)
    li, lf = np.zeros((B, _LAB_I), np.int32), np.zeros((B, _LAB_F), np.float32)
    for b, s in enumerate(samples):
        for l, pre in enumerate((s["pre"], s["pre2"])):
            if pre is None:
                continue
            for k, t in enumerate(pre["tiles"]):
                q = l * 4 + k
                li[b, 2 * q], li[b, 2 * q + 1] = rec_start[t["frame"]], len(split.labels[t["frame"]])
                lf[b, 4 * q:4 * q + 4] = (t["w"], t["h"], t["lab_padw"], t["lab_padh"])
            li[b, 16 + l] = 1 | (2 if pre["mosaic"] else 0) | (4 if pre["warp"] else 0)
            lf[b, 32 + l * 8:32 + l * 8 + 6] = np.asarray(pre["M"], np.float32)[:2].reshape(6)
            lf[b, 32 + l * 8 + 6] = pre["scale"]
        li[b, 18] = int(s["flipud"]) | (int(s["fliplr"]) << 1)
    return li, lf


def pack_images(imgs, rec_i, rec_f, lut, imgsz, device):
    """Host side of augment_images: the decoded (H, W, 3) uint8 device images of the pointer table and the three record arrays ->
    dict of device tensors (one upload each)"""
    if torch.device(device).type != "cuda":
        raise Y3DError("pack_images: the images are built on a HIP device (no host fallback)")
    if not imgs or any((not t.is_cuda) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 for t in imgs):
        raise Y3DError("pack_images: images must be (H, W, 3) uint8 tensors on a HIP device")
    imgs = [t.contiguous() for t in imgs]
    B = rec_i.shape[0]
    if rec_i.shape != (B, _REC_I) or rec_f.shape != (B, _REC_F) or lut.shape != (B, 3, 256):
        raise Y3DError("pack_images: record arrays of the wrong shape")
    for b in range(B):  # every tile must name an image of the table, with that image's size
        for l in range(2):
            for k in range(int(rec_i[b, l * _LAYER])):
                t = rec_i[b, l * _LAYER + 2 + k * _TILE:l * _LAYER + 2 + (k + 1) * _TILE]
                if not 0 <= t[0] < len(imgs) or tuple(imgs[t[0]].shape[:2]) != (int(t[1]), int(t[2])):
                    raise Y3DError("pack_images: a tile record does not match its image")
    src = torch.tensor([t.data_ptr() for t in imgs], dtype=torch.int64).to(device)
    return {"imgs": imgs, "src": src, "rec_i": _up(rec_i, device), "rec_f": _up(rec_f, device), "lut": _up(lut, device), "imgsz": int(imgsz)}


def augment_images(packed, mode="uint8"):
    """The image work of B samples, one HIP launch, no host synchronisation (capturable): allocates the output and launches.
    mode "uint8": (B, S, S, 3) uint8 for the stem (`y3d_stem_im2col_u8` divides by 255); "float": (B, 3, S, S) float32 in [0, 1]."""
    ri = packed["rec_i"]
    if not ri.is_cuda:
        raise Y3DError("augment_images: the packed records must live on a HIP device (no host fallback)")
    B, S, dev = ri.shape[0], packed["imgsz"], ri.device
    if mode == "float":
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    elif mode == "uint8":
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    else:
        raise ValueError("mode must be 'float' or 'uint8'")
    lib().yolo2d_image_aug(packed["src"].data_ptr(), packed["src"].shape[0], ri.data_ptr(), packed["rec_f"].data_ptr(), packed["lut"].data_ptr(),
                           B, S, 0 if mode == "float" else 1, out.data_ptr(), ops.stream())
    return out


def _label_table(label_rows, seg, lab_i, lab_f, device, whose):
    """What both label packers end with: the (n, 5) float32 label table (one dummy row when it is empty) and the two record arrays go
    to the device.  seg: (m, 2) int [first row, rows], every run of label rows the records name; all must lie inside the table."""
    import numpy as np
    rows = np.asarray(label_rows, np.float32).reshape(-1, 5)
    n = len(rows)
    if (seg < 0).any() or (seg.sum(1)[seg[:, 1] > 0] > n).any():
        raise Y3DError(f"{whose} label rows lie outside the label table")
    return {"rec": _up(rows if n else np.zeros((1, 5), np.float32), device), "n_rec": n, "lab_i": _up(lab_i, device), "lab_f": _up(lab_f, device)}


def _static_labels(packed, max_boxes, what):
    """The unwritten static layout both label encoders fill, for packed labels that live on the device -> (cap, dict)"""
    cap = _loss.check_max_boxes(max_boxes) or BASE_CAP
    li = packed["lab_i"]
    if not li.is_cuda or not packed["rec"].is_cuda or not packed["lab_f"].is_cuda:
        raise Y3DError(f"{what}: the packed labels must live on a HIP device (no host fallback)")
    B, dev = li.shape[0], li.device
    return cap, {"cls": torch.empty(B * cap, 1, dtype=torch.float32, device=dev), "bboxes": torch.empty(B * cap, 4, dtype=torch.float32, device=dev),
                 "batch_idx": torch.empty(B * cap, dtype=torch.float32, device=dev), "counts": torch.empty(B, dtype=torch.int32, device=dev)}


def pack_labels(label_rows, lab_i, lab_f, device):
    """Host side of encode_labels: the (n, 5) float32 label table and the two record arrays -> dict of device tensors"""
    if torch.device(device).type != "cuda":
        raise Y3DError("pack_labels: the label encoder runs on a HIP device (no host fallback)")
    if lab_i.shape[1:] != (_LAB_I,) or lab_f.shape != (lab_i.shape[0], _LAB_F):
        raise Y3DError("pack_labels: record arrays of the wrong shape")
    return _label_table(label_rows, lab_i[:, :16].reshape(-1, 2), lab_i, lab_f, device, "pack_labels: a tile's")


def encode_labels(packed, imgsz, max_boxes=None):
    """The label work of B samples + `collate_fn`, one HIP launch, no host synchronisation (capturable).  -> static layout of
    cap = max_boxes or 64 rows per image: `cls` (B*cap, 1) float32, `bboxes` (B*cap, 4) float32 xywh normalised, `batch_idx` (B*cap)
    float32 (-1 on unused rows, which are zeros and which `y3d_pad_targets` skips), `counts` (B,) int32: the true number of boxes of
    each image — one with more than cap keeps its first cap in the reference's order and shows the surplus here."""
    cap, o = _static_labels(packed, max_boxes, "encode_labels")
    li = packed["lab_i"]
    lib().yolo2d_encode_labels(packed["rec"].data_ptr(), int(packed["n_rec"]), li.data_ptr(), packed["lab_f"].data_ptr(), li.shape[0], int(imgsz), cap,
                               o["cls"].data_ptr(), o["bboxes"].data_ptr(), o["batch_idx"].data_ptr(), o["counts"].data_ptr(), ops.stream())
    return o


def compact_labels(static, counts, max_boxes=None):
    """Static layout -> the ragged tensors `collate_fn` returns, in its dtypes: cls (N, 1) float32, bboxes (N, 4) float32, batch_idx
    (N,) float32; an image contributes min(count, cap) rows.  A batch without a single box gives cls of shape (0,), as torch.cat of
    Format's empty tensors does.  counts: host ints (B,)."""
    cap = _loss.check_max_boxes(max_boxes) or BASE_CAP
    dev = static["cls"].device
    rows = torch.cat([torch.arange(b * cap, b * cap + min(int(c), cap)) for b, c in enumerate(counts)]).to(dev)
    out = {k: static[k].index_select(0, rows) for k in ("cls", "bboxes", "batch_idx")}
    if rows.numel() == 0:
        out["cls"] = out["cls"].reshape(0)
    return out


def build_batch(split, indices, args, device, mode="train", max_boxes=None, compact=False, img_mode="uint8"):
    """`collate_fn([dataset[i] for i in indices])` of the reference's YOLODataset (task detect) over `split`, with the image and label
    work on the device.  -> {"img", "cls", "bboxes", "batch_idx", "counts", "im_file", "ori_shape", "resized_shape"}; the per-box keys in
    encode_labels' static layout, or with compact=True (one read-back of the counts) in collate_fn's ragged shapes.  img_mode
    "uint8": (B, S, S, 3) uint8 in Format's channel order for the stem; "float": (B, 3, S, S) float32 in [0, 1].
    A `RectSplit` (mode "val" only) gives the validator's rectangular batch instead: see `_build_rect_batch`.  A `DeviceSplit` or a
    `DeviceRectSplit` builds the same batch from its resident frames (their `build_batch`), on the device it lives on."""
    if torch.device(device).type != "cuda":
        raise Y3DError("build_batch: the batch is built on a HIP device (no host fallback)")
    if img_mode not in ("uint8", "float"):
        raise ValueError("img_mode must be 'uint8' or 'float'")
    _loss.check_max_boxes(max_boxes)
    if isinstance(split, (DeviceSplit, DeviceRectSplit)):
        split.check_device(device)
        return split.build_batch(indices, args, mode=mode, max_boxes=max_boxes, compact=compact, img_mode=img_mode)
    if isinstance(split, RectSplit):
        return _build_rect_batch(split, indices, args, device, mode, max_boxes, compact, img_mode)
    return _build_square_batch(split, indices, args, device, mode, max_boxes, compact, img_mode)


def _frame_tables(split, frames, device):
    """The frames a host-built batch reads, sorted -> (slot: frame -> position in the pointer table, the decoded images in that order,
    rec_start: frame -> first row of its labels in the batch's label table, that table)"""
    import numpy as np
    slot = {f: n for n, f in enumerate(frames)}
    imgs = [split.decode(f, device) for f in frames]
    rec_start, row = {}, 0
    for f in frames:
        rec_start[f] = row
        row += len(split.labels[f])
    return slot, imgs, rec_start, np.concatenate([split.labels[f] for f in frames]) if frames else None  # (no frames: the packers refuse)


def _batch(img, lab, im_files, ori_shapes, shape, ratio_pad, max_boxes, compact):
    """The dictionary every 2D builder returns: the images, the label encoder's `lab`, and per image its file, its original (h, w), the
    `shape` it was resized into and (rect batches, else None) its ratio_pad.  compact: the per-box keys ragged, not in the static layout."""
    batch = {"img": img, "im_file": im_files, "ori_shape": ori_shapes, "resized_shape": [shape for _ in im_files]}
    if ratio_pad is not None:
        batch["ratio_pad"] = ratio_pad
    batch["counts"] = lab["counts"]
    batch.update(compact_labels(lab, lab["counts"].tolist(), max_boxes) if compact else {k: lab[k] for k in ("cls", "bboxes", "batch_idx")})
    return batch


def _build_square_batch(split, indices, args, device, mode, max_boxes, compact, img_mode):
    """build_batch over a `Split`, through `split.decode`: the host builds the five record arrays, the pointer table and the label table
    of the batch's own frames and uploads them.  (Over a `DeviceSplit` it opens no file either: `decode` is a view of the arena.)"""
    samples = [sample_augment(split, i, args, mode) for i in indices]
    frames = sorted({t["frame"] for x in samples for pre in (x["pre"], x["pre2"]) if pre is not None for t in pre["tiles"]})
    slot, imgs, rec_start, rows = _frame_tables(split, frames, device)
    ri, rf, lut = image_records(samples, slot)
    img = augment_images(pack_images(imgs, ri, rf, lut, split.imgsz, device), img_mode)
    li, lf = label_records(split, samples, rec_start)
    lab = encode_labels(pack_labels(rows, li, lf, device), split.imgsz, max_boxes)
    return _batch(img, lab, [split.im_files[x["index"]] for x in samples], [split.size(x["index"]) for x in samples],
                  (split.imgsz, split.imgsz), None, max_boxes, compact)


# ------------------------------------------------------------------------------------------------------------------------------
# Rectangular batches (the validator's dataset) and the letter-box both they and predict.Predictor go through
# ------------------------------------------------------------------------------------------------------------------------------
def letterbox_params(shape, new_shape, auto=False, scaleup=True, stride=32):
    """`LetterBox(new_shape, auto, scaleup=scaleup, stride=stride)` (data/augment.py:696-732, center=True, no scaleFill) on an image of
    `shape` (h, w), without the pixels: Python's round (half to even) wherever the reference rounds.  -> dict: r, new_unpad (w, h) as
    the reference holds it, dw, dh (halved: the label pads), top, bottom, left, right, canvas (H, W)."""
    h, w = int(shape[0]), int(shape[1])
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    H, W = int(new_shape[0]), int(new_shape[1])
    r = min(H / h, W / w)
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(w * r)), int(round(h * r))
    dw, dh = W - new_unpad[0], H - new_unpad[1]
    if auto:
        dw, dh = dw % int(stride), dh % int(stride)  # np.mod of two ints
    dw, dh = dw / 2, dh / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return dict(r=r, new_unpad=new_unpad, dw=dw, dh=dh, top=top, bottom=bottom, left=left, right=right,
                canvas=(new_unpad[1] + top + bottom, new_unpad[0] + left + right))


class RectSplit(Split):
    """The validator's dataset: a `Split` without augmentation whose images are sorted by aspect ratio and grouped into batches that
    each get their own stride-multiple shape — `set_rectangle` (data/base.py:226-249) replayed on the sizes `Split.size` reports.
    `batch_shapes[k]` is the (H, W) canvas of rect batch k; `batch_of(i)` the batch of (reordered) index i; `batches()` the index lists in
    loader order, which is what `build_batch` takes one at a time."""

    def __init__(self, img_dir_or_list, imgsz=640, batch=16, stride=32, pad=0.5):
        import numpy as np
        super().__init__(img_dir_or_list, imgsz, batch, augment=False)
        self.stride, self.pad = int(stride), pad
        if self.stride < 1 or self.stride % 4:
            raise Y3DError(f"yolo2d: rect stride {stride}: the canvas width must be a multiple of 4")
        bi = np.floor(np.arange(self.ni) / self.batch).astype(int)
        nb = bi[-1] + 1
        s = np.array([self.size(i) for i in range(self.ni)])  # hw
        ar = s[:, 0] / s[:, 1]
        irect = ar.argsort()
        self.irect = irect
        self.im_files = [self.im_files[i] for i in irect]
        self.label_files = [self.label_files[i] for i in irect]
        self.labels = [self.labels[i] for i in irect]
        self._hw0 = {n: (int(s[i, 0]), int(s[i, 1])) for n, i in enumerate(irect)}
        ar = ar[irect]
        shapes = [[1, 1]] * nb
        for i in range(nb):
            ari = ar[bi == i]
            mini, maxi = ari.min(), ari.max()
            if maxi < 1:
                shapes[i] = [maxi, 1]
            elif mini > 1:
                shapes[i] = [1, 1 / mini]
        self.batch_shapes = np.ceil(np.array(shapes) * self.imgsz / self.stride + self.pad).astype(int) * self.stride
        self.batch_index = bi

    def batch_of(self, index):
        index = int(index)
        if not 0 <= index < self.ni:
            raise IndexError(f"yolo2d: index {index} of {self.ni} images")
        return int(self.batch_index[index])

    def batches(self):
        return [[int(i) for i in range(k * self.batch, min((k + 1) * self.batch, self.ni))] for k in range(int(self.batch_index[-1]) + 1)]


def rect_sample(split, index):
    """`dataset[index]` of the rect=True validation dataset without pixels and labels: `get_image_and_label` (data/base.py:255-266) +
    LetterBox(new_shape, scaleup=False) on `rect_shape` + Format's bgr draw (one `random.uniform`, as the square `val` path).
    -> dict: index, batch, h0, w0, h, w (after load_image's resize), canvas (H, W), top, left, dw, dh, ratio_pad, p_bgr, rgb."""
    index = int(index)
    k = split.batch_of(index)
    (h0, w0), (h, w) = split.load(index)
    H, W = (int(v) for v in split.batch_shapes[k])
    lb = letterbox_params((h, w), (H, W), auto=False, scaleup=False)
    if lb["r"] != 1.0 or lb["new_unpad"] != (w, h):
        raise Y3DError(f"yolo2d: rect letter-box ratio {lb['r']} after load_image's resize (expected 1)")
    p_bgr = random.uniform(0, 1)
    return dict(index=index, batch=k, h0=h0, w0=w0, h=h, w=w, canvas=(H, W), top=lb["top"], left=lb["left"], dw=lb["dw"], dh=lb["dh"],
                ratio_pad=((h / h0, w / w0), (lb["left"], lb["top"])), p_bgr=p_bgr, rgb=p_bgr > 0.0)


def pack_letterbox(imgs, rec, H, W, device):
    """Host side of letterbox_images: the decoded (h0, w0, 3) uint8 device images of the pointer table and the (B, 8) int32 records
    [src, h0, w0, new_h, new_w, top, left, swap_rb] for an (H, W) canvas -> dict of device tensors.  Every record must name an image of
    the table with that image's size, and place its resized image inside the canvas."""
    import numpy as np
    if torch.device(device).type != "cuda":
        raise Y3DError("pack_letterbox: the images are built on a HIP device (no host fallback)")
    H, W = int(H), int(W)
    if H < 1 or W < 4 or W % 4:
        raise Y3DError(f"pack_letterbox: canvas {H} x {W}: the width must be a multiple of 4")
    if not imgs or any((not torch.is_tensor(t)) or (not t.is_cuda) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 for t in imgs):
        raise Y3DError("pack_letterbox: images must be (H, W, 3) uint8 tensors on a HIP device")
    imgs = [t.contiguous() for t in imgs]
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    if rec.ndim != 2 or rec.shape[1] != _LB_REC or not len(rec):
        raise Y3DError("pack_letterbox: records of the wrong shape")
    for r in rec:
        if not 0 <= r[0] < len(imgs) or tuple(imgs[r[0]].shape[:2]) != (int(r[1]), int(r[2])) or min(r[1:5]) < 1:
            raise Y3DError("pack_letterbox: a record does not match its image")
        if r[5] < 0 or r[6] < 0 or r[5] + r[3] > H or r[6] + r[4] > W:
            raise Y3DError("pack_letterbox: a record places its image outside the canvas")
    src = torch.tensor([t.data_ptr() for t in imgs], dtype=torch.int64).to(device)
    return {"imgs": imgs, "src": src, "rec": _up(rec, device), "H": H, "W": W}


def letterbox_images(packed, mode="uint8"):
    """B images letter-boxed into one (H, W) canvas, one HIP launch, no host synchronisation (capturable): allocates the output and
    launches.  mode "uint8": (B, H, W, 3) uint8 for the stem; "float": (B, 3, H, W) float32 in [0, 1]."""
    rec = packed["rec"]
    if not rec.is_cuda:
        raise Y3DError("letterbox_images: the packed records must live on a HIP device (no host fallback)")
    B, H, W, dev = rec.shape[0], packed["H"], packed["W"], rec.device
    if W % 4:
        raise Y3DError(f"letterbox_images: canvas width {W} must be a multiple of 4")
    if mode == "float":
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    elif mode == "uint8":
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    else:
        raise ValueError("mode must be 'float' or 'uint8'")
    lib().letterbox_image(packed["src"].data_ptr(), packed["src"].shape[0], rec.data_ptr(), B, H, W, 0 if mode == "float" else 1,
                          out.data_ptr(), ops.stream())
    return out


def pack_letterbox_labels(label_rows, lab_i, lab_f, device):
    """Host side of letterbox_labels: the (n, 5) float32 label table, lab_i (B, 2) int32 [first row, rows] and lab_f (B, 4) float32
    [w, h, padw, padh] -> dict of device tensors"""
    import numpy as np
    if torch.device(device).type != "cuda":
        raise Y3DError("pack_letterbox_labels: the label encoder runs on a HIP device (no host fallback)")
    lab_i, lab_f = np.ascontiguousarray(lab_i, dtype=np.int32), np.ascontiguousarray(lab_f, dtype=np.float32)
    if lab_i.ndim != 2 or lab_i.shape[1] != 2 or lab_f.shape != (lab_i.shape[0], 4) or not len(lab_i):
        raise Y3DError("pack_letterbox_labels: record arrays of the wrong shape")
    return _label_table(label_rows, lab_i, lab_i, lab_f, device, "pack_letterbox_labels: an image's")


def letterbox_labels(packed, H, W, max_boxes=None):
    """The validation label chain of B samples + `collate_fn`, one HIP launch, no host synchronisation (capturable), in encode_labels'
    static layout of cap = max_boxes or 64 rows per image; normalised by the (H, W) canvas."""
    cap, o = _static_labels(packed, max_boxes, "letterbox_labels")
    li = packed["lab_i"]
    lib().letterbox_labels(packed["rec"].data_ptr(), int(packed["n_rec"]), li.data_ptr(), packed["lab_f"].data_ptr(), li.shape[0], int(H), int(W), cap,
                           o["cls"].data_ptr(), o["bboxes"].data_ptr(), o["batch_idx"].data_ptr(), o["counts"].data_ptr(), ops.stream())
    return o


def rect_records(split, samples, slot, rec_start):
    """rect_sample's records -> (rec (B, 8) int32 of y3d_letterbox_image, lab_i (B, 2) int32, lab_f (B, 4) float32 of
    y3d_letterbox_labels); slot: index -> position in the pointer table, rec_start: index -> first row in the label table"""
    import numpy as np
    B = len(samples)
    rec, li, lf = np.zeros((B, _LB_REC), np.int32), np.zeros((B, 2), np.int32), np.zeros((B, 4), np.float32)
    for b, s in enumerate(samples):
        rec[b] = (slot[s["index"]], s["h0"], s["w0"], s["h"], s["w"], s["top"], s["left"], int(not s["rgb"]))
        li[b] = (rec_start[s["index"]], len(split.labels[s["index"]]))
        lf[b] = (s["w"], s["h"], s["dw"], s["dh"])
    return rec, li, lf


def _rect_indices(split, indices, args, mode):
    """What every rect builder checks first -> the indices as ints: a validation batch, not empty, all of one rect batch"""
    _check_args(args)
    if mode != "val":
        raise Y3DError(f"yolo2d: a RectSplit builds validation batches only (mode {mode!r}); rect training batches are not supported")
    indices = [int(i) for i in indices]
    if not indices:
        raise Y3DError("yolo2d: an empty rect batch")
    ks = {split.batch_of(i) for i in indices}
    if len(ks) != 1:
        raise Y3DError(f"yolo2d: indices of rect batches {sorted(ks)}: a rect batch has one shape, build them one at a time")
    return indices


def _build_rect_batch(split, indices, args, device, mode, max_boxes, compact, img_mode):
    """`collate_fn([dataset[i] for i in indices])` of the validator's rect=True YOLODataset: all indices of one rect batch, letter-boxed
    (ratio 1 after load_image's resize) into that batch's (H, W) canvas.  -> the keys of the square path, `resized_shape` = (H, W) per
    image, and `ratio_pad` = ((h / h0, w / w0), (left, top)) per image as `BoxStats.update_2d` reads it.  img_mode "uint8":
    (B, H, W, 3) uint8; "float": (B, 3, H, W) float32."""
    indices = _rect_indices(split, indices, args, mode)
    samples = [rect_sample(split, i) for i in indices]
    H, W = samples[0]["canvas"]
    slot, imgs, rec_start, rows = _frame_tables(split, sorted(set(indices)), device)
    rec, li, lf = rect_records(split, samples, slot, rec_start)
    img = letterbox_images(pack_letterbox(imgs, rec, H, W, device), img_mode)
    lab = letterbox_labels(pack_letterbox_labels(rows, li, lf, device), H, W, max_boxes)
    return _batch(img, lab, [split.im_files[i] for i in indices], [(s["h0"], s["w0"]) for s in samples], (H, W),
                  [s["ratio_pad"] for s in samples], max_boxes, compact)


# ------------------------------------------------------------------------------------------------------------------------------
# the split resident on the device: decoded once, then a batch is the draws, one small upload and three launches
# ------------------------------------------------------------------------------------------------------------------------------
_DRAW_W, _DRAW_LAYER, _DRAW_TAIL = 56, 23, 46  # Y3D_YOLO2D_DRAW_W (include/y3d.h): two layers of 23, then the sample's own nine values
PLAN_TABLES = (("rec_i", torch.int32, (_REC_I,)), ("rec_f", torch.float64, (_REC_F,)), ("lut", torch.uint8, (3, 256)),
               ("lab_i", torch.int32, (_LAB_I,)), ("lab_f", torch.float32, (_LAB_F,)))


def draw_table(samples):
    """sample_augment's records -> the (B, 56) float64 draw table of `y3d_yolo2d_plan_batch`.  Per layer (the sample at 0, its MixUp
    partner at 23): [present, mosaic, warp, the frame positions of tiles 0..3 (-1: no such tile), yc, xc, canvas, M[:2] (6), M_inv (6),
    scale]; then at 46: mix, r, hsv, the three gains, flipud, fliplr, bgr, 0.  Every value is carried exactly (M is float32)."""
    import numpy as np
    d = np.zeros((len(samples), _DRAW_W), np.float64)
    for b, s in enumerate(samples):
        for l, pre in enumerate((s["pre"], s["pre2"])):
            if pre is None:
                continue
            o = l * _DRAW_LAYER
            frames = [t["frame"] for t in pre["tiles"]]
            d[b, o:o + 3] = (1, pre["mosaic"], pre["warp"])
            d[b, o + 3:o + 7] = frames + [-1] * (4 - len(frames))
            d[b, o + 7:o + 10] = (pre["yc"], pre["xc"], pre["canvas"])
            d[b, o + 10:o + 16] = np.asarray(pre["M"], np.float32)[:2].reshape(6)
            d[b, o + 16:o + 22] = pre["M_inv"]
            d[b, o + 22] = pre["scale"]
        hsv = s["hsv_gain"] is not None
        d[b, _DRAW_TAIL:_DRAW_TAIL + 3] = (s["pre2"] is not None, s["r"], hsv)
        if hsv:
            d[b, _DRAW_TAIL + 3:_DRAW_TAIL + 6] = s["hsv_gain"]
        d[b, _DRAW_TAIL + 6:_DRAW_TAIL + 9] = (s["flipud"], s["fliplr"], not s["rgb"])
    return d


def plan_batch(split, draws, draws_dev=None, out=None):
    """The five record arrays of `y3d_yolo2d_image_aug` and `y3d_yolo2d_encode_labels` for a draw table over a DeviceSplit, one HIP launch
    (`y3d_yolo2d_plan_batch`), no allocation when `out` is given and no synchronisation (capturable).  draws: (B, 56) float64 on the host
    (numpy or tensor), rows as `draw_table` writes them; draws_dev: the same table on the device (uploaded here when None).  Frame
    positions outside the split are refused from the host table.  out: optionally the five output tensors (at least B rows each; the
    first B are written).  -> dict rec_i (B, 112) int32 with source index = dataset position, rec_f (B, 16) float64, lut (B, 3, 256)
    uint8, lab_i (B, 20) int32 with rows counted in `split.rec`, lab_f (B, 48) float32."""
    host, draws_dev, out = check_plan(draws, _DRAW_W, split.device, PLAN_TABLES, draws_dev, out)
    lib().yolo2d_plan_batch(split.frame_hw.data_ptr(), split.rec_span.data_ptr(), len(split), split.imgsz, host.data_ptr(), draws_dev.data_ptr(),
                            host.shape[0], *[out[k].data_ptr() for k, _, _ in PLAN_TABLES], ops.stream())
    return out


def _decode_rgb(path):
    """`Split.decode`'s arithmetic on the host: (h0, w0, 3) uint8 RGB, the EXIF orientation applied"""
    import numpy as np
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        return np.array(ImageOps.exif_transpose(im).convert("RGB"))


class _Resident(ResidentSplit):
    """What DeviceSplit and DeviceRectSplit share: the frames of a `Split` decoded once into one uint8 device arena, and the frame tables
    indexed by dataset position (the position in `im_files`): `arena`; `img_off` (N) int64; `frame_hw` (N, 2) int32 (h0, w0); `src` (N)
    int64 device pointers arena + offset, the pointer table both image kernels take with n_src = N; `rec` (R, 5) float32, all label rows
    in file order (one dummy row when there is none; `n_rec` = R); `rec_span` (N, 2) int32 (first row, rows)."""

    def _refusals(self, device, workers):
        """what is refused before any file is read -> the torch.device"""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise Y3DError(f"{type(self).__name__}: the split is held on a HIP device, not {dev} (no host fallback)")
        if int(workers) < 1:
            raise Y3DError(f"{type(self).__name__}: workers = {workers}")
        return dev

    def _load(self, dev, max_bytes, workers):
        import numpy as np
        # sizes from the file headers (Split.size's EXIF rule), the budget before anything is decoded or allocated
        self._layout(dev, [self.size(i) for i in range(self.ni)], max_bytes)
        n_rows = [len(r) for r in self.labels]
        self.n_rec, self.span_host = int(sum(n_rows)), span_table(n_rows)
        rec = np.concatenate(self.labels).astype(np.float32).reshape(-1, 5) if self.n_rec else np.zeros((1, 5), np.float32)
        self.rec = _up(rec, self.device, torch.float32)
        self._fill(self.span_host, lambda pos: _decode_rgb(self.im_files[pos]), lambda pos: self.im_files[pos], workers, _DRAW_W)
        self.src = _up(self.arena.data_ptr() + self.offsets, self.device, torch.int64)

    def decode(self, i, device):
        """`Split.decode` without the file: the arena view of frame i"""
        self.check_device(device)
        return self.frame(int(i))


class DeviceSplit(_Resident, Split):
    """A `Split` decoded once and held on the device (the reference's `YOLODataset(cache="ram")`, one step further): the files are listed
    and the labels read as `Split` does, the sizes come from the file headers, the bytes needed are checked against `max_bytes` (default:
    half of the device's free memory) before anything is decoded, then every frame is decoded with `min(workers, 16)` threads into one
    uint8 arena (each frame (h0, w0, 3) RGB at a multiple of 16 bytes, uploaded in large pinned chunks) next to the frame tables of
    `_Resident`.  Originals only: the image kernel samples the original frame.

    `build_batch` then returns what `build_batch(Split(...), ...)` returns, bit for bit, without touching a file: `sample_augment` per
    index (the same draws, the same buffer), one non-blocking upload of the draw table from a ring of pinned buffers and three launches
    (`plan_batch`, the image augmentation over the split's pointer table, the label encoder over the split's label rows).  `decode` is a
    view of the arena, so the host-built path (`_build_square_batch`) runs on a DeviceSplit as well, and opens no file either."""

    def __init__(self, img_dir_or_list, imgsz=640, batch=16, augment=True, device="cuda", max_bytes=None, workers=8):
        dev = self._refusals(device, workers)
        Split.__init__(self, img_dir_or_list, imgsz, batch, augment)
        self._load(dev, max_bytes, workers)

    def build_batch(self, indices, args, mode="train", max_boxes=None, compact=False, img_mode="uint8"):
        """`build_batch(split, indices, args, device, ...)` from the resident split: the same dictionary, bit for bit.  With compact=False
        nothing here waits for the device (but a ring buffer still in flight) and no file is opened."""
        if img_mode not in ("uint8", "float"):
            raise ValueError("img_mode must be 'uint8' or 'float'")
        _loss.check_max_boxes(max_boxes)
        samples = [sample_augment(self, i, args, mode) for i in indices]
        if not samples:
            raise Y3DError("build_batch: an empty batch")
        s = self.imgsz
        with torch.cuda.device(self.device):
            host, dev = self._ring.upload(draw_table(samples))
            plan = plan_batch(self, host, dev)
            img = augment_images({"src": self.src, "rec_i": plan["rec_i"], "rec_f": plan["rec_f"], "lut": plan["lut"], "imgsz": s}, img_mode)
            lab = encode_labels({"rec": self.rec, "n_rec": self.n_rec, "lab_i": plan["lab_i"], "lab_f": plan["lab_f"]}, s, max_boxes)
        return _batch(img, lab, [self.im_files[x["index"]] for x in samples], [self.size(x["index"]) for x in samples], (s, s), None,
                      max_boxes, compact)


class DeviceRectSplit(_Resident, RectSplit):
    """A `RectSplit` held on the device: the arena and frame tables of `_Resident`, indexed by the split's (aspect-ratio sorted) positions.
    A rect split has no randomness but Format's bgr draw, so the records of every batch are computed once at load with the host
    functions of the path-based builder (`rect_sample`, `rect_records`), with source index = position and label rows counted in `rec`,
    and uploaded once: `lb_rec` (N, 8) int32, `lb_lab_i` (N, 2) int32, `lb_lab_f` (N, 4) float32.  `build_batch` over a run of
    consecutive positions of one rect batch (what `batches()` lists) is then two launches over slices of those tables: no upload, no
    file.  Any other index list of one rect batch goes through the host-built path over the arena (`_build_rect_batch`)."""

    def __init__(self, img_dir_or_list, imgsz=640, batch=16, stride=32, pad=0.5, device="cuda", max_bytes=None, workers=8):
        dev = self._refusals(device, workers)
        RectSplit.__init__(self, img_dir_or_list, imgsz, batch, stride, pad)
        self._load(dev, max_bytes, workers)
        state = random.getstate()  # rect_sample draws Format's bgr number; the load leaves the generator as it found it
        try:
            self._samples = [rect_sample(self, i) for i in range(self.ni)]
        finally:
            random.setstate(state)
        same = {i: i for i in range(self.ni)}
        rec, li, lf = rect_records(self, self._samples, same, {i: int(self.span_host[i, 0]) for i in range(self.ni)})
        rec[:, 7] = 0  # a draw that asks for BGR (p_bgr == 0.0) is served by the host-built path
        for r, s in zip(rec, self._samples):
            H, W = s["canvas"]
            if min(r[1:5]) < 1 or r[5] < 0 or r[6] < 0 or r[5] + r[3] > H or r[6] + r[4] > W or W % 4:
                raise Y3DError(f"DeviceRectSplit: {self.im_files[s['index']]} does not fit its {H} x {W} canvas")
        self.lb_rec, self.lb_lab_i, self.lb_lab_f = _up(rec, self.device), _up(li, self.device), _up(lf, self.device)

    def build_batch(self, indices, args, mode="val", max_boxes=None, compact=False, img_mode="uint8"):
        """`build_batch(rect_split, indices, args, device, mode="val", ...)` from the resident split: the same dictionary, bit for bit"""
        if img_mode not in ("uint8", "float"):
            raise ValueError("img_mode must be 'uint8' or 'float'")
        _loss.check_max_boxes(max_boxes)
        indices = _rect_indices(self, indices, args, mode)
        a, b = indices[0], indices[0] + len(indices)
        state = random.getstate()
        rgb = [random.uniform(0, 1) > 0.0 for _ in indices]  # Format's bgr draw of every sample, as rect_sample draws it
        if indices != list(range(a, b)) or not all(rgb):
            random.setstate(state)
            return _build_rect_batch(self, indices, args, self.device, mode, max_boxes, compact, img_mode)
        samples = self._samples[a:b]
        H, W = samples[0]["canvas"]
        with torch.cuda.device(self.device):
            img = letterbox_images({"src": self.src, "rec": self.lb_rec[a:b], "H": H, "W": W}, img_mode)
            lab = letterbox_labels({"rec": self.rec, "n_rec": self.n_rec, "lab_i": self.lb_lab_i[a:b], "lab_f": self.lb_lab_f[a:b]}, H, W, max_boxes)
        return _batch(img, lab, [self.im_files[i] for i in indices], [(s["h0"], s["w0"]) for s in samples], (H, W),
                      [s["ratio_pad"] for s in samples], max_boxes, compact)
