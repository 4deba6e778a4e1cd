"""Mints tests/golden/yolo2d_rect.npz from the REFERENCE's rect=True validation dataset and its predictor arithmetic, run on the CPU.

    python tools/make_golden_rect.py      # needs the reference checkout (oracle.ref_shim.import_reference)

Rect sets.  The dataset is a `YOLODataset` created without `__init__` (tools/make_golden_yolo2d.py explains why) over the twelve frames
of tests/yolo2d_tree.py with the label text of tests/golden/yolo2d_labels.npz, `rect=True`, `augment=False`, imgsz = 64, stride = 32,
pad = 0.5.  `set_rectangle`, `get_image_and_label`, `LetterBox` (with `rect_shape`), `Format` and `collate_fn` are the reference's own.
Two sets: batch = 4 (canvases 64 x 96, 96 x 96, 96 x 64: the three branches of `set_rectangle`, three frames tied at aspect ratio 1)
and batch = 5 (a ragged last batch of two).  The tool asserts that the three branches and a tie occur.  Recorded per set: `irect`,
`batch_shapes`, the file names in their new order, per sample `ori_shape`, the size after `load_image`, `resized_shape`, `ratio_pad`
with `(left, top)`, and per batch the collated `cls`, `bboxes`, `batch_idx`.

Predict sets.  `LetterBox(64, auto=all shapes equal, stride=32)` on blank images of listed shapes: the size handed to `cv2.resize`
(new_unpad), the four borders handed to `cv2.copyMakeBorder`, the output shape.  Then `ops.scale_boxes(canvas, boxes, ori_shape)`
(+ its `clip_boxes`) on float32 rows that leave the image on each of the four sides; the `gain` and `pad` it computes are read off
through recording stand-ins for the `min` and `round` its module sees.

OpenCV is absent here; `cv2.resize` / `cv2.copyMakeBorder` are SHAPE-only stand-ins, as in tools/make_golden_yolo2d.py: no pixel of the
reference is recorded.  The fixture holds data only: recorded numbers and names.
"""
from __future__ import annotations

import os
import random
import shutil
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402
import yolo2d_tree as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "yolo2d_rect.npz")
IMGSZ, STRIDE, PAD, NC = 64, 32, 0.5, 20
RECT_SETS = {"b4": 4, "b5": 5}
# name -> list of (h, w): equal shapes (auto), a zero pad, mixed shapes with up-scaling, odd pads on either axis, a width that rounds
# half to even (37 * 0.5 = 18.5 -> 18) and 1-pixel-wide / 1-pixel-high images
PREDICT_SETS = {
    "auto": [(48, 100), (48, 100)],
    "auto_zero": [(32, 64)],
    "auto_square": [(64, 64), (64, 64)],
    "auto_up": [(20, 30)],
    "mixed": [(60, 100), (100, 60), (64, 64), (32, 48), (48, 32), (128, 37), (40, 1)],
    "thin": [(7, 1), (1, 7)],
}


def install_cv2(log):
    from PIL import Image
    cv2 = sys.modules["cv2"]
    cv2.imread = lambda f, *a: np.ascontiguousarray(np.array(Image.open(f).convert("RGB"))[..., ::-1])

    def resize(im, dsize, interpolation=None):
        log.append(("resize", tuple(int(v) for v in dsize)))
        return np.zeros((dsize[1], dsize[0], 3), np.uint8)

    def border(img, t, b, l, r, kind, value=None):
        log.append(("border", (int(t), int(b), int(l), int(r))))
        return np.pad(img, ((t, b), (l, r), (0, 0)), constant_values=114)

    cv2.resize, cv2.copyMakeBorder = resize, border
    return cv2


def make_dataset(YOLODataset, split, batch):
    from yolov10_3d_amd import yolo2d
    ds = object.__new__(YOLODataset)
    ds.use_segments = ds.use_keypoints = ds.use_obb = False
    ds.data = {"names": {i: str(i) for i in range(NC)}}
    ds.imgsz, ds.augment, ds.rect, ds.single_cls, ds.prefix = IMGSZ, False, True, False, ""
    ds.im_files = list(split.im_files)
    ds.labels = [dict(im_file=f, shape=split.size(i), cls=lb[:, 0:1].copy(), bboxes=lb[:, 1:].copy(), segments=[], keypoints=None, normalized=True,
                      bbox_format="xywh") for i, (f, lb) in enumerate(zip(split.im_files, split.labels))]
    ds.ni = len(ds.labels)
    ds.batch_size, ds.stride, ds.pad = batch, STRIDE, PAD
    ds.buffer, ds.max_buffer_length = [], 0
    ds.set_rectangle()
    ds.ims, ds.im_hw0, ds.im_hw = [None] * ds.ni, [None] * ds.ni, [None] * ds.ni
    ds.npy_files = [Path(f).with_suffix(".npy") for f in ds.im_files]
    ds.transforms = ds.build_transforms(hyp=SimpleNamespace(**dict(yolo2d.DATA_ARGS, mask_ratio=4, overlap_mask=True)))
    return ds


def rect_set(YOLODataset, img_dir, batch, out, name):
    from yolov10_3d_amd import yolo2d
    split = yolo2d.Split(img_dir, IMGSZ, batch, augment=False)
    s = np.array([split.size(i) for i in range(split.ni)])
    ar = s[:, 0] / s[:, 1]
    ds = make_dataset(YOLODataset, split, batch)
    irect = np.array([split.im_files.index(f) for f in ds.im_files], np.int64)  # set_rectangle keeps its permutation to itself
    assert np.array_equal(ar[irect], np.sort(ar))
    out[f"{name}/batch"] = np.array(batch)
    out[f"{name}/irect"] = irect
    out[f"{name}/batch_shapes"] = np.asarray(ds.batch_shapes, np.int64)
    out[f"{name}/files"] = np.array([os.path.basename(f) for f in ds.im_files])
    ori, hw, res, ratio, lt, bidx_of = [], [], [], [], [], []
    random.seed(7)
    nb = int(ds.batch[-1]) + 1
    for k in range(nb):
        items = [i for i in range(ds.ni) if ds.batch[i] == k]
        samples = [ds[i] for i in items]
        for i, smp in zip(items, samples):
            ori.append(smp["ori_shape"])
            hw.append(ds.load_image(i)[2])
            res.append(tuple(int(v) for v in smp["resized_shape"]))
            ratio.append(smp["ratio_pad"][0])
            lt.append(smp["ratio_pad"][1])
            bidx_of.append(k)
            assert tuple(smp["img"].shape[1:]) == tuple(int(v) for v in ds.batch_shapes[k])
        batch_out = YOLODataset.collate_fn([dict(x) for x in samples])
        for key in ("cls", "bboxes", "batch_idx"):
            out[f"{name}/c{k}/{key}"] = batch_out[key].numpy()
    out[f"{name}/ori_shape"] = np.array(ori, np.int64)
    out[f"{name}/hw"] = np.array(hw, np.int64)
    out[f"{name}/resized_shape"] = np.array(res, np.int64)
    out[f"{name}/ratio"] = np.array(ratio, np.float64)
    out[f"{name}/left_top"] = np.array(lt, np.int64)
    out[f"{name}/batch_of"] = np.array(bidx_of, np.int64)
    return ar[irect], ds


def predict_set(A, ops, log, shapes, out, name, rng):
    import torch
    auto = len(set(shapes)) == 1
    lb = A.LetterBox(IMGSZ, auto=auto, stride=STRIDE)
    unpad, borders, canvases = [], [], []
    for h, w in shapes:
        del log[:]
        im = lb(image=np.zeros((h, w, 3), np.uint8))
        rs = [v for t, v in log if t == "resize"]
        unpad.append(rs[0] if rs else (w, h))
        borders.append([v for t, v in log if t == "border"][0])
        canvases.append(im.shape[:2])
    assert len(set(canvases)) == 1, (name, canvases)
    H, W = canvases[0]
    out[f"{name}/shapes"] = np.array(shapes, np.int64)
    out[f"{name}/auto"] = np.array(auto)
    out[f"{name}/canvas"] = np.array([H, W], np.int64)
    out[f"{name}/new_unpad"] = np.array(unpad, np.int64)  # (w, h)
    out[f"{name}/borders"] = np.array(borders, np.int64)  # top, bottom, left, right
    gains, pads, bin_, bout = [], [], [], []
    for (h, w), (t, b, l, r) in zip(shapes, borders):
        n = 24
        lo = rng.uniform(-20, np.array([W, H]) + 10, (n, 2))
        box = np.concatenate([lo, lo + rng.uniform(0.5, 40, (n, 2))], 1).astype(np.float32)
        box[0] = (-5.25, 10.5, 20.125, 30.0)          # leaves on the left
        box[1] = (W - 12.5, 8.0, W + 6.75, 20.5)      # right
        box[2] = (l + 1.0, -7.5, l + 9.0, t + 4.25)   # top
        box[3] = (l + 1.0, H - 9.5, l + 9.0, H + 3.0)  # bottom
        seen = {"min": [], "round": []}
        ops.min = lambda *a, _s=seen: (_s["min"].append(min(*a)), _s["min"][-1])[1]
        ops.round = lambda v, _s=seen: (_s["round"].append(round(v)), _s["round"][-1])[1]
        try:
            res = ops.scale_boxes((H, W), torch.from_numpy(box.copy()), (h, w, 3))
        finally:
            del ops.min, ops.round
        assert len(seen["min"]) == 1 and len(seen["round"]) == 2
        gains.append(seen["min"][0])
        pads.append(seen["round"])
        bin_.append(box)
        bout.append(res.numpy())
        o = bout[-1]
        assert (o[:, [0, 2]] == 0).any() and (o[:, [0, 2]] == w).any() and (o[:, [1, 3]] == 0).any() and (o[:, [1, 3]] == h).any(), (name, h, w)
    out[f"{name}/gain"] = np.array(gains, np.float64)
    out[f"{name}/pad"] = np.array(pads, np.int64)  # (padw, padh)
    out[f"{name}/boxes_in"] = np.stack(bin_)
    out[f"{name}/boxes_out"] = np.stack(bout)
    return borders, unpad


def main():
    R.import_reference()
    from ultralytics.data import augment as A
    from ultralytics.data import dataset as D
    from ultralytics.data.dataset import YOLODataset
    from ultralytics.utils import ops
    import torch
    D.torch = torch  # the reference's data/dataset.py uses torch in collate_fn without importing it
    log = []
    install_cv2(log)
    text = np.load(os.path.join(ROOT, "tests", "golden", "yolo2d_labels.npz"))["label_text"]
    out = {"imgsz": np.array(IMGSZ), "stride": np.array(STRIDE), "pad": np.array(PAD), "rect_sets": np.array(list(RECT_SETS)),
           "predict_sets": np.array(list(PREDICT_SETS))}
    root = tempfile.mkdtemp(prefix="y3d_rect_")
    try:
        img_dir = T.write_tree(root, text)
        for name, batch in RECT_SETS.items():
            ar, ds = rect_set(YOLODataset, img_dir, batch, out, name)
            if name == "b4":
                bs = [tuple(int(v) for v in x) for x in ds.batch_shapes]
                assert bs == [(64, 96), (96, 96), (96, 64)], bs  # maxi < 1, neither, mini > 1
                assert int((ar == 1).sum()) == 3  # a tie
            else:
                assert int((ds.batch == ds.batch[-1]).sum()) == 2  # a ragged last batch
    finally:
        shutil.rmtree(root, ignore_errors=True)
    rng = np.random.default_rng(20261018)
    seen_b, seen_u = [], []
    for name, shapes in PREDICT_SETS.items():
        b, u = predict_set(A, ops, log, shapes, out, name, rng)
        seen_b += b
        seen_u += u
    assert any(l != r for _, _, l, r in seen_b) and any(t != b for t, b, _, _ in seen_b) and any(v == (0, 0, 0, 0) for v in seen_b)
    assert (18, 64) in seen_u  # 37 * 0.5 = 18.5 rounds to even
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): rect sets {list(RECT_SETS)}, predict sets {list(PREDICT_SETS)}")


if __name__ == "__main__":
    main()
