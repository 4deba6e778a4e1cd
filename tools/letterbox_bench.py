"""Times the letter-box kernels (csrc/letterbox.hip) at B = 32 with HIP events, medians of --iters launches, and prints one JSON line.

`y3d_letterbox_image`, uint8 and float output, four placements:
  * 640 x 640 canvas, copy path: 640 x 480 sources at top = 80 (a rect / predict letter-box of ratio 1);
  * 640 x 640 canvas, resize path: 500 x 375 sources resized to 640 x 480 (what `load_image` + a ratio-1 letter-box amount to);
  * 448 x 640 canvas, resize path: 640 x 480 sources resized to 597 x 448 at left = 21 (the predictor's letter-box into that canvas);
  * 448 x 640 canvas, copy path: 597 x 448 sources at left = 21 (a 640 x 480 source cannot be copied into a 448-row canvas).
Next to each time: the bytes the launch moves (the output written + the source pixels under the placed image, each counted once) over
the time.  For scale the same run times `yolo2d.augment_images` (the square training batch builder) at B = 32, imgsz
640, and the two small kernels: `y3d_letterbox_labels` (32 images, 12-40 rows each, cap 64) and `y3d_predict_rows` (32 x 300 rows).
No target is claimed.

    python tools/letterbox_bench.py [--batch 32] [--iters 200]
"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo2d_tree import write_tree  # noqa: E402

from yolov10_3d_amd import predict, yolo2d  # noqa: E402

DEV = "cuda"


def device_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(10):
        fn()
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return {"median": round(ms[len(ms) // 2], 4), "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[(len(ms) * 9) // 10], 4)}


def image_case(B, H, W, h0, w0, nh, nw, iters, rng):
    top, left = int(round((H - nh) / 2 - 0.1)), int(round((W - nw) / 2 - 0.1))
    imgs = [torch.from_numpy(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).to(DEV) for _ in range(B)]
    rec = np.array([[b, h0, w0, nh, nw, top, left, b % 2] for b in range(B)], np.int32)
    packed = yolo2d.pack_letterbox(imgs, rec, H, W, DEV)
    out = {"canvas": [H, W], "source": [h0, w0], "placed": [nh, nw], "path": "copy" if (nh, nw) == (h0, w0) else "resize"}
    for mode, px in (("uint8", 3), ("float", 12)):
        t = device_ms(lambda: yolo2d.letterbox_images(packed, mode), iters)
        moved = B * (H * W * px + h0 * w0 * 3)
        out[mode] = dict(t, bytes=moved, TBps=round(moved / (t["median"] * 1e-3) / 1e12, 3))
    return out


def augment_case(B, iters):
    """the square training batch of tools/yolo2d_bench.py: 24 frames of 640 x 480, 480 x 640 and 500 x 375, default hyper-parameters"""
    rng = np.random.default_rng(7)
    wh = [[(640, 480), (480, 640), (500, 375)][i % 3] for i in range(24)]
    text = []
    for i in range(24):
        rows = []
        for _ in range(int(rng.integers(12, 41))):
            w, h = rng.uniform(0.05, 0.4, 2)
            rows.append(f"{rng.integers(80)} {rng.uniform(w / 2, 1 - w / 2):.6f} {rng.uniform(h / 2, 1 - h / 2):.6f} {w:.6f} {h:.6f}\n")
        text.append("".join(rows))
    root = tempfile.mkdtemp(prefix="y3d_letterbox_bench_")
    try:
        split = yolo2d.Split(write_tree(root, text, wh), 640, B)
        random.seed(0)
        np.random.seed(0)
        items = [i % len(split) for i in range(B)]
        for _ in range(3):  # fill the mosaic buffer as a running loader has it
            samples = [yolo2d.sample_augment(split, i, yolo2d.data_args()) for i in items]
        frames = sorted({t["frame"] for s in samples for pre in (s["pre"], s["pre2"]) if pre is not None for t in pre["tiles"]})
        imgs = [split.decode(f, DEV) for f in frames]
        ri, rf, lut = yolo2d.image_records(samples, {f: n for n, f in enumerate(frames)})
        pi = yolo2d.pack_images(imgs, ri, rf, lut, 640, DEV)
        aug = device_ms(lambda: yolo2d.augment_images(pi, "uint8"), iters)
        # the label kernel on the same label files
        rect = yolo2d.RectSplit(os.path.join(root, "images"), 640, B)
        its = rect.batches()[0]
        smp = [yolo2d.rect_sample(rect, i) for i in its]
        start = np.concatenate([[0], np.cumsum([len(rect.labels[i]) for i in its])])
        _, li, lf = yolo2d.rect_records(rect, smp, {i: n for n, i in enumerate(its)}, {i: int(start[n]) for n, i in enumerate(its)})
        pl = yolo2d.pack_letterbox_labels(np.concatenate([rect.labels[i] for i in its]), li, lf, DEV)
        H, W = smp[0]["canvas"]
        lab = device_ms(lambda: yolo2d.letterbox_labels(pl, H, W), iters)
        return aug, dict(lab, images=len(its), rows=int(start[-1]))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    B = a.batch
    rng = np.random.default_rng(3)
    out = {"bench": "letterbox", "batch": B, "device": torch.cuda.get_device_name(0)}
    out["image"] = [image_case(B, 640, 640, 480, 640, 480, 640, a.iters, rng), image_case(B, 640, 640, 375, 500, 480, 640, a.iters, rng),
                    image_case(B, 448, 640, 480, 640, 448, 597, a.iters, rng), image_case(B, 448, 640, 448, 597, 448, 597, a.iters, rng)]
    aug, lab = augment_case(B, a.iters)
    out["augment_images_uint8_ms"] = aug
    out["letterbox_labels_ms"] = lab
    preds = torch.rand(B, 300, 6, device=DEV) * 640
    preds[..., 4] = torch.rand(B, 300, device=DEV)
    meta = torch.tensor([[480, 640, 1.0, 0, 80]] * B, dtype=torch.float32).to(DEV)
    out["predict_rows_ms"] = dict(device_ms(lambda: predict.predict_rows(preds, meta, 0.25), a.iters), rows=[B, 300])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
