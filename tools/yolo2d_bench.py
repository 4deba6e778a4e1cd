"""Times the 2D batch builder at B = 32, imgsz = 640: the device time of each kernel (`yolo2d.augment_images`, `yolo2d.encode_labels`,
HIP events) and the host time of the stages of `yolo2d.build_batch` (PNG decode, the random draws, the uploads, the record packing,
the whole call).  The tree is written for the run: 24 frames of 640 x 480 and 480 x 640 (long side 640, so `load_image` does not
resize them) and 500 x 375 (resized to 640 x 480 by the kernel), 12-40 boxes each; default hyper-parameters, so a sample is cut from
up to eight frames.  Prints one JSON line; no target is claimed.

    python tools/yolo2d_bench.py [--batch 32] [--imgsz 640] [--iters 100]
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from yolo2d_tree import write_tree  # noqa: E402

from yolov10_3d_amd import yolo2d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    wh = [[(640, 480), (480, 640), (500, 375)][i % 3] for i in range(24)]
    text = []
    for i in range(24):
        rows = []
        for _ in range(int(rng.integers(12, 41))):
            w, h = rng.uniform(0.05, 0.4, 2)
            rows.append(f"{rng.integers(80)} {rng.uniform(w / 2, 1 - w / 2):.6f} {rng.uniform(h / 2, 1 - h / 2):.6f} {w:.6f} {h:.6f}\n")
        text.append("".join(rows))
    root = tempfile.mkdtemp(prefix="y3d_yolo2d_bench_")
    try:
        run(a, write_tree(root, text, wh))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def run(a, img_dir):
    dev = "cuda"
    split = yolo2d.Split(img_dir, a.imgsz, a.batch)
    for i in range(len(split)):  # the sizes come from the file headers once; keep that out of the draw time
        split.size(i)
    args = yolo2d.data_args()
    items = [i % len(split) for i in range(a.batch)]
    random.seed(0)
    np.random.seed(0)

    def sync_ms(t0):
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    stages = {k: [] for k in ("draws", "decode", "upload", "pack_images", "pack_labels", "build_batch")}
    boxes, frames_used = [], []
    for it in range(12):
        t0 = time.perf_counter()
        samples = [yolo2d.sample_augment(split, i, args) for i in items]
        stages["draws"].append((time.perf_counter() - t0) * 1e3)  # host only: nothing to wait for
        frames = sorted({t["frame"] for s in samples for pre in (s["pre"], s["pre2"]) if pre is not None for t in pre["tiles"]})
        frames_used.append(len(frames))
        t0 = time.perf_counter()
        arrs = [np.array(Image.open(split.im_files[f]).convert("RGB")) for f in frames]
        stages["decode"].append(sync_ms(t0))
        t0 = time.perf_counter()
        imgs = [torch.from_numpy(x).to(dev) for x in arrs]
        stages["upload"].append(sync_ms(t0))
        slot = {f: n for n, f in enumerate(frames)}
        t0 = time.perf_counter()
        ri, rf, lut = yolo2d.image_records(samples, slot)
        pi = yolo2d.pack_images(imgs, ri, rf, lut, a.imgsz, dev)
        stages["pack_images"].append(sync_ms(t0))
        t0 = time.perf_counter()
        start, row = {}, 0
        for f in frames:
            start[f] = row
            row += len(split.labels[f])
        li, lf = yolo2d.label_records(split, samples, start)
        pl = yolo2d.pack_labels(np.concatenate([split.labels[f] for f in frames]), li, lf, dev)
        stages["pack_labels"].append(sync_ms(t0))
        t0 = time.perf_counter()
        batch = yolo2d.build_batch(split, items, args, dev, max_boxes=256)
        stages["build_batch"].append(sync_ms(t0))
        boxes.append(int(batch["counts"].max()))
    host = {k: round(statistics.median(v[2:]), 3) for k, v in stages.items()}

    def device_ms(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for _ in range(10):
            fn()
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        ms = sorted(s.elapsed_time(e) for s, e in ev)
        return {"median": round(ms[len(ms) // 2], 4), "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[(len(ms) * 9) // 10], 4)}

    out = {"bench": "yolo2d", "batch": a.batch, "imgsz": a.imgsz, "frames_per_batch_median": statistics.median(frames_used),
           "largest_box_count_seen": max(boxes),
           "image_aug_uint8_ms": device_ms(lambda: yolo2d.augment_images(pi, "uint8")),
           "image_aug_float_ms": device_ms(lambda: yolo2d.augment_images(pi, "float")),
           "encode_labels_ms": device_ms(lambda: yolo2d.encode_labels(pl, a.imgsz, 256)),
           "host_stage_ms_median": host}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
