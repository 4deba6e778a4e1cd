"""Times the Waymo / Omni3D batch builder at B = 32: the label encoder launch (`json3d.encode_labels`, HIP events) and the host-side
stages of `json3d.build_batch` (PNG read / decode, JSON parse and record packing, the random draws, the uploads, the image
augmentation, the label encoding) on the 12-frame splits of tests/golden/waymo_labels.npz / omni3d_labels.npz (frames a quarter of
Waymo's size).  Prints one JSON line per dataset; no target is claimed.

    python tools/json3d_labels_bench.py [--batch 32] [--iters 200] [--dataset waymo omni3d]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from json3d_tree import fixture, write_tree  # noqa: E402

from yolov10_3d_amd import json3d, kitti  # noqa: E402


def bench(dataset, batch, iters):
    from PIL import Image
    dev = "cuda"
    z = fixture(dataset)
    path = write_tree(tempfile.mkdtemp(prefix=f"y3d_{dataset}_bench_"), z, dataset, images=True)
    n = len(z["img_id"])
    items = [i % n for i in range(batch)]
    args = kitti.data_args()

    def sync_ms(t0):
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    stages = {k: [] for k in ("json_parse", "read_decode", "draws", "upload", "image_aug", "label_pack", "label_encode", "build_batch")}
    for it in range(12):
        np.random.seed(it)
        t0 = time.perf_counter()
        sp = json3d.Split(path, dataset)
        recs = [sp.records(sp.ids[p]) for p in range(n)]
        stages["json_parse"].append(sync_ms(t0))
        t0 = time.perf_counter()
        frames = [Image.open(sp.file(sp.ids[p])).convert("RGB") for p in items]
        arrs = [np.array(im) for im in frames]
        stages["read_decode"].append(sync_ms(t0))
        t0 = time.perf_counter()
        draws = []
        for p, im in zip(items, frames):
            first = [True]

            def info(q, _first=first, _size=im.size):
                size, _first[0] = (_size if _first[0] else None), False
                P = sp.P2(sp.ids[q])
                return (P[0, 2], P[1, 2], P[0, 0], P[1, 1]), len(recs[q]), size

            draws += kitti.sample_augment(n, [p], info, args, "train", json3d.MAX_OBJS, json3d.RESOLUTION)
        P2s = [json3d.flip_calib(sp.P2(sp.ids[p]), im.size) if d["flip"] else sp.P2(sp.ids[p]) for p, im, d in zip(items, frames, draws)]
        stages["draws"].append(sync_ms(t0))
        t0 = time.perf_counter()
        imgs = [torch.from_numpy(x).to(dev) for x in arrs]
        parts = [imgs[d["partner"] % len(imgs)] if d["mixed"] else None for d in draws]
        stages["upload"].append(sync_ms(t0))
        t0 = time.perf_counter()
        kitti.augment_images(imgs, parts, [d["flip"] for d in draws], [d["trans_inv"] for d in draws], json3d.RESOLUTION, mode="uint8")
        stages["image_aug"].append(sync_ms(t0))
        t0 = time.perf_counter()
        packed = json3d.pack_labels([recs[p] for p in items], [recs[d["partner"]] if d["mixed"] else None for d in draws], P2s,
                                    [d["trans"] for d in draws], [d["flip"] for d in draws], [d["scale"] for d in draws],
                                    [im.size for im in frames], dev, dataset)
        stages["label_pack"].append(sync_ms(t0))
        t0 = time.perf_counter()
        json3d.encode_labels(packed)
        stages["label_encode"].append(sync_ms(t0))
        t0 = time.perf_counter()
        json3d.build_batch(path, items, args, dev, dataset=dataset)  # the split stays parsed between calls
        stages["build_batch"].append(sync_ms(t0))
    host = {k: round(statistics.median(v[2:]), 3) for k, v in stages.items()}
    # the encoder launch alone, device time
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(10):
        json3d.encode_labels(packed)
    for s, e in ev:
        s.record()
        json3d.encode_labels(packed)
        e.record()
    torch.cuda.synchronize()
    dev_ms = sorted(s.elapsed_time(e) for s, e in ev)
    print(json.dumps({"bench": f"json3d_labels_{dataset}", "batch": batch, "objects": int(packed["rec"].shape[0]),
                      "encode_labels_ms_median": round(dev_ms[len(dev_ms) // 2], 4), "encode_labels_ms_p10": round(dev_ms[len(dev_ms) // 10], 4),
                      "host_stage_ms_median": host}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--dataset", nargs="+", default=["waymo", "omni3d"])
    a = ap.parse_args()
    for d in a.dataset:
        bench(d, a.batch, a.iters)


if __name__ == "__main__":
    main()
