"""Times the KITTI batch builder at B = 32: the label encoder launch (`kitti.encode_labels`, HIP events) and the host-side stages of
`kitti.build_batch` (PNG read / decode, the random draws, the uploads, the image augmentation, the label encoding) on the 12-frame tree
of tests/golden/kitti_labels.npz (KITTI-sized frames).  Prints one JSON line; no target is claimed.

    python tools/kitti_labels_bench.py [--batch 32] [--iters 200]
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
from kitti_labels_tree import fixture, write_tree  # noqa: E402

from yolov10_3d_amd import kitti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    dev = "cuda"
    z = fixture()
    root = write_tree(tempfile.mkdtemp(prefix="y3d_kitti_bench_"), z, images=True)
    n = len(z["label_text"])
    items = [i % n for i in range(a.batch)]  # frames 0 .. n-1 repeated: batch slot p < n holds frame p
    args = kitti.data_args()
    path = lambda sub, i, ext: os.path.join(root, "training", sub, f"{i:06d}.{ext}")
    from PIL import Image

    def sync_ms(t0):
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    stages = {k: [] for k in ("read_decode", "draws", "upload", "image_aug", "label_pack", "label_encode", "build_batch")}
    for it in range(12):
        np.random.seed(it)
        t0 = time.perf_counter()
        frames = [Image.open(path("image_2", i, "png")) for i in items]
        arrs = [np.array(im.convert("RGB")) for im in frames]
        labels = [kitti.read_label(path("label_2", i, "txt")) for i in items]
        calibs = [kitti.read_calib(path("calib", i, "txt")) for i in items]
        stages["read_decode"].append(sync_ms(t0))
        t0 = time.perf_counter()
        info = lambda p: ((calibs[p][0, 2], calibs[p][1, 2], calibs[p][0, 0], calibs[p][1, 1]), len(labels[p]["type"]),
                          tuple(int(v) for v in z["frame_wh"][p]))
        draws = kitti.sample_augment(n, items, info, args)
        P2s = [kitti.flip_calib(P, im.size) if d["flip"] else P for P, im, d in zip(calibs, frames, draws)]
        stages["draws"].append(sync_ms(t0))
        t0 = time.perf_counter()
        imgs = [torch.from_numpy(x).to(dev) for x in arrs]
        parts = [imgs[d["partner"] % len(imgs)] if d["mixed"] else None for d in draws]
        stages["upload"].append(sync_ms(t0))
        t0 = time.perf_counter()
        kitti.augment_images(imgs, parts, [d["flip"] for d in draws], [d["trans_inv"] for d in draws], kitti.RESOLUTION, mode="uint8")
        stages["image_aug"].append(sync_ms(t0))
        t0 = time.perf_counter()
        packed = kitti.pack_labels(labels, [labels[d["partner"] % len(labels)] if d["mixed"] else None for d in draws], P2s,
                                   [d["trans"] for d in draws], [d["flip"] for d in draws], [d["scale"] for d in draws],
                                   [im.size for im in frames], dev)
        stages["label_pack"].append(sync_ms(t0))
        t0 = time.perf_counter()
        kitti.encode_labels(packed)
        stages["label_encode"].append(sync_ms(t0))
        t0 = time.perf_counter()
        kitti.build_batch(root, items, args, dev)
        stages["build_batch"].append(sync_ms(t0))
    host = {k: round(statistics.median(v[2:]), 3) for k, v in stages.items()}
    # the encoder launch alone, device time
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for _ in range(10):
        kitti.encode_labels(packed)
    for s, e in ev:
        s.record()
        kitti.encode_labels(packed)
        e.record()
    torch.cuda.synchronize()
    dev_ms = sorted(s.elapsed_time(e) for s, e in ev)
    print(json.dumps({"bench": "kitti_labels", "batch": a.batch, "encode_labels_ms_median": round(dev_ms[len(dev_ms) // 2], 4),
                      "encode_labels_ms_p10": round(dev_ms[len(dev_ms) // 10], 4), "host_stage_ms_median": host}))


if __name__ == "__main__":
    main()
