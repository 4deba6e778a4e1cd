"""Times the 2D batch builder at B = 32, imgsz = 640 from files and from a split resident on the device (`yolo2d.DeviceSplit`), on the
frame mix of tools/yolo2d_bench.py (24 frames of 640 x 480, 480 x 640 and 500 x 375, 12-40 boxes each, default hyper-parameters)
written to a temporary directory.  Reports the path-based `yolo2d.build_batch` (wall time to the finished batch); the cached one as
host wall time (the call only enqueues work) and as wall time to the finished batch; the host-built records over the same resident
frames (`_build_square_batch` on the DeviceSplit: no file, but the five record arrays, the pointer table and the label table built on
the host and uploaded), which is what the plan kernel replaces; the host time of the draws and of the draw table alone; the device time
of the three launches (HIP events around each, medians of --iters); the one-off load (time, bytes); and a cached rect batch against
the path-based one.  Prints one JSON line; no target is claimed: the yardstick is the path-based builder in the same run.

    python tools/yolo2d_cache_bench.py [--batch 32] [--imgsz 640] [--iters 100]
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
    root = tempfile.mkdtemp(prefix="y3d_yolo2d_cache_bench_")
    try:
        run(a, write_tree(root, text, wh))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def run(a, img_dir):
    dev = "cuda"
    args = yolo2d.data_args()
    med = lambda v: round(statistics.median(v), 4)

    def seed(n):
        random.seed(n)
        np.random.seed(n)

    def wall_ms(fn, sync):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    plain = yolo2d.Split(img_dir, a.imgsz, a.batch)
    n = len(plain)
    for i in range(n):  # the sizes come from the file headers once; keep that out of the build time, as tools/yolo2d_bench.py does
        plain.size(i)
    items = [i % n for i in range(a.batch)]
    disk = []
    for it in range(12):
        seed(it)
        disk.append(wall_ms(lambda: yolo2d.build_batch(plain, items, args, dev, max_boxes=256), True))
    loads = []
    for _ in range(3):
        t0 = time.perf_counter()
        split = yolo2d.DeviceSplit(img_dir, a.imgsz, a.batch, device=dev)
        torch.cuda.synchronize()
        loads.append((time.perf_counter() - t0) * 1e3)
    arena = yolo2d.DeviceSplit(img_dir, a.imgsz, a.batch, device=dev)  # the same frames, records built on the host
    host, done, host_built, draws, table = [], [], [], [], []
    for it in range(a.iters + 5):
        seed(it)
        host.append(wall_ms(lambda: split.build_batch(items, args, max_boxes=256), False))
        seed(it)
        done.append(wall_ms(lambda: split.build_batch(items, args, max_boxes=256), True))
        seed(it)
        host_built.append(wall_ms(lambda: yolo2d._build_square_batch(arena, items, args, dev, "train", 256, False, "uint8"), True))
        seed(it)
        t0 = time.perf_counter()
        samples = [yolo2d.sample_augment(arena, i, args) for i in items]
        draws.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        d = yolo2d.draw_table(samples)
        table.append((time.perf_counter() - t0) * 1e3)
    # the three launches, each between two events, on the draws of the last seed
    d_host = torch.from_numpy(d)
    d_dev = d_host.to(dev)
    plan = yolo2d.plan_batch(split, d_host, d_dev)
    pi = {"src": split.src, "rec_i": plan["rec_i"], "rec_f": plan["rec_f"], "lut": plan["lut"], "imgsz": a.imgsz}
    pl = {"rec": split.rec, "n_rec": split.n_rec, "lab_i": plan["lab_i"], "lab_f": plan["lab_f"]}
    stages = {"plan_batch": lambda: yolo2d.plan_batch(split, d_host, d_dev, out=plan),
              "image_aug": lambda: yolo2d.augment_images(pi, "uint8"),
              "encode_labels": lambda: yolo2d.encode_labels(pl, a.imgsz, 256)}
    device_ms = {}
    for name, fn in stages.items():
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
        for _ in range(10):
            fn()
        for s, e in ev:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        device_ms[name] = med([s.elapsed_time(e) for s, e in ev])
    # a rect batch of the validator's dataset
    rect = yolo2d.RectSplit(img_dir, a.imgsz, a.batch)
    t0 = time.perf_counter()
    rect_dev = yolo2d.DeviceRectSplit(img_dir, a.imgsz, a.batch, device=dev)
    torch.cuda.synchronize()
    rect_load = (time.perf_counter() - t0) * 1e3
    first = rect.batches()[0]
    rect_disk = [wall_ms(lambda: yolo2d.build_batch(rect, first, args, dev, mode="val"), True) for _ in range(12)]
    rect_host = [wall_ms(lambda: yolo2d.build_batch(rect_dev, first, args, dev, mode="val"), False) for _ in range(a.iters + 5)]
    rect_done = [wall_ms(lambda: yolo2d.build_batch(rect_dev, first, args, dev, mode="val"), True) for _ in range(a.iters + 5)]
    print(json.dumps({"bench": "yolo2d_cache", "batch": a.batch, "imgsz": a.imgsz, "frames": n, "device": torch.cuda.get_device_name(0),
                      "disk_build_batch_ms_median": med(disk[2:]),
                      "cached_build_batch_host_ms_median": med(host[5:]), "cached_build_batch_finished_ms_median": med(done[5:]),
                      "arena_host_built_records_finished_ms_median": med(host_built[5:]),
                      "draws_host_ms_median": med(draws[5:]), "draw_table_host_ms_median": med(table[5:]),
                      "cached_launch_device_ms_median": device_ms, "cached_launches_device_ms_sum": round(sum(device_ms.values()), 4),
                      "load_ms_median": med(loads), "load_ms_first": round(loads[0], 3), "arena_bytes": split.nbytes,
                      "rect_batch_images": len(first), "rect_disk_build_batch_ms_median": med(rect_disk[2:]),
                      "rect_cached_build_batch_host_ms_median": med(rect_host[5:]),
                      "rect_cached_build_batch_finished_ms_median": med(rect_done[5:]), "rect_load_ms": round(rect_load, 3)}))


if __name__ == "__main__":
    main()
