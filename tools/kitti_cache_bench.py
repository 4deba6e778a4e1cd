"""Times the KITTI batch builder at B = 32 from disk and from a split resident on the device (`kitti.DeviceSplit`), on the 12-frame
tree of tests/golden/kitti_labels.npz (KITTI-sized frames) written to a temporary directory: the path-based `kitti.build_batch` (wall
time to the finished batch), the cached one as host wall time (the call only enqueues work), as wall time to the finished batch and as
device time of its three launches (HIP events around each), and the one-off load (time, bytes).  Prints one JSON line; no target is
claimed.

    python tools/kitti_cache_bench.py [--batch 32] [--iters 50]
"""
import argparse
import json
import os
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
from kitti_labels_tree import fixture, write_tree  # noqa: E402

from yolov10_3d_amd import kitti, ops  # noqa: E402
from yolov10_3d_amd._lib import lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    z = fixture()
    root = write_tree(tempfile.mkdtemp(prefix="y3d_kitti_cache_bench_"), z, images=True)
    try:
        n = len(z["label_text"])
        items = [i % n for i in range(a.batch)]
        args = kitti.data_args()
        med = lambda v: round(statistics.median(v), 4)

        def wall_ms(fn, sync):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        disk = []
        for it in range(12):
            np.random.seed(it)
            disk.append(wall_ms(lambda: kitti.build_batch(root, items, args, dev), True))
        loads = []
        for _ in range(3):
            t0 = time.perf_counter()
            split = kitti.DeviceSplit(root, device=dev)
            torch.cuda.synchronize()
            loads.append((time.perf_counter() - t0) * 1e3)
        host, done = [], []
        for it in range(a.iters + 5):
            np.random.seed(it)
            host.append(wall_ms(lambda: split.build_batch(items, args), False))
            np.random.seed(it)
            done.append(wall_ms(lambda: split.build_batch(items, args), True))
        # the three launches, each between two events, on the draws of one seed
        np.random.seed(0)
        draws = kitti.sample_augment(n, items, split.frame_info, args)
        table = torch.from_numpy(kitti.draw_table(items, draws))
        table_dev = table.to(dev)
        plan = kitti.plan_batch(split, table, table_dev)
        W, H = kitti.RESOLUTION
        img = torch.empty(a.batch, H, W, 3, dtype=torch.uint8, device=dev)
        packed = {"rec": split.rec, "img_i": plan["img_i"], "img_f": plan["img_f"], "mean_size": split.mean_size}
        stages = {
            "plan_batch": lambda: kitti.plan_batch(split, table, table_dev, out=plan),
            "image_aug": lambda: lib().kitti_image_aug(plan["src"].data_ptr(), plan["src2"].data_ptr(), plan["hw"].data_ptr(), plan["flip"].data_ptr(),
                                                       plan["trans_inv"].data_ptr(), a.batch, H, W, 1, img.data_ptr(), ops.stream()),
            "encode_labels": lambda: kitti.encode_labels(packed),
        }
        device_ms = {}
        for name, fn in stages.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
            for _ in range(5):
                fn()
            for s, e in ev:
                s.record()
                fn()
                e.record()
            torch.cuda.synchronize()
            device_ms[name] = med([s.elapsed_time(e) for s, e in ev])
        print(json.dumps({"bench": "kitti_cache", "batch": a.batch, "frames": n, "disk_build_batch_ms_median": med(disk[2:]),
                          "cached_build_batch_host_ms_median": med(host[5:]), "cached_build_batch_finished_ms_median": med(done[5:]),
                          "cached_launch_device_ms_median": device_ms, "cached_launches_device_ms_sum": round(sum(device_ms.values()), 4),
                          "load_ms_median": med(loads), "load_ms_first": round(loads[0], 3), "arena_bytes": split.nbytes}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
