"""Times the Waymo batch builder at B = 32 with mixup on, on a synthetic Waymo-shaped tree written to a temporary directory (64 PNG
frames of 1920 x 1280, one camera, a few boxes each), in three arms: the path-based `json3d.build_batch`, which opens and decodes
every frame and every mixup partner per batch; a `json3d.DeviceSplit` with every frame in HBM; and the same split with every frame in
the pinned host tier (`max_bytes=0`), from where the distinct frames of a batch are copied to the device per batch.  Per arm: the host
wall time of a build (the resident builds only enqueue work) and the device time between two events recorded around it; for the two
splits also the one-off load.  Prints one JSON line; no target is claimed.

    python tools/json3d_cache_bench.py [--batch 32] [--iters 30] [--frames 64]
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

from yolov10_3d_amd import json3d, kitti  # noqa: E402

W, H = 1920, 1280
CALIB = [[2055.0, 0.0, 939.0, 0.0], [0.0, 2055.0, 641.0, 0.0], [0.0, 0.0, 1.0, 0.0]]


def write_tree(root, frames):
    """`frames` PNGs of W x H (a smooth pattern under seeded noise, so the files neither collapse to nothing nor are pure noise) and
    the split JSON with three boxes per frame -> the JSON's path"""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:W]
    images, anns = [], []
    for i in range(frames):
        px = np.stack([(xx // (3 + c) + yy // (2 + c) + 41 * i + 67 * c) % 256 for c in range(3)], -1) + rng.randint(-6, 7, (H, W, 3))
        name = f"images/{i:06d}.png"
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8), "RGB").save(os.path.join(root, name), compress_level=3)
        images.append({"id": i, "file_name": name, "calib": CALIB})
        for k in range(3):
            z = 12.0 + 9.0 * k + (i % 5)
            x = -4.0 + 4.0 * k
            u, v = CALIB[0][0] * x / z + CALIB[0][2], CALIB[1][1] * 1.0 / z + CALIB[1][2]
            anns.append({"image_id": i, "category_id": 1 + (k + i) % 3, "bbox": [u - 60.0, v - 90.0, 120.0, 100.0], "dim": [1.6, 1.9, 4.4],
                         "translation": [x, 1.0, z], "rotation_y": 0.3 * k - 0.2, "num_lidar": 50})
    path = os.path.join(root, "split.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": anns}, f)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--disk-iters", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda"
    root = tempfile.mkdtemp(prefix="y3d_json3d_cache_bench_")
    try:
        path = write_tree(root, a.frames)
        file_bytes = sum(os.path.getsize(os.path.join(root, "images", f)) for f in os.listdir(os.path.join(root, "images")))
        args = kitti.data_args()
        assert args.mixup
        med = lambda v: round(statistics.median(v), 4)
        order = np.random.RandomState(1).permutation(a.frames)
        items = [int(order[i % a.frames]) for i in range(a.batch)]

        def timed(build, seed):
            """-> (host ms until the call returns, device ms between the events around it)"""
            np.random.seed(seed)
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            t0 = time.perf_counter()
            build()
            host = (time.perf_counter() - t0) * 1e3
            e.record()
            torch.cuda.synchronize()
            return host, s.elapsed_time(e)

        def arm(build, iters, warm):
            t = [timed(build, it) for it in range(warm + iters)][warm:]
            return {"host_ms_median": med([h for h, _ in t]), "device_ms_median": med([d for _, d in t])}

        out = {"bench": "json3d_cache", "batch": a.batch, "frames": a.frames, "frame_wh": [W, H], "png_bytes": file_bytes,
               "decoded_bytes": a.frames * W * H * 3}
        out["path"] = arm(lambda: json3d.build_batch(path, items, args, dev, dataset="waymo"), a.disk_iters, 1)
        for name, kw in (("hbm", dict(max_bytes=None)), ("host", dict(max_bytes=0, host_bytes=a.frames * W * H * 3))):
            t0 = time.perf_counter()
            split = json3d.DeviceSplit(path, "waymo", device=dev, **kw)
            torch.cuda.synchronize()
            load = (time.perf_counter() - t0) * 1e3
            assert split.n_dev == (a.frames if name == "hbm" else 0)
            np.random.seed(0)
            staged = split._stage([p for pos, d in zip(items, split.sample(items, args)) for p in (pos, d["partner"])])[0]
            out[name] = dict(arm(lambda: split.build_batch(items, args), a.iters, 5), load_ms=round(load, 1), n_dev=split.n_dev,
                             staged_frames_seed0=len(staged))
            del split
        for name in ("hbm", "host"):
            out[name]["host_ratio_to_path"] = round(out["path"]["host_ms_median"] / out[name]["host_ms_median"], 1)
            out[name]["device_ratio_to_path"] = round(out["path"]["device_ms_median"] / out[name]["device_ms_median"], 1)
        print(json.dumps(out))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
