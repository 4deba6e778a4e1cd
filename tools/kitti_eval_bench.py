"""Times the device KITTI evaluator (yolov10_3d_amd.kitti_eval) on a synthetic KITTI-val-sized set.

    python tools/kitti_eval_bench.py [--images 3769] [--dets 50] [--gts 6] [--reps 5]

get_official_eval_result for Car, Pedestrian and Cyclist (three metrics each, AOS on), timed in two parts: packing the annos into
box records + upload, and the evaluation proper (overlaps, both statistics passes, the host threshold scan and the AP tables; ends in
a device synchronise) and, separately, the text
parsing of the same set written as KITTI files (eval_from_scratch's host side).  Prints one JSON line.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(rng, n_img, n_det, n_gt):
    names = np.array(["Car", "Car", "Car", "Pedestrian", "Cyclist", "Van", "DontCare"])
    gts, dts = [], []
    for _ in range(n_img):
        ng = int(rng.integers(max(n_gt - 3, 1), n_gt + 4))
        loc = np.stack([rng.uniform(-15, 15, ng), rng.uniform(1, 2.5, ng), rng.uniform(5, 60, ng)], 1).astype(np.float32)
        dims = np.stack([rng.uniform(0.8, 4.5, ng), rng.uniform(1.4, 1.9, ng), rng.uniform(0.6, 1.8, ng)], 1).astype(np.float32)
        x1, y1 = rng.uniform(0, 1100, ng), rng.uniform(100, 250, ng)
        bbox = np.stack([x1, y1, x1 + rng.uniform(20, 200, ng), y1 + rng.uniform(15, 150, ng)], 1).astype(np.float32)
        g = {"name": names[rng.integers(0, len(names), ng)], "bbox": bbox, "location": loc, "dimensions": dims,
             "rotation_y": rng.uniform(-3.14, 3.14, ng).astype(np.float32), "alpha": rng.uniform(-3.14, 3.14, ng).astype(np.float32),
             "occluded": rng.integers(0, 3, ng).astype(np.float32), "truncated": rng.choice([0.0, 0.1, 0.4], ng).astype(np.float32)}
        src = rng.integers(0, ng, n_det)
        d = {"name": np.where(rng.random(n_det) < 0.8, g["name"][src], "Car"), "bbox": g["bbox"][src] + rng.normal(0, 3, (n_det, 4)).astype(np.float32),
             "location": g["location"][src] + rng.normal(0, 0.3, (n_det, 3)).astype(np.float32),
             "dimensions": g["dimensions"][src] * (1 + rng.normal(0, 0.05, (n_det, 3))).astype(np.float32),
             "rotation_y": g["rotation_y"][src] + rng.normal(0, 0.1, n_det).astype(np.float32),
             "alpha": g["alpha"][src] + rng.normal(0, 0.2, n_det).astype(np.float32),
             "occluded": np.zeros(n_det, np.float32), "truncated": np.zeros(n_det, np.float32),
             "score": (rng.integers(1, 100, n_det) / 100).astype(np.float32)}
        d["name"] = np.where(d["name"] == "DontCare", "Car", d["name"])
        gts.append(g)
        dts.append(d)
    return gts, dts


def write_text(root, gts, dts):
    def line(a, i, det):
        f = lambda v: f"{float(v):.2f}"
        l, h, w = a["dimensions"][i]
        vals = [a["alpha"][i], *a["bbox"][i], h, w, l, *a["location"][i], a["rotation_y"][i]] + ([a["score"][i]] if det else [])
        return " ".join([str(a["name"][i]), f(a["truncated"][i]), str(int(a["occluded"][i]))] + [f(v) for v in vals])

    for sub, annos, det in (("label_2", gts, False), ("preds", dts, True)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for k, a in enumerate(annos):
            with open(os.path.join(root, sub, f"{k:06d}.txt"), "w") as fh:
                fh.write("".join(line(a, i, det) + "\n" for i in range(len(a["name"]))))
    return os.path.join(root, "label_2"), os.path.join(root, "preds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3769)
    ap.add_argument("--dets", type=int, default=50)
    ap.add_argument("--gts", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from yolov10_3d_amd import kitti_eval as KE
    if not torch.cuda.is_available():
        raise SystemExit("kitti_eval_bench needs a HIP device")
    rng = np.random.default_rng(0)
    gts, dts = synth(rng, args.images, args.dets, args.gts)
    classes = ["Car", "Pedestrian", "Cyclist"]

    def device_part():
        t0 = time.perf_counter()
        P = KE.Packed(gts, dts)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = [KE.get_official_eval_result(gts, dts, c, _packed=P) for c in classes]
        torch.cuda.synchronize()
        return out, t1 - t0, time.perf_counter() - t1

    first = device_part()[0]   # warm-up: code objects, allocator
    pack, times = [], []
    for _ in range(args.reps):
        _, tp, te = device_part()
        pack.append(tp)
        times.append(te)
    with tempfile.TemporaryDirectory() as tmp:
        gd, dd = write_text(tmp, gts, dts)
        files = sorted(os.listdir(dd))
        ptimes = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            [KE.read_label_file(os.path.join(gd, f)) for f in files]
            [KE.read_label_file(os.path.join(dd, f), det=True) for f in files]
            ptimes.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        KE.eval_from_scratch(gd, dd, classes)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
    print(json.dumps({"metric": "kitti_eval_official_3cls", "images": args.images, "dets_per_image": args.dets,
                      "gts_total": int(sum(len(g["name"]) for g in gts)), "pack_upload_ms_median": 1e3 * float(np.median(pack)),
                      "device_eval_ms_median": 1e3 * float(np.median(times)),
                      "device_eval_ms_all": [round(1e3 * t, 2) for t in times], "text_parse_ms_median": 1e3 * float(np.median(ptimes)),
                      "eval_from_scratch_ms": 1e3 * whole, "car_3d_moderate_ap40": first[0]["detail"]["Car"]["3d@0.70"][1]}))


if __name__ == "__main__":
    main()
