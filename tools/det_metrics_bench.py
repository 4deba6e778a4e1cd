"""Times the device box metrics (yolov10_3d_amd.metrics.BoxStats) on two synthetic validation-set sizes.

    python tools/det_metrics_bench.py [--reps 5]

  * coco: 5 000 images x 300 rows (update_2d, batches of 32), about 7 gts per image, 80 classes;
  * kitti: 3 769 images x 50 decode rows (update_3d, batches of 16, about 60 % kept), about 6 gts per image, 3 classes.
The inputs are generated on the device first.  Each rep times every update_* call of the set (ending in a device synchronise) and then
get_stats (which ends in its copy back); the median of the reps is reported.  Prints one JSON line per set.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_batch(g, B, K, nc, n_gt, mode, dev):
    ng = torch.randint(max(n_gt - 4, 0), n_gt + 5, (B,), generator=g)
    bidx = torch.repeat_interleave(torch.arange(B), ng).float()
    N = int(ng.sum())
    xy = torch.rand(N, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(N, 2, generator=g) * 0.15 + 0.02
    cls = torch.randint(0, nc, (N, 1), generator=g).float()
    batch = {"batch_idx": bidx.to(dev), "cls": cls.to(dev), "bboxes": torch.cat((xy, wh), 1).to(dev)}
    S = 640
    if mode == "2d":
        H0, W0 = 480, 640
        batch.update(ori_shape=[(H0, W0)] * B, ratio_pad=[((1.0, 1.0), (0.0, 80.0))] * B, imgsz=(S, S))
        scale = torch.tensor([S, S, S, S])
    else:
        H0, W0 = 375, 1242
        batch.update(ori_shape=[(H0, W0)] * B)
        scale = torch.tensor([W0, H0, W0, H0])
    # detections: jittered copies of the gts (a third of the rows) plus random boxes
    src = torch.randint(0, max(N, 1), (B, K), generator=g)
    xyxy = torch.cat((xy - wh / 2, xy + wh / 2), 1) if N else torch.zeros(1, 4)
    box = xyxy[src] + torch.randn(B, K, 4, generator=g) * 0.01
    rnd = torch.rand(B, K, generator=g) < 0.67
    x1y1 = torch.rand(int(rnd.sum()), 2, generator=g) * 0.8
    box[rnd] = torch.cat((x1y1, x1y1 + torch.rand(int(rnd.sum()), 2, generator=g) * 0.1 + 0.02), 1)
    box = box * scale
    c = torch.where(rnd, torch.randint(0, nc, (B, K), generator=g).float(), cls.reshape(-1)[src] if N else torch.zeros(B, K))
    conf = torch.rand(B, K, generator=g)
    if mode == "2d":
        preds = torch.cat((box, conf[..., None], c[..., None]), 2).float().to(dev)
        return preds, None, batch
    rows = torch.zeros(B, K, 14, dtype=torch.float64)
    rows[..., 0], rows[..., 2:6], rows[..., 13] = c.double(), box.double(), conf.double()
    return rows.to(dev), (conf > 0.4).to(dev), batch


def bench(name, n_img, B, K, nc, n_gt, mode, reps, dev):
    import yolov10_3d_amd as y3d
    g = torch.Generator().manual_seed(0)
    data = [synth_batch(g, min(B, n_img - i), K, nc, n_gt, mode, dev) for i in range(0, n_img, B)]
    names = {i: str(i) for i in range(nc)}
    t_up, t_get, res = [], [], None
    for _ in range(reps + 1):  # the first rep warms up (allocations, code objects)
        st = y3d.metrics.BoxStats(nc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for preds, keep, batch in data:
            if mode == "2d":
                st.update_2d(preds, batch)
            else:
                st.update_3d(preds, keep, batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = st.get_stats(y3d.metrics.Det3dMetrics(names=names))
        t2 = time.perf_counter()
        t_up.append((t1 - t0) * 1e3)
        t_get.append((t2 - t1) * 1e3)
    print(json.dumps({"metric": f"det_metrics_{name}", "images": n_img, "rows_per_image": K, "classes": nc, "batch": B,
                      "update_ms": round(float(np.median(t_up[1:])), 2), "get_stats_ms": round(float(np.median(t_get[1:])), 2),
                      "map50_95": round(float(res["metrics/mAP50-95(B)"]), 5), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    bench("coco", 5000, 32, 300, 80, 7, "2d", args.reps, dev)
    bench("kitti", 3769, 16, 50, 3, 6, "3d", args.reps, dev)


if __name__ == "__main__":
    main()
