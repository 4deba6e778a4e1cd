"""Times assignment plus loss of one 2D head set (loss.Loss2dFn: y3d_tal2d_assign or y3d_tal2d_assign_crowded, then y3d_loss2d) on
crowded batches.

    python tools/crowded_loss_bench.py [--reps 30] [--batch 32] [--size 640] [--nc 80]

B = 32 images of 640 x 640 (8400 anchors over strides 8 / 16 / 32), 80 classes, bf16 maps, with 8, 64, 256 and 512 boxes in EVERY image.
Up to 64 boxes both routes run on the same maps and targets: the dense one on 64-row targets (max_boxes=None) and the crowded one on
128-row targets (max_boxes=128), alternating inside the timed loop; above 64 only the crowded one exists (capacity = the box count).
A call is timed between two device events; the median over the reps is reported, after three untimed calls per route.  The targets are
padded once, outside the timed window.  Prints one JSON line per box count.  Not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows_of(g, B, per_image, nc):
    """(B * per_image, 6) label rows [batch_idx | cls | box xywh in [0, 1]], images interleaved"""
    n = B * per_image
    bi = (torch.arange(n) % B).float().view(n, 1)
    cls = torch.randint(0, nc, (n, 1), generator=g).float()
    cxy = 0.05 + 0.9 * torch.rand(n, 2, generator=g)
    wh = 0.03 + 0.22 * torch.rand(n, 2, generator=g)
    return torch.cat((bi, cls, cxy, wh), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    args = ap.parse_args()
    import yolov10_3d_amd as y3d
    from yolov10_3d_amd import loss as PL
    from yolov10_3d_amd._lib import lib
    dev = torch.device("cuda")
    y3d.set_compute_dtype(torch.bfloat16)
    B, S, nc = args.batch, args.size, args.nc
    strides = [8.0, 16.0, 32.0]
    g = torch.Generator().manual_seed(0)
    maps = [y3d.ops._dense_any(torch.randn(B, 64 + nc, int(S // s), int(S // s), generator=g).to(dev), torch.bfloat16) for s in strides]
    A = sum(m.shape[2] * m.shape[3] for m in maps)
    cfg = PL.LossCfg2d(strides, nc, 10, 0.5, 6.0, (7.5, 0.5, 1.5))

    def call(gt, n_used):
        return PL.Loss2dFn.apply(cfg, gt, n_used, *maps)

    for per_image in (8, 64, 256, 512):
        rows = rows_of(g, B, per_image, nc).to(dev)
        routes = {}
        if per_image <= PL.TARGET_CAP:
            routes["dense"] = PL.pad_targets(rows, B, 5, (float(S), float(S)))
        routes["crowded"] = PL.pad_targets(rows, B, 5, (float(S), float(S)), cap=max(128, per_image))
        PL.check_target_overflow(wait=True)
        out = {}
        for name, (gt, n_used) in routes.items():
            for _ in range(3):
                out[name] = call(gt, n_used)
        torch.cuda.synchronize()
        times = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, (gt, n_used) in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(gt, n_used)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        res = {"metric": "crowded_loss", "boxes_per_image": per_image, "batch": B, "anchors": A, "classes": nc, "dtype": "bf16", "reps": args.reps}
        for name, (gt, _) in routes.items():
            n = gt.shape[1]
            fl = lib().tal2d_scratch_floats(B, n, A, 10) if name == "crowded" else lib().tal3d_scratch_floats(B, n, A, 10)
            res[f"{name}_ms"] = round(float(np.median(times[name])), 3)
            res[f"{name}_min_ms"] = round(float(np.min(times[name])), 3)
            res[f"{name}_rows"] = n
            res[f"{name}_scratch_mb"] = round(fl * 4 / 2 ** 20, 1)
            res[f"{name}_fg"] = int(out[name][2].sum())
        if len(routes) == 2:
            res["routes_equal"] = bool(torch.equal(out["dense"][2], out["crowded"][2]) and torch.equal(out["dense"][3], out["crowded"][3])
                                       and torch.equal(out["dense"][1], out["crowded"][1]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
