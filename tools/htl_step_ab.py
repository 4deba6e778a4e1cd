"""Hierarchical task learning, end to end: the S-3D micro-step (forward + loss + backward) with the loss items weighted from the device
table (`htl` on: y3d_loss3d_weighted, loss = sum(weights * items)) against the step as it was (`htl` off: y3d_loss3d, loss = sum(items) * B),
in ONE process on the same model and batches, in alternating blocks of eager micro-steps whose order flips every round (host clock
around a device synchronise).  The figures are medians over the blocks, the spread is printed.  Then the `y3d_htl_update` launch alone:
the median over blocks of back-to-back launches, each block between two synchronises.
    python tools/htl_step_ab.py [--yaml yolov10s_3D.yaml] [--batch 32] [--imgsz 640] [--block 10] [--blocks 6]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (synth_batch)
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default="yolov10s_3D.yaml")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev, B = "cuda", a.batch
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(a.yaml).to(dev).train()
    model.model[-1].restack()
    batches = [bench.synth_batch(B, a.imgsz, a.imgsz, 100 + j, dev) for j in range(4)]
    model.criterion = model.init_criterion()
    hw = train.HtlWeights(dev)
    hw.table.copy_(torch.tensor([0.8, 0.8, 0.4, 0.3, 0.2, 0.5] * 2))  # every item weighted: the rows all carry work

    def steps(n, on):
        model.criterion.set_item_weights(hw.table if on else None)
        items = None
        for j in range(n):
            loss, items = model(batches[j % len(batches)])
            loss.backward()
            model.zero_grad(set_to_none=True)
        return items

    for on in (False, True):  # warm-up: every shape of both arms
        items = steps(3, on)
        print(f"htl {'on ' if on else 'off'}: last items {[round(float(v), 4) for v in items]}", flush=True)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for r in range(a.blocks):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(a.block, on)
            torch.cuda.synchronize()
            ms[on].append(1e3 * (time.perf_counter() - t0) / a.block)
    off, on_ = statistics.median(ms[False]), statistics.median(ms[True])
    fmt = lambda v: "[" + ", ".join(f"{x:.2f}" for x in v) + "]"  # noqa: E731
    print(f"{a.yaml}, B={B}, {a.imgsz}x{a.imgsz}, eager micro-step, {a.blocks} x {a.block} per arm: htl off {off:.2f} ms {fmt(ms[False])}; "
          f"on {on_:.2f} ms {fmt(ms[True])}; ratio on/off {on_ / off:.4f}", flush=True)
    items = items.detach().float().contiguous()
    us = []
    for r in range(a.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e in range(100):
            hw.update(items, 6 + e % 50)
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0) / 100)
    print(f"y3d_htl_update: {statistics.median(us):.1f} us per launch, back to back (100 per block) [" + ", ".join(f"{x:.1f}" for x in us) + "]", flush=True)


if __name__ == "__main__":
    main()
