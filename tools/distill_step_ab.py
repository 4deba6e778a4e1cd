"""Feature distillation, end to end: training images/s of the S-3D step with `distillation` off (the yardstick: the step as it was)
against the same step with it on, against a resident random teacher map, in ONE process on the same model, optimizer and batches, in
alternating blocks of eager steps whose order flips every round (host clock around a device synchronise).  The figures are medians
over the blocks, the spread is printed.
    python tools/distill_step_ab.py [--yaml yolov10s_3D.yaml] [--batch 32] [--imgsz 640] [--block 10] [--blocks 4]
    python tools/distill_step_ab.py --arm on --steps 6      # one arm only, for a kernel trace (rocprofv3 --kernel-trace --stats -- python ...)"""
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
from yolov10_3d_amd import loss as PL  # noqa: E402
from yolov10_3d_amd.optim import build_optimizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default="yolov10s_3D.yaml")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--arm", choices=("on", "off"), default=None)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev, B = "cuda", a.batch
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(a.yaml).to(dev).train()
    head = model.model[-1]
    opt = build_optimizer(model)
    head.restack()
    C = head.dep[0][0].conv.out_channels
    batches = [bench.synth_batch(B, a.imgsz, a.imgsz, 100 + j, dev) for j in range(4)]
    g = torch.Generator().manual_seed(9)
    for b in batches:  # a DINOv2-sized map (patch 14) in the compute dtype, resident on the device; every fourth image mixed
        b["teacher_emb"] = torch.randn(B, C, a.imgsz // 14, a.imgsz // 14, generator=g).to(dev).bfloat16()
        b["mixed"] = (torch.arange(B) % 4 == 0).to(torch.uint8).to(dev)
    crits = {}
    for on in (False, True):
        model.args.distillation = on
        crits[on] = PL.DetectLoss3d(model)

    def steps(n, on):
        model.criterion, head.distill = crits[on], on
        items = None
        for j in range(n):
            loss, items = model(batches[j % len(batches)])
            loss.backward()
            opt.step(max_norm=10.0)
            opt.zero_grad()
        return items

    if a.arm is not None:
        items = steps(a.steps, a.arm == "on")
        torch.cuda.synchronize()
        print(f"arm {a.arm}: {a.steps} steps, last items {[round(float(v), 4) for v in items]}", flush=True)
        return
    for on in (False, True):  # warm-up: every shape of both arms
        items = steps(3, on)
        print(f"distillation {'on ' if on else 'off'}: {items.numel()} items, last {[round(float(v), 4) for v in items]}", flush=True)
    torch.cuda.synchronize()
    ips = {False: [], True: []}
    for r in range(a.blocks):
        for on in ((False, True) if r % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(a.block, on)
            torch.cuda.synchronize()
            ips[on].append(a.block * B / (time.perf_counter() - t0))
    off, on_ = statistics.median(ips[False]), statistics.median(ips[True])
    fmt = lambda v: "[" + ", ".join(f"{x:.1f}" for x in v) + "]"
    print(f"{a.yaml}, B={B}, {a.imgsz}x{a.imgsz}, eager, {a.blocks} x {a.block} steps per arm: distillation off {off:.1f} images/s {fmt(ips[False])}; "
          f"on {on_:.1f} images/s {fmt(ips[True])}; ratio {on_ / off:.4f}; extra time per step {1e3 * B * (1 / on_ - 1 / off):.3f} ms", flush=True)


if __name__ == "__main__":
    main()
