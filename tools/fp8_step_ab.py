"""fp8 data gradient, end to end: training images/s with fp8 weights + fp8 forward (the parent path, switch off) against the same with
`set_fp8_dgrad(True)`, in ONE process on the same model, optimizer and batches, in alternating blocks of eager steps (host clock around
a device synchronise).  The yardstick is the switch-off arm; the figures are medians over the blocks, the spread is printed.
    python tools/fp8_step_ab.py [--configs s32,x16] [--imgsz 640] [--block 10] [--blocks 4]"""
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
from yolov10_3d_amd import ops  # noqa: E402
from yolov10_3d_amd.optim import build_optimizer  # noqa: E402

CONFIGS = {"s32": ("yolov10s_3D.yaml", 32), "x16": ("yolov10x_3D.yaml", 16), "s4": ("yolov10s_3D.yaml", 4)}


def run(name, imgsz, block, blocks):
    yaml, B = CONFIGS[name]
    dev = "cuda"
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(yaml).to(dev).train()
    opt = build_optimizer(model)
    if hasattr(model.model[-1], "restack"):
        model.model[-1].restack()
    batches = [bench.synth_batch(B, imgsz, imgsz, 100 + j, dev) for j in range(4)]

    def steps(n, on):
        y3d.set_fp8_dgrad(on)
        seen = []
        for j in range(n):
            if j == 0:
                ops.TIMER = ops.KernelTimer(lambda key: seen.append(key[0]) or False)
            loss, _ = model(batches[j % len(batches)])
            loss.backward()
            ops.TIMER = None
            opt.step(max_norm=10.0)
            opt.zero_grad()
        return seen

    for on in (False, True):  # warm-up: every shape of both arms
        seen = steps(3, on)
        print(f"{name} switch {'on ' if on else 'off'}: per step conv_fwd_fp8 {seen.count('conv_fwd_fp8')}, conv_dgrad_fp8 {seen.count('conv_dgrad_fp8')}, "
              f"conv_dgrad (bf16) {seen.count('conv_dgrad')}", flush=True)
    torch.cuda.synchronize()
    ips = {False: [], True: []}
    for _ in range(blocks):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(block, on)
            torch.cuda.synchronize()
            ips[on].append(block * B / (time.perf_counter() - t0))
    off, on_ = statistics.median(ips[False]), statistics.median(ips[True])
    fmt = lambda v: "[" + ", ".join(f"{x:.1f}" for x in v) + "]"
    print(f"{name} ({yaml}, B={B}, {imgsz}x{imgsz}, eager, {blocks} x {block} steps per arm): fp8 forward only {off:.1f} images/s {fmt(ips[False])}; "
          f"+ fp8 data gradient {on_:.1f} images/s {fmt(ips[True])}; ratio {on_ / off:.4f}", flush=True)
    del model, opt, batches
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="s32,x16")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    y3d.set_compute_dtype(torch.bfloat16)
    y3d.set_weight_quant("fp8")
    y3d.set_fp8_conv(True)
    try:
        for name in a.configs.split(","):
            run(name, a.imgsz, a.block, a.blocks)
    finally:
        y3d.set_fp8_conv(False)
        y3d.set_weight_quant(None)


if __name__ == "__main__":
    main()
