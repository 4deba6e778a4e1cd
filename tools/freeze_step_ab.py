"""Frozen layers, end to end (results: profiles/freeze_step_ab.txt): the eager micro-step - forward, loss, backward - of
one model with `freeze` None / 11 (the backbone) / 23 (everything but the head), in ONE process on one MI355X.  Three models are
built from one seed and frozen with `train.apply_freeze`; the settings run in alternating blocks whose order rotates every round.
Per block: device time between two events, the host time until the last launch of the block is enqueued, and
`torch.cuda.max_memory_allocated()` (the three models are resident throughout: about 3 x the parameters sit under every peak).
Medians over the blocks and their range are printed.

    python tools/freeze_step_ab.py [--yaml yolov10s_3D.yaml] [--batch 32] [--imgsz 640] [--block 10] [--blocks 5]
    python tools/freeze_step_ab.py --arm 11 --steps 10     # one setting only, for a kernel trace in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/freeze_step_ab.py --arm 11 --steps 10
      (launches per micro-step: the difference of the dispatch counts of two such runs over the difference of their --steps; the
       first steps of a process also pack weights and build tables)"""
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

ARMS = {"none": None, "11": 11, "23": 23}


def build(name, freeze):
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(name).to("cuda").train()
    model.model[-1].restack()
    frozen = train.apply_freeze(model, freeze)
    return model, len(frozen)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--yaml", default="yolov10s_3D.yaml")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--arm", choices=tuple(ARMS), default=None)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    y3d.set_compute_dtype(torch.bfloat16)
    batches = [bench.synth_batch(a.batch, a.imgsz, a.imgsz, 100 + j, "cuda") for j in range(4)]

    def steps(model, n):
        items = None
        for j in range(n):
            loss, items = model(batches[j % len(batches)])
            loss.backward()
            del loss
            model.zero_grad(set_to_none=True)
        return items

    if a.arm is not None:
        model, nf = build(a.yaml, ARMS[a.arm])
        items = steps(model, a.steps)
        torch.cuda.synchronize()
        print(f"freeze {a.arm}: {nf} frozen tensors, {a.steps} micro-steps, last items {[round(float(v), 4) for v in items]}", flush=True)
        return
    models = {}
    for arm, freeze in ARMS.items():
        models[arm], nf = build(a.yaml, freeze)
        items = steps(models[arm], 3)  # warm-up: every shape of every setting
        n = sum(p.numel() for p in models[arm].parameters())
        nt = sum(p.numel() for p in models[arm].parameters() if p.requires_grad)
        print(f"freeze {arm:4s}: {nf} frozen tensors, {nt / 1e6:.2f} of {n / 1e6:.2f} M parameters trainable; items after warm-up "
              f"{[round(float(v), 4) for v in items]}", flush=True)
    torch.cuda.synchronize()
    dev_ms, host_ms, peak = ({k: [] for k in ARMS} for _ in range(3))
    order = list(ARMS)
    for r in range(a.blocks):
        for arm in order[r % 3:] + order[:r % 3]:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            steps(models[arm], a.block)
            host_ms[arm].append(1e3 * (time.perf_counter() - t0) / a.block)
            e1.record()
            torch.cuda.synchronize()
            dev_ms[arm].append(e0.elapsed_time(e1) / a.block)
            peak[arm].append(torch.cuda.max_memory_allocated() / 2 ** 20)
    print(f"{a.yaml}, B = {a.batch}, {a.imgsz}x{a.imgsz}, bf16, eager micro-step (forward + loss + backward), {a.blocks} alternating blocks of "
          f"{a.block} micro-steps per setting")
    rng = lambda v: f"median {statistics.median(v):8.3f} (min {min(v):8.3f}, max {max(v):8.3f})"
    for arm in ARMS:
        print(f"  freeze {arm:4s}: device ms per micro-step {rng(dev_ms[arm])}; host enqueue ms {rng(host_ms[arm])}; "
              f"peak allocated {max(peak[arm]):.0f} MiB", flush=True)
    base = statistics.median(dev_ms["none"])
    for arm in ("11", "23"):
        d = statistics.median(dev_ms[arm])
        print(f"  freeze {arm} against none: {d - base:+.3f} ms device per micro-step ({100 * (d - base) / base:+.1f} %)")


if __name__ == "__main__":
    main()
