"""Measurements of the gradient-accumulation route (results: profiles/train_accum_ab.txt).

    python tools/train_accum_ab.py kernel  [--models yolov10s_3D.yaml yolov10x_3D.yaml]   # y3d_mt_grad_acc over a model's parameter tables
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/train_accum_ab.py kernel     # ... the same under the kernel trace, a run of its own
    python tools/train_accum_ab.py micro   [--model yolov10s_3D.yaml --batch 32 --imgsz 640]  # micro-step 2 of a window: arena route / autograd route
    python tools/train_accum_ab.py trainer [--model yolov10s_3D.yaml --batch 32 --imgsz 640]  # Trainer.fit images/s over one synthetic epoch

kernel:  the launch `GradAccumulator.add()` makes (every parameter of the model, chunk 16384), timed with device events over enough
         launches to exceed a second; traffic = 12 bytes per element (8 read, 4 written).
micro:   the SECOND micro-batch of an accumulate-2 window, which is where the routes differ - forward + loss + backward + `add()` into
         the arena, against forward + loss + backward with autograd adding into the persistent `p.grad` tensor by tensor.  The two are
         alternated (ABAB...), each timed span holds enough micro-steps to exceed a second, medians and the spread of the repeats are
         printed.  Both are launched eagerly.
trainer: `Trainer.fit` over one epoch of a resident synthetic split (bench.synth_batch), images per second from the host clock
         around fit(), no validator."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import optim, train  # noqa: E402
from bench import synth_batch  # noqa: E402

DEV = "cuda"


def build(name):
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(name).to(DEV).train()
    model.model[-1].restack()
    return model


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernel(a):
    for name in a.models:
        model = build(name)
        ps = [p for p in model.parameters() if p.requires_grad]
        acc = optim.GradAccumulator(ps)
        n = sum(p.numel() for p in ps)
        grads = [torch.randn_like(p) for p in ps]

        for p, g in zip(ps, grads):
            p.grad = g
        acc.add()  # builds the tables and uploads the gradient pointers; the timed loop repeats its launch without the host work around it
        tb = acc._tabs[next(iter(acc._tabs))]
        L, st = y3d.lib(), torch.cuda.current_stream().cuda_stream
        args = (tb.ptr["arena"].data_ptr(), tb.col["grads"].dev.data_ptr(), tb.sizes.data_ptr(), *tb.chunks, st)

        def add():
            L.mt_grad_acc(*args)

        for _ in range(5):
            add()
        torch.cuda.synchronize()
        spans = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            acc.reset()
            e0.record()
            for _ in range(a.launches):
                add()
            e1.record()
            torch.cuda.synchronize()
            spans.append(e0.elapsed_time(e1) / a.launches)
        ms = median(spans)
        print(f"kernel {name}: {len(ps)} tensors, {n / 1e6:.2f} M elements, {tb.nchunks} workgroups; "
              f"{1e3 * ms:.1f} us per launch (median of {a.repeats} x {a.launches} back-to-back launches, min {1e3 * min(spans):.1f}, "
              f"max {1e3 * max(spans):.1f}); {12 * n / (ms * 1e-3) / 1e12:.2f} TB/s at 12 B per element", flush=True)
        del model, acc, grads


def micro(a):
    model = build(a.model)
    ps = [p for p in model.parameters() if p.requires_grad]
    acc = optim.GradAccumulator(ps)
    batches = [synth_batch(a.batch, a.imgsz, a.imgsz, 1 + j, DEV) for j in range(4)]
    k = [0]

    def fwd_bwd():
        b = batches[k[0] % len(batches)]
        k[0] += 1
        loss, _ = model(b)
        loss.backward()

    def arena_first():
        acc.reset()
        for p in ps:
            p.grad = None
        fwd_bwd()
        acc.add()

    def arena_second():
        fwd_bwd()
        acc.add()

    def autograd_first():
        for p in ps:
            p.grad = None
        fwd_bwd()

    def autograd_second():
        fwd_bwd()  # AccumulateGrad adds into the persistent p.grad, one launch per tensor

    routes = {"arena": (arena_first, arena_second), "autograd": (autograd_first, autograd_second)}
    for first, second in routes.values():
        for _ in range(3):
            first()
            second()
    torch.cuda.synchronize()
    spans = {r: [] for r in routes}
    host = {r: [] for r in routes}
    for _ in range(a.repeats):
        for r, (first, second) in routes.items():
            first()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.steps):
                second()  # (every one of them is a "second" micro-step: the sums only grow, nothing steps)
            e1.record()
            host[r].append(1e3 * (time.perf_counter() - t0) / a.steps)
            torch.cuda.synchronize()
            spans[r].append(e0.elapsed_time(e1) / a.steps)
    print(f"micro-step 2 of a window, {a.model}, B = {a.batch}, {a.imgsz}x{a.imgsz}, bf16, eager; {a.repeats} alternating repeats of {a.steps} micro-steps")
    for r in routes:
        v = spans[r]
        print(f"  {r:9s} median {median(v):.3f} ms per micro-step (min {min(v):.3f}, max {max(v):.3f}; the span's host enqueue time: median "
              f"{median(host[r]):.3f} ms); {len(ps) if r == 'autograd' else 1} accumulate launch(es)", flush=True)
    d = median(spans["autograd"]) - median(spans["arena"])
    print(f"  autograd - arena = {d:+.3f} ms per micro-step ({100 * d / median(spans['autograd']):+.2f} %)")


class SynthSplit:
    """`nbatch` resident synthetic batches served as one epoch"""

    def __init__(self, batch, imgsz, nbatch):
        self.batches = [synth_batch(batch, imgsz, imgsz, 1 + j, DEV) for j in range(nbatch)]
        self.n = batch * nbatch

    def __len__(self):
        return self.n

    def epoch(self, batch, args, shuffle=True, seed=0):
        return iter(self.batches)


def trainer(a):
    model = build(a.model)
    split = SynthSplit(a.batch, a.imgsz, a.nbatch)
    for label in ("first epoch (tables, packs and allocator warm up)", "second run"):
        t = train.Trainer(model, split, None, epochs=1, batch=a.batch, nbs=2 * a.batch, warmup_epochs=0, optimizer="SGD", lr0=0.01)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.fit()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"Trainer.fit {a.model}, B = {a.batch}, {a.imgsz}x{a.imgsz}, accumulate 2, {a.nbatch} batches, {label}: {len(split) / dt:.1f} images/s "
              f"({1e3 * dt / a.nbatch:.2f} ms per micro-step incl. half an optimizer step + EMA update)", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernel", "micro", "trainer"))
    ap.add_argument("--models", nargs="+", default=["yolov10s_3D.yaml", "yolov10x_3D.yaml"])
    ap.add_argument("--model", default="yolov10s_3D.yaml")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=40, help="micro: micro-steps per timed span")
    ap.add_argument("--launches", type=int, default=12000, help="kernel: launches per timed span")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nbatch", type=int, default=48, help="trainer: batches of the synthetic epoch")
    a = ap.parse_args(argv)
    {"kernel": kernel, "micro": micro, "trainer": trainer}[a.what](a)


if __name__ == "__main__":
    main()
