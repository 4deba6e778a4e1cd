"""The depth predictor (modules.DepthPredictor) at the training shape: B = 32, 1280 x 384, S-3D widths (128, 256, 512), bf16.

    python tools/depth_predictor_bench.py [--batch 32] [--iters 20]                  # forward + backward with HIP events, launch count
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/depth_predictor_bench.py --iters 5     # per-kernel times, a run of its own

Prints the predictor's forward + backward time (median of --iters after a warm-up), the number of library launches of one forward +
backward (counted at the binding), and for every new kernel the bytes it moves at this shape, so that a kernel trace's times turn into
bytes over time against the 6.29 TB/s copy rate."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import modules, ops  # noqa: E402

COPY_RATE = 6.29e12


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args(argv)
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    B, ch, sizes = a.batch, (128, 256, 512), ((48, 160), (24, 80), (12, 40))
    m = modules.DepthPredictor(ch).to("cuda")
    feats = [ops.to_nhwc(torch.randn(B, c, *s, device="cuda"), torch.bfloat16).requires_grad_(True) for c, s in zip(ch, sizes)]
    cot = torch.randn(B, 81, *sizes[1], device="cuda").bfloat16()

    def step():
        for f in feats:
            f.grad = None
        m.zero_grad(set_to_none=True)
        logits = m(feats)[0]
        logits.backward(cot)

    L = ops.lib()
    counts = {}
    for name in [n[4:] for n in L.protos if n not in ("y3d_last_error",)]:
        fn = getattr(L, name)

        def wrapped(*args, _n=name, _fn=fn):
            counts[_n] = counts.get(_n, 0) + 1
            return _fn(*args)

        setattr(L, name, wrapped)
    step()
    step()
    counts.clear()
    step()
    torch.cuda.synchronize()
    plain = {"gn_chunks", "colsum_blocks", "conv_kpad", "conv2d_wgrad_plan", "conv2d_stat_rows", "conv2d_route", "conv2d_wgrad_splits"}
    launches = {k: v for k, v in counts.items() if k not in plain}
    print(f"library calls of one forward + backward: {sum(launches.values())}  {dict(sorted(launches.items()))}")
    times = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    print(f"forward + backward, B = {B}: median {statistics.median(times):.3f} ms, min {min(times):.3f} ms over {a.iters} iterations")
    M = B * sizes[1][0] * sizes[1][1]
    mb = M * 128 * 2
    rows = (("gn_stats_kernel (3 sources)", 2 * 3 * mb), ("gn_stats_kernel (1 source)", 2 * mb), ("gn_apply_kernel<3>", 4 * mb), ("gn_apply_kernel<1>", 2 * mb),
            ("gn_bwd_reduce_kernel<3>", 4 * mb), ("gn_bwd_reduce_kernel<1>", 2 * mb), ("gn_bwd_apply_kernel<3>", 7 * mb), ("gn_bwd_apply_kernel<1>", 3 * mb),
            ("resize_fwd_kernel", mb // 4 * 5), ("resize_bwd_kernel", mb // 4 * 5), ("colsum_part_kernel", M * 88 * 2), ("depth_expect_kernel", 2 * M * 88 * 2))
    print("bytes per launch at this shape (time at the 6.29 TB/s copy rate):")
    for name, nbytes in rows:
        print(f"  {name:30s} {nbytes / 1e6:8.2f} MB   {nbytes / COPY_RATE * 1e6:6.2f} us")


if __name__ == "__main__":
    main()
