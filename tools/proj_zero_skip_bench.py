"""Zero-skip of the head projection backward (csrc/proj_bn_mfma.hip, y3d_set_proj_zero_skip) on the bench step's own launches.

One eager bench step (synthetic batch -> model -> loss -> backward) runs with spies on y3d_proj_group_bn_bwd (modes 0 / 1) and
y3d_proj_group_bwd_weight_bn_mfma.  While the step's tensors are alive, each spied launch is repeated with the switch off and on
alternating (HIP events, ROUNDS rounds of REPS launches per arm; median [min..max] of the rounds, in us), on
  (a) dense random `dout` of the same shape      - the class branches / crowded images: on must not be slower than off's spread
  (b) the step's real `dout`                     - what the flagship workload gives the kernels
and the share of active chunks (16 / 32 pixels with a non-+0 value in the branch's outputs) is printed per level and head set.

    python tools/proj_zero_skip_bench.py [--batch 32] [--imgsz 640] [--reps 10] [--rounds 5]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops  # noqa: E402
from bench import synth_batch  # noqa: E402

# argument positions in the two entry points (include/y3d.h)
BN = {"dout": 6, "dsw": 7, "couts": 9, "nb": 1, "cin": 2, "P": 21}
WG = {"dout": 5, "dsw": 6, "couts": 7, "nb": 0, "cin": 1, "P": 15}


def time_arms(L, fn, args, reps, rounds):
    """-> {0: [us per launch, one per round], 1: [...]}, the switch alternating off / on inside every round"""
    out = {0: [], 1: []}
    old = L.set_proj_zero_skip(1)
    try:
        for sw in (0, 1):  # warm
            L.set_proj_zero_skip(sw)
            fn(*args)
        for _ in range(rounds):
            for sw in (0, 1):
                L.set_proj_zero_skip(sw)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn(*args)
                e1.record()
                torch.cuda.synchronize()
                out[sw].append(e0.elapsed_time(e1) / reps * 1e3)
    finally:
        L.set_proj_zero_skip(old)
    return out


def fmt(v):
    return f"{statistics.median(v):7.1f} [{min(v):6.1f}..{max(v):6.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--model", default="yolov10s_3D.yaml")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = y3d.lib()
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(a.model).to(dev).train()
    if hasattr(model.model[-1], "restack"):
        model.model[-1].restack()
    batch = synth_batch(a.batch, a.imgsz, a.imgsz, seed=1, device=dev, nc=model.yaml["nc"])
    rows, shares = [], []
    real = {"bn": L.proj_group_bn_bwd, "wg": L.proj_group_bwd_weight_bn_mfma}
    g = torch.Generator(device=dev).manual_seed(3)

    def measure(kind, name, pos, args):
        P, dsw = args[pos["P"]], args[pos["dsw"]]
        dense = torch.randn(P * dsw, device=dev, generator=g).to(torch.bfloat16)
        alt = list(args)
        alt[pos["dout"]] = dense.data_ptr()
        ta, tb = time_arms(L, real[kind], alt, a.reps, a.rounds), time_arms(L, real[kind], args, a.reps, a.rounds)
        rows.append((P, args[pos["cin"]], name, ta, tb))

    def spy_bn(*args):
        measure("bn", "bn reduce" if args[0] == 0 else "bn apply", BN, args)
        return real["bn"](*args)

    def spy_wg(*args):
        measure("wg", "weight grad (+ slab fold)", WG, args)
        return real["wg"](*args)

    orig_backward = ops.FusedConvBNProjFn.backward

    def backward(ctx, dout):
        B, tot, H, W = dout.shape
        d = dout.permute(0, 2, 3, 1).reshape(B * H * W, tot).contiguous().view(torch.int16)
        n = len(ctx.meta[0])
        couts = [int(w.shape[0]) for w in list(ctx.saved_tensors)[-n:]]
        off, per = 0, []
        for co in couts:
            nz = (d[:, off:off + co] != 0).any(1)
            off += co
            sh = []
            for chunk in (16, 32):
                pad = torch.zeros(-(-nz.numel() // chunk) * chunk, dtype=torch.bool, device=nz.device)
                pad[:nz.numel()] = nz
                sh.append(float(pad.view(-1, chunk).any(1).float().mean()))
            per.append((co, float(nz.float().mean()), sh[0], sh[1]))
        shares.append((B * H * W, per))
        return orig_backward(ctx, dout)

    L.proj_group_bn_bwd, L.proj_group_bwd_weight_bn_mfma = spy_bn, spy_wg
    ops.FusedConvBNProjFn.backward = staticmethod(backward)
    try:
        loss, _ = model(batch)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        L.proj_group_bn_bwd, L.proj_group_bwd_weight_bn_mfma = real["bn"], real["wg"]
        ops.FusedConvBNProjFn.backward = staticmethod(orig_backward)
    assert rows, "the step made no MFMA head-projection backward launch"
    print(f"us per launch, median [min..max] of {a.rounds} rounds x {a.reps} launches, switch off / on alternating")
    print(f"{'P':>8} {'cin':>4} {'kernel':<26} | {'(a) dense off':>24} {'(a) dense on':>24} | {'(b) real off':>24} {'(b) real on':>24}")
    tot = [0.0] * 4
    for P, cin, name, ta, tb in sorted(rows, key=lambda r: (-r[0], r[2])):
        print(f"{P:8d} {cin:4d} {name:<26} | {fmt(ta[0]):>24} {fmt(ta[1]):>24} | {fmt(tb[0]):>24} {fmt(tb[1]):>24}")
        for i, v in enumerate((ta[0], ta[1], tb[0], tb[1])):
            tot[i] += statistics.median(v)
    print(f"sum of medians (us): dense off {tot[0]:.1f} on {tot[1]:.1f} | real off {tot[2]:.1f} on {tot[3]:.1f}")
    print("share of pixels / 16-pixel chunks / 32-pixel chunks with a non-+0 dout value, per branch (cout):")
    for P, per in sorted(shares, key=lambda s: -s[0]):
        half = len(per) // 2
        for tag, part in (("head set 0", per[:half]), ("head set 1", per[half:])):
            cells = "  ".join(f"({co}) {100 * px:.2f}/{100 * c16:.1f}/{100 * c32:.1f}" for co, px, c16, c32 in part)
            print(f"  P={P:<7d} {tag}: {cells}")


if __name__ == "__main__":
    main()
