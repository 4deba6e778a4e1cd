"""Times the drawing kernels (csrc/draw3d.hip, plot.py) at the size a validation batch has: B = 32 images of 1242 x 375 with K = 50
boxes each (700 segments per image), the BEV maps at 600 x 1200.  HIP events, medians of --iters calls after a warm-up, every launch on
its own and the two chains a user calls; for scale, the device-to-device copy of one canvas batch (what any renderer that does not
draw in place pays first), once between two fixed buffers, which stay in the 256 MB last-level cache, and once round a ring of
buffers larger than that cache, which is what a copy of fresh data costs.  One JSON line on stdout, the same line and a table in profiles/draw_bench.txt.

The boxes are `y3d_predict3d_rows`' output for the `synth` recipe of tests/predict3d_ref.py (boxes inside a 1280 x 384 canvas, depth
3 .. 63 m) at conf = 0.25 and at conf = -1 (every slot used).  Painting is idempotent, so every timed call does the same work.
No target is claimed.

    python tools/draw_bench.py [--batch 32] [--iters 200] [--out profiles/draw_bench.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import predict3d_ref as PR  # noqa: E402

from yolov10_3d_amd import plot, predict  # noqa: E402

DEV = "cuda"
H, W, K = 375, 1242, 50
BEV = dict(max_dist=60, scale=10)
RING = 8


def device_ms(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return {"median": round(ms[len(ms) // 2], 4), "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[(len(ms) * 9) // 10], 4)}


def case(B, conf, iters):
    torch.manual_seed(0)
    preds = PR.synth(torch.Generator().manual_seed(K), B, K).to(DEV)
    calib6, P2, ratio, inv = (torch.from_numpy(a).to(DEV) for a in PR.synth_camera(B))
    P2 = P2.double()
    rows, c3, _, counts = predict.predict3d_rows(preds, calib6, P2, ratio, inv, conf)
    canvas = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=DEV)
    other = torch.empty_like(canvas)
    ring = [canvas.clone() for _ in range(RING)]  # 8 x 44.7 MB and 8 x 69.1 MB: neither ring fits the last-level cache
    step = {"canvas": 0, "bev": 0}

    def ring_copy(bufs, key):
        i = step[key] = (step[key] + 1) % RING
        bufs[i].copy_(bufs[i - 1])
    R = BEV["max_dist"] * BEV["scale"]
    bev = plot.draw_bev(c3, rows, counts, **BEV)
    segs, srgb = plot.box3d_segments(c3, rows, counts, P2)
    quads, qrgb = plot.bev_quads(c3, rows, counts, BEV["scale"], R, R)
    bev_ring = [bev.clone() for _ in range(RING)]
    before = canvas.clone()
    plot.draw_segments(canvas, segs, srgb, thickness=2)
    out = {"boxes": int(counts.sum()), "segments_finite": int(torch.isfinite(segs).all(-1).sum()),
           "pixels_drawn": int((canvas != before).any(-1).sum()), "bev_pixels_drawn": int((bev != bev.new_tensor(plot.bev_background(**BEV))).any(-1).sum()),
           "ms": {
               "box3d_segments": device_ms(lambda: plot.box3d_segments(c3, rows, counts, P2), iters),
               "draw_segments_t2": device_ms(lambda: plot.draw_segments(canvas, segs, srgb, thickness=2), iters),
               "draw_segments_t5": device_ms(lambda: plot.draw_segments(canvas, segs, srgb, thickness=5), iters),
               "draw_boxes3d_chain": device_ms(lambda: plot.draw_boxes3d(canvas, c3, rows, counts, P2), iters),
               "bev_quads": device_ms(lambda: plot.bev_quads(c3, rows, counts, BEV["scale"], R, R), iters),
               "draw_quads_bev": device_ms(lambda: plot.draw_quads(bev, quads, qrgb), iters),
               "draw_bev_chain": device_ms(lambda: plot.draw_bev(c3, rows, counts, **BEV), iters),
               "copy_canvas_batch_d2d_cached": device_ms(lambda: other.copy_(canvas), iters),
               "copy_canvas_batch_d2d_ring": device_ms(lambda: ring_copy(ring, "canvas"), iters),
               "copy_bev_batch_d2d_cached": device_ms(lambda: bev_ring[1].copy_(bev_ring[0]), iters),
               "copy_bev_batch_d2d_ring": device_ms(lambda: ring_copy(bev_ring, "bev"), iters),
           }}
    return {"conf": conf, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_bench.txt"))
    a = ap.parse_args()
    out = {"bench": "draw3d", "batch": a.batch, "K": K, "canvas": [H, W], "bev": [600, 1200], "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "cases": [case(a.batch, conf, a.iters) for conf in (0.25, -1.0)]}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(f"drawing kernels, B = {a.batch}, K = {K}, canvases {W} x {H}, BEV 1200 x 600; HIP events, ms per call: median (p10 .. p90)\n")
        for c in out["cases"]:
            f.write(f"\nconf {c['conf']}: {c['boxes']} boxes, {c['segments_finite']} segments kept by the near clip, {c['pixels_drawn']} canvas pixels "
                    f"and {c['bev_pixels_drawn']} BEV pixels painted\n")
            for k, v in c["ms"].items():
                f.write(f"  {k:30s} {v['median']:.4f} ({v['p10']:.4f} .. {v['p90']:.4f})\n")
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
