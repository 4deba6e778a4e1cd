"""captured eval forward + post-process of YOLOv10-S-3D at 640 x 640, `use_o2m_depth` off vs on (the dense one-to-many head, its
post-process over 250 rows and the depth vote), timed as tools/infer_graph_ab.py times its arms:
python tools/o2m_eval_ab.py [batch] [replays]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolov10_3d_amd as y3d
import bench
from yolov10_3d_amd.graph import GraphedForward
from yolov10_3d_amd.predict import raw_rows3d

B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
y3d.set_compute_dtype(torch.bfloat16)
torch.manual_seed(0)
model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").cuda().eval()
img = bench.synth_batch(B, 640, 640, 1, "cuda")["img"]

outs = {}
for rnd in range(2):
    for flag in (False, True):
        g = GraphedForward(lambda im: raw_rows3d(model, im, 50, use_o2m_depth=flag), img)
        for _ in range(5):
            g(g.inputs[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            o = g(g.inputs[0])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        outs[flag] = o.clone()
        print(f"use_o2m_depth {flag!s:5}: {B * n / dt:9.1f} images/s, {1e3 * dt / n:.3f} ms per batch of {B}", flush=True)
        del g
keep = [c for c in range(37) if c != 33]
print("columns other than the depth identical:", torch.equal(outs[False][..., keep], outs[True][..., keep]),
      "| depths changed:", int((outs[False][..., 33] != outs[True][..., 33]).sum()), "of", outs[True][..., 33].numel())
