"""What the confusion-matrix launch adds to a validation pass: `val.Validator3d` on YOLOv10-S-3D (random weights) at batch 32 with
plots=True and plots=False, on the synthetic KITTI tree of tests/kitti_labels_tree.py (its 12 frames listed 8 times: 96 images at
1280 x 384).  One warm-up pass, then the median wall time of five passes each; one JSON line.

    python tools/validator_bench.py [--graph]
"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import yolov10_3d_amd as y3d  # noqa: E402
from kitti_labels_tree import fixture, write_tree  # noqa: E402
from yolov10_3d_amd import val  # noqa: E402


def main():
    import torch
    graph = "--graph" in sys.argv
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10s_3D.yaml")).to("cuda")
    with tempfile.TemporaryDirectory() as tmp:
        z = fixture()
        root = write_tree(tmp, z, images=True)
        n = len(z["label_text"])
        open(os.path.join(root, "ImageSets", "val.txt"), "w").write("".join(f"{i % n:06d}\n" for i in range(8 * n)))
        out = {"model": "yolov10s_3D", "batch": 32, "images": 8 * n, "graph": graph}
        for plots in (True, False):
            v = val.Validator3d(model, root, batch=32, plots=plots, graph=graph)
            v()
            times = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                v()
                times.append(time.perf_counter() - t0)
            med = statistics.median(times)
            out[f"plots_{plots}"] = {"images_per_s": round(v.seen / med, 1), "pass_s": [round(t, 4) for t in times], "speed_ms_per_image": v.speed}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
