"""Validate a model on a split: a thin command line over `val.Validator3d` / `val.Validator2d`.

    python tools/validate.py yolov10s_3D.yaml --weights s3d.pt --data /data/kitti                       # KITTI root or split file
    python tools/validate.py yolov10s_3D.yaml --weights s3d.pt --data waymo/val.json --dataset waymo    # Waymo / Omni3D split JSON
    python tools/validate.py yolov10n.yaml --weights n.pt --data /data/coco/images/val2017 --imgsz 640  # 2D: an image directory or list
    python tools/validate.py yolov10s_3D.yaml --weights s3d.pt --data /data/kitti --use-o2m-depth      # depths voted by the one-to-many set

The checkpoint is a state_dict (or a pickled model, or a dict with "model" / "ema") and goes through `BaseModel.load`.  Prints the
results dict, the speed and the confusion matrix ([predicted, true], the last index is background)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import val, yolo2d  # noqa: E402


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", help="model yaml, e.g. yolov10s_3D.yaml or yolov10n.yaml")
    ap.add_argument("--weights", help="checkpoint for BaseModel.load (random weights without it)")
    ap.add_argument("--data", required=True, help="KITTI root / split file, a Waymo / Omni3D split JSON, or a 2D image directory / list")
    ap.add_argument("--dataset", default="kitti", choices=("kitti", "waymo", "omni3d"))
    ap.add_argument("--nc", type=int)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640, help="2D models: the rect split's image size")
    ap.add_argument("--conf", type=float, default=0.001)
    ap.add_argument("--max-det", type=int)
    ap.add_argument("--single-cls", action="store_true")
    ap.add_argument("--no-plots", action="store_true", help="skip the confusion matrix")
    ap.add_argument("--graph", action="store_true", help="replay the eval forward from a hipGraph")
    ap.add_argument("--use-o2m-depth", action="store_true",
                    help="3D models: every depth becomes the vote of the one-to-many proposals (the reference's use_o2m_depth)")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.use_o2m_depth and not any(row[2] == "v10Detect3d" for row in y3d.yaml_model_load(a.model)["head"]):
        ap.error("--use-o2m-depth applies to the 3D models")
    cfg = y3d.yaml_model_load(a.model)
    is3d = any(row[2] == "v10Detect3d" for row in cfg["head"])
    model = (y3d.YOLOv10_3DDetectionModel if is3d else y3d.YOLOv10DetectionModel)(cfg, nc=a.nc)
    if a.weights:
        ck = torch.load(a.weights, map_location="cpu", weights_only=False)
        if isinstance(ck, dict) and not all(torch.is_tensor(v) for v in ck.values()):
            ck = ck.get("ema") or ck.get("model") or ck
        got, own = model.load(ck)
        print(f"loaded {got} of {own} tensors from {a.weights}")
    model = model.to("cuda")
    common = dict(conf=a.conf, single_cls=a.single_cls, plots=not a.no_plots, graph=a.graph)
    if is3d:
        v = val.Validator3d(model, a.data, dataset=a.dataset, batch=a.batch, max_det=a.max_det or 50, use_o2m_depth=a.use_o2m_depth,
                            **common)
    else:
        split = yolo2d.RectSplit(a.data, a.imgsz, a.batch, int(model.stride.max()))
        v = val.Validator2d(model, split, max_det=a.max_det or 300, **common)
    results = v()
    print({k: float(x) for k, x in results.items()})
    print("images", v.seen, "targets per class", v.nt_per_class.tolist(), "speed (ms per image)", v.speed)
    if not a.no_plots:
        np.set_printoptions(linewidth=200, suppress=True)
        print(v.confusion_matrix.matrix.astype(np.int64))


if __name__ == "__main__":
    main()
