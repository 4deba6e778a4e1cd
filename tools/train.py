"""Train a model on a resident split: a thin command line over `train.Trainer`.

    python tools/train.py yolov10s_3D.yaml --data /data/kitti --epochs 100 --batch 32 --save-dir runs/s3d      # KITTI root or split file
    python tools/train.py yolov10s_3D.yaml --data waymo/train.json --val waymo/val.json --dataset waymo         # Waymo / Omni3D split JSONs
    python tools/train.py yolov10n.yaml --data /data/coco/images/train2017 --val /data/coco/images/val2017     # 2D: image directories / lists
    python tools/train.py yolov10s_3D.yaml --data /data/kitti --resume runs/s3d/weights/last.pt --save-dir runs/s3d
    python tools/train.py yolov10s_3D.yaml --data /data/kitti --htl --save-dir runs/s3d_htl                     # hierarchical task learning
    python tools/train.py yolov10s_3D.yaml --data /data/kitti --pretrained-body v10s_2d.pt --freeze 11          # transfer: frozen backbone

The training split is decoded once and held on the device (`kitti.DeviceSplit`, `json3d.DeviceSplit`, `yolo2d.DeviceSplit`); the
validator (`val.Validator3d` / `val.Validator2d`, twice the training batch as in the reference) runs on the EMA model.  Without --val
a KITTI root validates on its ImageSets/val.txt; the other datasets train without validation.  One line is printed per epoch;
`--save-dir` gets results.csv and weights/{last,best}.pt, which `tools/validate.py --weights` reads."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import json3d, kitti, train, val, yolo2d  # noqa: E402


def freeze_arg(text):
    """"11" -> 11 (layers 0..10); "0,1,2" -> [0, 1, 2]"""
    try:
        return [int(t) for t in text.split(",")] if "," in text else int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--freeze {text}: a layer count or a comma-separated list of layer indices") from None


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", help="model yaml, e.g. yolov10s_3D.yaml or yolov10n.yaml")
    ap.add_argument("--data", required=True, help="KITTI root / split file, a Waymo / Omni3D split JSON, or a 2D image directory / list")
    ap.add_argument("--val", help="the validation split, in the form of --data")
    ap.add_argument("--dataset", default="kitti", choices=("kitti", "waymo", "omni3d"))
    ap.add_argument("--weights", help="initial weights for BaseModel.load (a state_dict, or a dict with 'ema' / 'model')")
    ap.add_argument("--nc", type=int)
    ap.add_argument("--imgsz", type=int, default=640, help="2D models: the training image size")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--nbs", type=int, default=64)
    ap.add_argument("--optimizer", default="auto", choices=("SGD", "Adam", "Adamax", "AdamW", "NAdam", "RAdam", "auto"))
    ap.add_argument("--lr0", type=float, default=0.001)
    ap.add_argument("--lrf", type=float, default=0.01)
    ap.add_argument("--momentum", type=float, default=0.937)
    ap.add_argument("--weight-decay", type=float, default=0.0005)
    ap.add_argument("--warmup-epochs", type=float, default=3.0)
    ap.add_argument("--warmup-momentum", type=float, default=0.8)
    ap.add_argument("--warmup-bias-lr", type=float, default=0.1)
    ap.add_argument("--cos-lr", action="store_true")
    ap.add_argument("--close-mixup", type=int, default=0)
    ap.add_argument("--close-mosaic", type=int, default=0)
    ap.add_argument("--val-period", type=int, default=1)
    ap.add_argument("--patience", type=int, default=150)
    ap.add_argument("--save-dir")
    ap.add_argument("--save-period", type=int, default=-1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-norm", type=float, default=10.0)
    ap.add_argument("--htl", action="store_true", help="3D models: hierarchical task learning (cfg/default.yaml:121), weights kept on the device")
    ap.add_argument("--fgdm", action="store_true", help="3D KITTI models: train the head's depth predictor on the foreground depth maps "
                    "(sets fgdm_predictor, fgdm_loss and load_depth_maps; the split needs its segmentation masks)")
    ap.add_argument("--resume", help="a last.pt of this trainer: continue at its epoch + 1")
    ap.add_argument("--freeze", type=freeze_arg, help="freeze layers: N (layers 0..N-1) or a comma-separated list of layer indices, e.g. 0,1,2")
    ap.add_argument("--pretrained-body", help="fill every layer but the detection head from a trainer checkpoint or a state_dict file "
                    "(BaseModel.load_pretrained_body), e.g. a 2D model of the same scale")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    y3d.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    cfg = y3d.yaml_model_load(a.model)
    is3d = any(row[2] == "v10Detect3d" for row in cfg["head"])
    if a.fgdm:
        if not is3d or a.dataset != "kitti":
            raise SystemExit("--fgdm: the foreground depth maps exist for 3D models on KITTI only")
        cfg["fgdm_predictor"] = True
    torch.manual_seed(a.seed)
    model = (y3d.YOLOv10_3DDetectionModel if is3d else y3d.YOLOv10DetectionModel)(cfg, nc=a.nc)
    if a.weights:
        ck = torch.load(a.weights, map_location="cpu", weights_only=False)
        if isinstance(ck, dict) and not all(torch.is_tensor(v) for v in ck.values()):
            ck = ck.get("ema") or ck.get("model") or ck
        got, own = model.load(ck)
        print(f"loaded {got} of {own} tensors from {a.weights}")
    if a.pretrained_body:
        print(f"loaded {model.load_pretrained_body(a.pretrained_body)} body tensors from {a.pretrained_body}")
    model = model.to("cuda").train()
    if a.fgdm:
        model.args.fgdm_loss = True
    validator = None
    if is3d:
        if a.dataset == "kitti":
            split = kitti.DeviceSplit(a.data, mode="train", load_depth_maps=a.fgdm)
            data_args = kitti.data_args(load_depth_maps=True) if a.fgdm else kitti.data_args()
            vsrc = a.val or (a.data if os.path.isdir(a.data) else None)
            vsplit = kitti.DeviceSplit(vsrc, mode="val") if vsrc else None
        else:
            split, data_args = json3d.DeviceSplit(a.data, a.dataset, mode="train"), kitti.data_args()
            vsplit = json3d.DeviceSplit(a.val, a.dataset, mode="val") if a.val else None
        if vsplit is not None:
            validator = lambda m: val.Validator3d(m, vsplit, dataset=a.dataset, batch=2 * a.batch, plots=False)  # noqa: E731
    else:
        split, data_args = yolo2d.DeviceSplit(a.data, a.imgsz, a.batch), yolo2d.data_args()
        if a.val:
            vsplit = yolo2d.DeviceRectSplit(a.val, a.imgsz, 2 * a.batch, int(model.stride.max()))
            validator = lambda m: val.Validator2d(m, vsplit, plots=False)  # noqa: E731
    t = train.Trainer(model, split, validator, epochs=a.epochs, batch=a.batch, nbs=a.nbs, optimizer=a.optimizer, lr0=a.lr0, lrf=a.lrf,
                      momentum=a.momentum, weight_decay=a.weight_decay, warmup_epochs=a.warmup_epochs, warmup_momentum=a.warmup_momentum,
                      warmup_bias_lr=a.warmup_bias_lr, cos_lr=a.cos_lr, close_mixup=a.close_mixup, close_mosaic=a.close_mosaic,
                      val_period=a.val_period, patience=a.patience, save_dir=a.save_dir, save_period=a.save_period, seed=a.seed,
                      data_args=data_args, max_norm=a.max_norm, resume=a.resume, htl=a.htl or None, freeze=a.freeze)

    def line(h):
        skip = ("epoch", "fitness")
        print(f"epoch {h['epoch'] + 1}/{a.epochs}  " + "  ".join(f"{k} {v:.4g}" for k, v in h.items() if k not in skip and v is not None)
              + (f"  fitness {h['fitness']:.4g}" if h["fitness"] is not None else ""), flush=True)

    t.on_epoch_end = line
    t.fit()
    print(f"{len(t.history)} epochs, best fitness {t.best_fitness}, optimizer steps skipped for non-finite gradients: "
          f"{int(t.opt.last_norm[4]) if t.opt.last_norm is not None else 0}")


if __name__ == "__main__":
    main()
