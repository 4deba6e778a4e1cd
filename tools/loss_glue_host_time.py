"""Host time of one `DetectLoss3d` call on the bench model (results: profiles/loss_glue_refactor_ab.txt): S-3D, B = 32,
640 x 640, bf16, the predictions of one training forward kept and the criterion called on them over and over.  Timed is the host side
of a call - until its last launch is enqueued: 30 warm-up calls, then 12 blocks of 30 calls with no synchronisation inside a block and
one between blocks.  Prints the median, mean and range of the 12 block means in us per call, and the last call's items.

    python tools/loss_glue_host_time.py [LABEL]

To compare two versions of loss.py, run it in a fresh process per version, alternating, from the root of each tree."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (synth_batch)
import yolov10_3d_amd as y3d  # noqa: E402


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "tree"
    assert torch.cuda.is_available(), "needs a HIP device"
    y3d.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    model = y3d.YOLOv10_3DDetectionModel("yolov10s_3D.yaml").to("cuda").train()
    model.model[-1].restack()
    batch = bench.synth_batch(32, 640, 640, 100, "cuda")
    preds = model.predict(batch["img"])
    crit = model.init_criterion()
    assert type(crit).__name__ == "DetectLoss3d" and "_y3d_maps" in preds
    for _ in range(30):
        loss, items = crit(preds, batch)
    torch.cuda.synchronize()
    per = []
    for _ in range(12):
        t0 = time.perf_counter()
        for _ in range(30):
            loss, items = crit(preds, batch)
        per.append(1e6 * (time.perf_counter() - t0) / 30)
        torch.cuda.synchronize()
    print(f"{label} DetectLoss3d host us per call: median {statistics.median(per):.1f} mean {statistics.mean(per):.1f} min {min(per):.1f} "
          f"max {max(per):.1f} (12 blocks of 30 calls); items {[round(float(v), 4) for v in items]}", flush=True)


if __name__ == "__main__":
    main()
