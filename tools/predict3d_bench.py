"""Times the 3D predictor's row pass (`y3d_predict3d_rows`, csrc/predict3d.hip) against the two-step path it replaces, in the same run:
B = 32, K = 50 (the validator's max_det) and K = 300, HIP events, medians of --iters calls.  One JSON line on stdout, the same line
and a table in profiles/predict3d_bench.txt.

  * new:  `predict.predict3d_rows` — decode, confidence filter, ordered compaction, corners and projections, one launch, no
    synchronisation (every argument already on the device);
  * old:  `kitti.decode_preds_device` followed by boolean-mask compaction in torch (`rows[keep]` and `keep.sum(1)`: the masked select
    waits for the device to learn its output size), with the inverse transforms as a batch carries them (host arrays, stacked and
    uploaded by every call, as its callers pay today);
  * old, resident:  the same with the inverse transforms and the mean-size table already on the device, as the new side has them.
    Neither old form computes corners: the reference builds those on the host, one Python object
    per box, which is not timed here.

The predictions are the `synth` recipe of tests/predict3d_ref.py; about half the rows pass conf = 0.25.  No target is claimed.

    python tools/predict3d_bench.py [--batch 32] [--iters 200] [--out profiles/predict3d_bench.txt]
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

from yolov10_3d_amd import kitti, predict  # noqa: E402

DEV = "cuda"
CONF = 0.25


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


def case(B, K, iters):
    preds = PR.synth(torch.Generator().manual_seed(K), B, K).to(DEV)
    cam = PR.synth_camera(B)
    calib6, P2, ratio, inv = (torch.from_numpy(a).to(DEV) for a in cam)
    P2 = P2.double()
    inv_host = list(cam[3])  # as a batch carries them (info["trans_inv"]): decode_preds_device stacks and uploads them per call

    def new():
        return predict.predict3d_rows(preds, calib6, P2, ratio, inv, CONF)

    def old():
        rows, keep = kitti.decode_preds_device(preds, calib6, ratio, inv_host, threshold=CONF)
        return rows[keep], keep.sum(1)

    ms = torch.tensor(kitti.CLS_MEAN_SIZE, dtype=torch.float64).to(DEV)

    def old_resident():  # everything on the device already, as the new side has it: kernel against kernel + torch's compaction
        rows, keep = kitti.decode_preds_device(preds, calib6, ratio, inv, threshold=CONF, cls_mean_size=ms)
        return rows[keep], keep.sum(1)

    counts = new()[3]
    for fn in (old, old_resident):
        flat, n = fn()
        assert torch.equal(counts.long(), n) and flat.shape[0] == int(n.sum())
    return {"rows": [B, K], "kept": int(n.sum()), "new_ms": device_ms(new, iters), "old_ms": device_ms(old, iters),
            "old_resident_ms": device_ms(old_resident, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict3d_bench.txt"))
    a = ap.parse_args()
    out = {"bench": "predict3d_rows", "batch": a.batch, "conf": CONF, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "cases": [case(a.batch, K, a.iters) for K in (50, 300)]}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write("predict3d_rows (one launch: decode + filter + compaction + corners + projection) against decode_preds_device + torch\n"
                "boolean-mask compaction (no corners), HIP events, ms per call: median (p10 .. p90)\n\n")
        for c in out["cases"]:
            n, o, r = c["new_ms"], c["old_ms"], c["old_resident_ms"]
            f.write(f"B = {c['rows'][0]}, K = {c['rows'][1]}, {c['kept']} rows kept at conf {CONF}: new {n['median']} ({n['p10']} .. {n['p90']}), "
                    f"old {o['median']} ({o['p10']} .. {o['p90']}), old with device-resident arguments {r['median']} ({r['p10']} .. {r['p90']})\n")
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
