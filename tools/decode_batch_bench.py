"""Times the label decode (`y3d_decode_labels`, csrc/decode_labels.hip) at B = 32 in both layouts of the batch builders, and today's only
other route to label corners on the same frames, in the same run.  One JSON line on stdout, the same line and a table in
profiles/decode_batch_bench.txt.  No target is claimed: the launch is latency-bound (32 single-wave workgroups).

  * launch, static / ragged:  `kitti.decode_labels` with every argument on the device already (what a graph captures): rows, corners3d,
    corners_img and counts, one launch, HIP events, median of --iters calls;
  * wrapper, static / ragged:  `kitti.decode_batch_device` on a batch dictionary: the same launch behind the uploads of ori_shape, the six
    calibration constants, trans_inv and P2, and the casts of the per-box tensors (wall clock around a synchronised call);
  * files:  `kitti_eval.read_label_file` + `plot.corners3d_of` per frame + `plot.pack_boxes` (one upload) on label files that hold the
    same boxes (wall clock): corners only (from float32 fields), no rows, no projection, and only for datasets that have such files.

The batch is the `synth` recipe of tests/decode_batch_ref.py with 0 .. 50 boxes per image.

    python tools/decode_batch_bench.py [--batch 32] [--iters 200] [--out profiles/decode_batch_bench.txt]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import decode_batch_ref as D  # noqa: E402

from yolov10_3d_amd import kitti, kitti_eval, plot  # noqa: E402

DEV = "cuda"
NAMES = ("Car", "Pedestrian", "Cyclist")


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


def wall_ms(fn, iters):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    return {"median": round(ms[len(ms) // 2], 4), "p10": round(ms[len(ms) // 10], 4), "p90": round(ms[(len(ms) * 9) // 10], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_batch_bench.txt"))
    a = ap.parse_args()
    B = a.batch
    counts = [int(v) for v in np.random.default_rng(B).integers(0, 51, B)]
    lab, ori, c6, P2, rp, inv = D.synth(counts, 32)
    static, cnt = D.to_static(lab, B, 50)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    shared = [dev(ori), dev(c6), dev(rp), dev(inv), dev(P2), dev(np.asarray(kitti.CLS_MEAN_SIZE))]
    rag_t, st_t, cnt_t = {k: dev(v) for k, v in lab.items()}, {k: dev(v) for k, v in static.items()}, dev(cnt)
    outs = {True: kitti.decode_labels(st_t, cnt_t, *shared, True, False, 50), False: kitti.decode_labels(rag_t, None, *shared, True, False, 50)}
    for x, y in zip(outs[True], outs[False]):
        assert torch.equal(x, y), "the two layouts disagree"
    assert outs[True][3].tolist() == counts

    def batch_of(t, c):
        b = dict(t, ori_shape=[np.array(o) for o in ori], ratio_pad=shared[2], info=[{"trans_inv": m} for m in inv],
                 im_file=[f"{i:06d}.txt" for i in range(B)])
        if c is not None:
            b["counts"] = c
        return b

    calibs = [tuple(c) for c in c6]
    res = {"bench": "decode_labels", "batch": B, "boxes": int(sum(counts)), "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "launch_static_ms": device_ms(lambda: kitti.decode_labels(st_t, cnt_t, *shared, True, False, 50, out=outs[True]), a.iters),
           "launch_ragged_ms": device_ms(lambda: kitti.decode_labels(rag_t, None, *shared, True, False, 50, out=outs[False]), a.iters),
           "wrapper_static_ms": wall_ms(lambda: kitti.decode_batch_device(batch_of(st_t, cnt_t), calibs, P2), a.iters),
           "wrapper_ragged_ms": wall_ms(lambda: kitti.decode_batch_device(batch_of(rag_t, None), calibs, P2), a.iters)}

    rows = outs[True][0].cpu().numpy()
    with tempfile.TemporaryDirectory(prefix="y3d_decode_batch_bench_") as tmp:
        for b in range(B):  # the same boxes as label files (15 columns, full precision)
            with open(os.path.join(tmp, f"{b:06d}.txt"), "w") as f:
                for r in rows[b, :counts[b]]:
                    f.write(" ".join([NAMES[int(r[0])], "0.0", "0", repr(float(r[1]))] + [repr(float(v)) for v in r[2:13]]) + "\n")

        def files():
            per = [plot.corners3d_of(kitti_eval.read_label_file(os.path.join(tmp, f"{b:06d}.txt"))) if counts[b] else np.zeros((0, 8, 3)) for b in range(B)]
            return plot.pack_boxes(per, DEV)

        c3, n = files()
        assert n.tolist() == counts
        # read_label_file parses to float32, as the reference's evaluator does: the same boxes within that rounding
        np.testing.assert_allclose(c3.cpu().numpy(), outs[True][1][:, :c3.shape[1]].cpu().numpy(), rtol=0, atol=1e-4)
        res["files_ms"] = wall_ms(files, max(20, a.iters // 4))

    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(f"y3d_decode_labels at B = {B}, {res['boxes']} boxes (0 .. 50 per image), ms per call: median (p10 .. p90)\n\n")
        for key, what in (("launch_static_ms", "launch, static layout (HIP events, arguments on the device)"),
                          ("launch_ragged_ms", "launch, ragged layout (HIP events, arguments on the device)"),
                          ("wrapper_static_ms", "decode_batch_device on a batch dictionary, static (wall clock, with its uploads)"),
                          ("wrapper_ragged_ms", "decode_batch_device on a batch dictionary, ragged (wall clock, with its uploads)"),
                          ("files_ms", "read_label_file + corners3d_of + pack_boxes on the same boxes (wall clock; corners only)")):
            m = res[key]
            f.write(f"{what}: {m['median']} ({m['p10']} .. {m['p90']})\n")
        f.write("\n" + line + "\n")


if __name__ == "__main__":
    main()
