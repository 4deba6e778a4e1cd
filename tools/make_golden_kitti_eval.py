"""Mints tests/golden/kitti_eval.npz from the REFERENCE's KITTI evaluator (data/datasets/kitti_eval.py), run on the CPU.

    python tools/make_golden_kitti_eval.py        # needs the reference checkout (oracle.ref_shim.import_reference)

The reference's rotated IoU is a numba.cuda kernel; oracle.ref_shim stubs numba so the decorated functions are plain Python.  Two
rebinds make its device geometry run on numpy: `cuda.local.array` allocates float32 arrays, and `rotate_iou_gpu_eval` becomes a double
loop over the reference's own `devRotateIoUEval(query_box, box, criterion)`, the operand order of `rotate_iou_kernel_eval`.  (The
reference's 16-float vertex list overflows for near-coincident boxes; the stub gives such lists room instead of an IndexError.)

A synthetic set with everything the evaluator branches on is written as KITTI text files (labels: 15 columns; detections: 16, the
layout `save_results` writes) and scored by the reference's `eval_from_scrach` for Car / Pedestrian / Cyclist in AP40 and AP11.  No det
overlaps a gt or a DontCare box within 1e-4 of a min-overlap (0.25, 0.3, 0.5, 0.7) in any metric, so fp32 rounding differences
between this emulation and the HIP kernels cannot flip a match.  The fixture holds data only: annos, overlaps, detail tables.
"""
from __future__ import annotations

import math
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kitti_eval.npz")
GT_CLASSES = ["Car"] * 8 + ["Pedestrian"] * 3 + ["Cyclist"] * 3 + ["Van", "Person_sitting", "Truck", "Misc", "Tram", "DontCare", "DontCare"]
DIMS = {"Car": (1.5, 1.6, 3.9), "Van": (2.2, 1.9, 5.0), "Truck": (3.2, 2.5, 9.0), "Tram": (3.5, 2.6, 15.0), "Misc": (1.5, 1.5, 2.5),
        "Pedestrian": (1.75, 0.65, 0.85), "Person_sitting": (1.3, 0.6, 0.9), "Cyclist": (1.75, 0.6, 1.75)}
MARGIN_AT = (0.25, 0.3, 0.5, 0.7)


def load_reference():
    R.import_reference()
    import ultralytics.data.datasets.kitti_eval as KE
    KE.numba.float32 = np.float32
    KE.cuda = types.SimpleNamespace(local=types.SimpleNamespace(array=lambda shape, dtype: np.zeros((48,) if tuple(shape) == (16,) else shape,
                                                                                                     np.float32)))

    def rotate_iou_cpu(boxes, query_boxes, criterion=-1, device_id=0):
        b, q = boxes.astype(np.float32), query_boxes.astype(np.float32)
        iou = np.zeros((b.shape[0], q.shape[0]), dtype=np.float32)
        for n in range(b.shape[0]):
            for k in range(q.shape[0]):
                iou[n, k] = KE.devRotateIoUEval(q[k], b[n], criterion)
        return iou.astype(boxes.dtype)

    KE.rotate_iou_gpu_eval = rotate_iou_cpu
    return KE


def fmt(v):
    return f"{v:.2f}"


def gt_line(rng, name):
    if name == "DontCare":
        x1, y1 = rng.uniform(0, 1100), rng.uniform(120, 250)
        return f"DontCare -1 -1 -10 {fmt(x1)} {fmt(y1)} {fmt(x1 + rng.uniform(20, 120))} {fmt(y1 + rng.uniform(15, 60))} -1 -1 -1 -1000 -1000 -1000 -10"
    h, w, l = (d * rng.uniform(0.9, 1.1) for d in DIMS[name])
    x, y, z = rng.uniform(-15, 15), rng.uniform(1.0, 2.5), rng.uniform(5, 50)
    ry = [0.0, math.pi / 2, -math.pi / 2, rng.uniform(-math.pi, math.pi)][rng.integers(4)]
    x1, y1 = rng.uniform(0, 1100), float(rng.integers(100, 250))
    bh = [25.0, 40.0, float(rng.integers(15, 150)), rng.uniform(15, 150)][rng.integers(4)]
    occ = int(rng.choice(4, p=[0.45, 0.25, 0.2, 0.1]))
    trunc = float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6, 0.8], p=[0.4, 0.2, 0.15, 0.1, 0.1, 0.05]))
    alpha = rng.uniform(-math.pi, math.pi)
    vals = [trunc, occ, alpha, x1, y1, x1 + rng.uniform(20, 200), y1 + bh, h, w, l, x, y, z, ry]
    return " ".join([name, fmt(trunc), str(occ)] + [fmt(v) for v in vals[2:]])


def det_line(rng, src):
    """a perturbed copy of gt line `src`, or (src None) a random false positive"""
    if src is None:
        name = ["Car", "Pedestrian", "Cyclist"][rng.integers(3)]
        src = gt_line(rng, name).split()
    else:
        src = src.split()
        name = src[0] if rng.random() > 0.1 else ["Car", "Pedestrian", "Cyclist", "Van"][rng.integers(4)]
    v = [float(s) for s in src[3:15]]
    alpha, (x1, y1, x2, y2), (h, w, l), (x, y, z), ry = v[0], v[1:5], v[5:8], v[8:11], v[11]
    j = lambda s: rng.normal(0, s)
    x1, x2 = x1 + j(2), x2 + j(2)
    if rng.random() < 0.15:  # det heights exactly at the MIN_HEIGHT edges
        y1 = float(round(y1))
        y2 = y1 + [25.0, 40.0][rng.integers(2)]
    else:
        y1, y2 = y1 + j(1.5), y2 + j(1.5)
    h, w, l = h * (1 + j(0.03)), w * (1 + j(0.03)), l * (1 + j(0.03))
    x, y, z, ry, alpha = x + j(0.06), y + j(0.05), z + j(0.12), ry + j(0.05), alpha + j(0.3)
    score = float(rng.integers(5, 100)) / 100
    return " ".join([name, "0.0", "0"] + [fmt(t) for t in (alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score)])


def parse(lines, ncol):
    t = np.array(" ".join(lines).split(), dtype=str).reshape(-1, ncol)
    f = lambda c: t[:, c].astype(np.float32)
    a = {"name": t[:, 0], "truncated": f(1), "occluded": f(2), "alpha": f(3), "bbox": f(slice(4, 8)), "dimensions": f([10, 8, 9]),
         "location": f(slice(11, 14)), "rotation_y": f(14)}
    if ncol == 16:
        a["score"] = f(15)
    return a


def near_margin(KE, gt, dt):
    """(n_dt,) bool: the det overlaps some gt (3 metrics) or DontCare box (criterion 0) within 1e-4 of a min-overlap"""
    nd, ng = len(dt["name"]), len(gt["name"])
    bad = np.zeros(nd, bool)
    if nd == 0 or ng == 0:
        return bad
    box3d = lambda a: np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], 1)
    bev = lambda a: box3d(a)[:, [0, 2, 3, 5, 6]]
    ovs = [KE.image_box_overlap(dt["bbox"], gt["bbox"]), KE.bev_box_overlap(bev(dt), bev(gt)).astype(np.float64),
           KE.box3d_overlap(box3d(dt), box3d(gt), z_axis=1, z_center=1.0).astype(np.float64)]
    dc = gt["bbox"][gt["name"] == "DontCare"].astype(np.float64)
    if dc.shape[0]:
        ovs.append(KE.image_box_overlap(dt["bbox"], dc, 0))
    for o in ovs:
        o = np.asarray(o, np.float64)
        for m in MARGIN_AT:
            bad |= (np.abs(o - m) < 1e-4).any(1)
    return bad


def synth(KE, rng, n_img):
    gts, dets = [], []
    for i in range(n_img):
        ng = 0 if i % 11 == 3 else int(rng.integers(1, 9))
        g = [gt_line(rng, GT_CLASSES[rng.integers(len(GT_CLASSES))]) for _ in range(ng)]
        real = [s for s in g if not s.startswith("DontCare")]
        srcs = [] if i % 13 == 5 else [s for s in real if rng.random() < 0.85] + [s for s in real if rng.random() < 0.15]
        srcs += [None] * (0 if i % 13 == 5 else int(rng.integers(0, 4)))
        d = [det_line(rng, s) for s in srcs]
        for _ in range(200):
            bad = near_margin(KE, parse(g, 15), parse(d, 16)) if d else np.zeros(0, bool)
            if not bad.any():
                break
            d = [det_line(rng, srcs[k]) if bad[k] else d[k] for k in range(len(d))]
        else:
            raise RuntimeError(f"image {i}: no det set clear of the margins")
        gts.append(g)
        dets.append(d)
    return gts, dets


def write_dir(root, gts, dets, names):
    gd, dd = os.path.join(root, "label_2"), os.path.join(root, "preds")
    os.makedirs(gd, exist_ok=True)
    os.makedirs(dd, exist_ok=True)
    for f, g, d in zip(names, gts, dets):
        open(os.path.join(gd, f), "w").write("".join(s + "\n" for s in g))
        open(os.path.join(dd, f), "w").write("".join(s + "\n" for s in d))
    return gd, dd


def pack_annos(prefix, annos):
    out = {f"{prefix}n": np.array([len(a["name"]) for a in annos], np.int64)}
    for k in annos[0]:
        out[prefix + k] = np.concatenate([a[k] for a in annos], 0)
    return out


def main():
    KE = load_reference()
    rng = np.random.default_rng(20261015)
    n_img = 96
    gts, dets = synth(KE, rng, n_img)
    names = [f"{i:06d}.txt" for i in range(n_img)]
    gt_annos, dt_annos = [parse(g, 15) for g in gts], [parse(d, 16) for d in dets]
    out = {}
    out.update(pack_annos("gt_", gt_annos))
    out.update(pack_annos("dt_", dt_annos))
    for metric in range(3):
        ovs = KE.calculate_iou_partly(dt_annos, gt_annos, metric, 50, z_axis=1, z_center=1.0)[0]
        out[f"ov{metric}"] = np.concatenate([np.asarray(o, np.float32).reshape(-1) for o in ovs])
    with tempfile.TemporaryDirectory() as tmp:
        gd, dd = write_dir(tmp, gts, dets, names)
        for mode in (40, 11):
            for cls in ("Car", "Pedestrian", "Cyclist"):
                det = KE.eval_from_scrach(gd, dd, [cls], ap_mode=mode)
                for k, v in det.items():
                    out[f"detail{mode}|{cls}|{k}"] = np.asarray(v, np.float64)
        # 7 images alone make empty parts in the reference (get_split_parts); 43 images without gts or dets add nothing to tp, fp, fn
        sub = os.path.join(tmp, "sub")
        gd, dd = write_dir(sub, gts[:7] + [[]] * 43, dets[:7] + [[]] * 43, names[:7] + [f"{i:06d}.txt" for i in range(900, 943)])
        det = KE.eval_from_scrach(gd, dd, ["Car"], ap_mode=40)
        for k, v in det.items():
            out[f"subset40|Car|{k}"] = np.asarray(v, np.float64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {n_img} images, {len(out['gt_name'])} gts, {len(out['dt_name'])} dets")


if __name__ == "__main__":
    main()
