"""Mints tests/golden/kitti_labels.npz from the REFERENCE's `KITTIDataset.__getitem__` + `collate_fn` (data/datasets/kitti.py), run
on the CPU.

    python tools/make_golden_kitti_labels.py      # needs the reference checkout (oracle.ref_shim.import_reference)

A synthetic KITTI tree (12 frames at real KITTI sizes, three calibration groups, one per size) is written to a temp dir: PNGs whose
pixels are `frame_pixels(i, W, H)` (a test regenerates them), calibration files and labels covering every class (Van, Misc, Truck,
DontCare included), the truncation / occlusion / box-height levels, objects behind the camera, outside the crop and beyond
max_depth, a 55-line frame (the max_objs cap) and a frame where nothing survives.  Four argument sets (defaults, cam_dis, val mode,
no mixup) are each run over a seeded sequence of items, the way a `workers=0` DataLoader draws them; the script records the random
decisions of every sample, the flipped P2, and the reference-collated batch in the reference's own dtypes.

OpenCV is absent: `cv2.getAffineTransform` is supplied as the exact float64 three-point solve for the duration of the run.  Every
object a sample looks at is kept 1e-4 away from the depth thresholds, from the pixel bounds of its projected 3D centre and from the
heading-bin edges (asserted; offending label lines are redrawn), so fp64 rounding differences cannot flip a decision.  The fixture
holds data only: label / calib text, draws, the reference's outputs.
"""
from __future__ import annotations

import math
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402
from kitti_labels_tree import frame_pixels  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kitti_labels.npz")
MARGIN = 1e-4
RES = (1280, 384)
# three calibration groups, one per KITTI frame size: (W, H, fu, cu, fv, cv, P03, P13, P23)
GROUPS = [(1242, 375, 721.5377, 609.5593, 721.5377, 172.854, 44.85728, 0.2163791, 0.002745884),
          (1224, 370, 707.0493, 604.0814, 707.0493, 180.5066, 45.75831, -0.3454157, 0.004981016),
          (1238, 374, 718.3351, 600.3891, 718.3351, 181.5122, 44.50382, 0.1371122, 0.003013617)]
FRAME_GROUP = [0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
N_LINES = [6, 9, 55, 4, 12, 5, 8, 30, 7, 10, 3, 14]
EMPTY_FRAME = 5  # no line of this frame survives the filters
DIMS = {"Car": (1.52, 1.63, 3.88), "Van": (2.2, 1.9, 5.0), "Truck": (3.2, 2.5, 9.0), "Misc": (1.5, 1.5, 2.5),
        "Pedestrian": (1.76, 0.66, 0.84), "Cyclist": (1.74, 0.6, 1.76)}
CLASSES = ["Car"] * 6 + ["Pedestrian"] * 2 + ["Cyclist"] * 2 + ["Van", "Misc", "Truck", "DontCare"]
ARGSETS = {  # name -> (dataset mode, argument overrides, seed, items)
    "default": ("train", dict(), 101, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 0, 4, 9]),
    "camdis": ("train", dict(cam_dis=True), 202, [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]),
    "val": ("val", dict(), 303, [0, 2, 5, 6, 7, 9, 11, 1]),
    "nomix": ("train", dict(mixup=0.0), 404, [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]),
}
PERBOX = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx")


def calib_text(g):
    W, H, fu, cu, fv, cv, p03, p13, p23 = GROUPS[g]
    p2 = f"{fu:e} 0.000000e+00 {cu:e} {p03:e} 0.000000e+00 {fv:e} {cv:e} {p13:e} 0.000000e+00 0.000000e+00 1.000000e+00 {p23:e}"
    r0 = "1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00"
    tr = "0.000000e+00 -1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 -1.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00"
    return f"P0: {p2}\nP1: {p2}\nP2: {p2}\nP3: {p2}\nR0_rect: {r0}\nTr_velo_to_cam: {tr}\nTr_imu_to_velo: {tr}\n"


def label_line(rng, g, empty=False):
    W, H, fu, cu, fv, cv = GROUPS[g][:6]
    name = CLASSES[rng.integers(len(CLASSES))]
    if empty and name in ("Car", "Pedestrian", "Cyclist"):
        name = ["Van", "Misc", "DontCare", name][rng.integers(4)]
    f = lambda v: f"{v:.2f}"
    if name == "DontCare":
        x1, y1 = rng.uniform(0, W - 80), rng.uniform(100, 250)
        return f"DontCare -1 -1 -10 {f(x1)} {f(y1)} {f(x1 + rng.uniform(10, 70))} {f(y1 + rng.uniform(10, 40))} -1 -1 -1 -1000 -1000 -1000 -10"
    kind = rng.choice(["near", "behind", "far", "beyond", "outside"], p=[0.68, 0.07, 0.1, 0.07, 0.08])
    z = {"near": rng.uniform(4, 60), "behind": rng.uniform(-8, 0.6), "far": rng.uniform(60, 110), "beyond": rng.uniform(100, 170),
         "outside": rng.uniform(6, 40)}[kind]
    h, w, l = (d * rng.uniform(0.9, 1.1) for d in DIMS[name])
    half = (W / 2) * abs(z) / fu
    x = rng.uniform(-0.75, 0.75) * half if kind != "outside" else rng.choice([-1, 1]) * rng.uniform(1.05, 1.6) * half
    y = rng.uniform(1.0, 2.2)
    zz = max(abs(z), 2.0)
    u, v = fu * x / zz + cu, fv * y / zz + cv
    bh = fv * h / zz if rng.random() < 0.7 else [20.0, 26.0, 30.0, 39.0, 45.0, 60.0][rng.integers(6)]
    if kind in ("far", "beyond") and rng.random() < 0.7:
        bh = rng.uniform(26, 60)  # tall enough to pass the level filter and reach the depth checks
    bw = fu * l / zz * 0.7 + 5
    x1, x2 = np.clip([u - bw / 2, u + bw / 2], 0, W - 1)
    y2 = min(v, H - 1.0)
    y1 = max(y2 - bh, 0.0)
    if x2 - x1 < 2:
        x1, x2 = max(x2 - 20, 0), min(x1 + 20, W - 1)
    trunc = float(rng.choice([0.0, 0.0, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.9]))
    occ = int(rng.choice(4, p=[0.45, 0.25, 0.2, 0.1]))
    ry = rng.uniform(-math.pi, math.pi)
    alpha = rng.uniform(-math.pi, math.pi)
    return " ".join([name, f(trunc), str(occ)] + [f(t) for t in (alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry)])


def write_tree(root, labels):
    for sub in ("training/image_2", "training/calib", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    from PIL import Image
    for i, g in enumerate(FRAME_GROUP):
        W, H = GROUPS[g][:2]
        p = os.path.join(root, "training/image_2", f"{i:06d}.png")
        if not os.path.exists(p):
            Image.fromarray(frame_pixels(i, W, H), "RGB").save(p)
        open(os.path.join(root, "training/calib", f"{i:06d}.txt"), "w").write(calib_text(g))
        open(os.path.join(root, "training/label_2", f"{i:06d}.txt"), "w").write("".join(s + "\n" for s in labels[i]))
    for split in ("train", "val"):
        open(os.path.join(root, "ImageSets", f"{split}.txt"), "w").write("".join(f"{i:06d}\n" for i in range(len(FRAME_GROUP))))


def affine_from_points(src, dst):
    """cv2.getAffineTransform: the exact 2x3 map through three point pairs, in float64"""
    A = np.hstack((np.asarray(src, np.float64), np.ones((3, 1))))
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T.copy()


def install_hooks(K, KU, rec):
    """record the random draws, the crop matrices and the flipped P2 of every __getitem__ call"""
    cv2 = sys.modules["cv2"]
    cv2.getAffineTransform = affine_from_points
    K.cv2 = KU.cv2 = cv2
    npr = np.random
    for name in ("random", "randn", "randint"):
        orig = getattr(npr, name)

        def wrap(*a, _orig=orig, _name=name, **k):
            v = _orig(*a, **k)
            rec["draws"].append((_name, v))
            return v

        setattr(K.np.random, name, wrap)
    orig_gat = K.get_affine_transform

    def gat(center, scale, rot, out, inv=0):
        r = orig_gat(center, scale, rot, out, inv=inv)
        rec["affine"] = (np.array(center, np.float64), np.array(scale, np.float64), r[0].copy(), r[1].copy())
        return r

    K.get_affine_transform = gat
    orig_flip = KU.Calibration.flip

    def flip(self, img_size):
        orig_flip(self, img_size)
        rec["flipP2"] = np.array(self.P2, np.float32)

    KU.Calibration.flip = flip


def parsed_records(KU, root):
    out = {"rec_n": [], "rec_cls": [], "rec_level": [], "rec_box": [], "rec_pos": [], "rec_f64": []}
    for i in range(len(FRAME_GROUP)):
        objs = KU.get_objects_from_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
        out["rec_n"].append(len(objs))
        for o in objs:
            out["rec_cls"].append(o.cls_type)
            out["rec_level"].append(o.level_str)
            assert o.box2d.dtype == np.float32 and o.pos.dtype == np.float32
            out["rec_box"].append(o.box2d)
            out["rec_pos"].append(o.pos)
            out["rec_f64"].append(np.array([o.trucation, o.occlusion, o.alpha, o.h, o.w, o.l, o.ry], np.float64))
    return {k: np.array(v) for k, v in out.items()}


def margin_violations(KU, root, labels, samples):
    """(frame, line) pairs whose decisions lie within MARGIN of an edge in some recorded sample"""
    bad = set()
    apc = 2 * np.pi / 12
    for s in samples:
        for frame, is_partner in ((s["item"], False), (s["partner"], True)):
            if frame < 0:
                continue
            W = GROUPS[FRAME_GROUP[s["item"]]][0]
            P2 = s["P2"].astype(np.float64)
            objs = KU.get_objects_from_label(os.path.join(root, "training/label_2", f"{frame:06d}.txt"))
            ncap = min(len(labels[s["item"]]), 50)
            cand = range(min(len(objs), 50 - ncap) if is_partner else ncap)
            for i in cand:
                o = objs[i]
                if o.cls_type not in ("Car", "Pedestrian", "Cyclist") or o.trucation > 0.5 or o.occlusion > 2:
                    continue
                box, pos, ry = o.box2d.astype(np.float64), o.pos.astype(np.float64), o.ry
                if s["flip"]:
                    box[0], box[2] = np.float32(W - box[2]), np.float32(W - box[0])
                    pos[0] = -pos[0]
                    ry = np.pi - ry
                    ry = ry - 2 * np.pi if ry > np.pi else ry + 2 * np.pi if ry < -np.pi else ry
                zs = pos[2] * s["scale"]
                if min(abs(zs - s["min_depth"]), abs(zs - s["max_depth"])) < MARGIN:
                    bad.add((frame, i))
                if o.level_str == "UnKnown" or zs < s["min_depth"]:
                    continue
                c = pos + np.array([0, -o.h / 2, 0])
                uv = (P2[:2, :3] @ c + P2[:2, 3]) / c[2]
                p = s["trans"] @ np.array([np.float32(uv[0]), np.float32(uv[1]), 1.0])
                if min(abs(p[0] + 1), abs(p[0] - RES[0]), abs(p[1] + 1), abs(p[1] - RES[1])) < MARGIN:
                    bad.add((frame, i))
                ub = (np.float32(box[0]) + np.float32(box[2])) / np.float32(2)
                a = ry - math.atan2(float(ub) - P2[0, 2], P2[0, 0])
                for edge in (np.pi, -np.pi, 3 * np.pi, -3 * np.pi):
                    if abs(a - edge) < MARGIN:
                        bad.add((frame, i))
                a = a - 2 * np.pi if a > np.pi else a + 2 * np.pi if a < -np.pi else a
                sh = (a % (2 * np.pi) + apc / 2) % (2 * np.pi)
                if abs(sh / apc - round(sh / apc)) * apc < MARGIN or abs(sh - 2 * np.pi) < MARGIN:
                    bad.add((frame, i))
    return bad


def run(K, KU, root, rec, labels):
    """every argument set over its items -> (per-sample draw records, {argset: collated batch})"""
    samples, batches = [], {}
    for name, (mode, over, seed, items) in ARGSETS.items():
        args = R.model_args(seed=0, load_depth_maps=False, **over)
        split = os.path.join(root, "ImageSets", f"{'val' if mode == 'val' else 'train'}.txt")
        ds = K.KITTIDataset(split, mode, args)
        np.random.seed(seed)
        outs = []
        for item in items:
            rec.update(draws=[], affine=None, flipP2=None)
            opened = []
            orig_get = ds.get_image
            ds.get_image = lambda idx, _o=orig_get: (opened.append(int(idx)), _o(idx))[1]
            out = ds[item]
            ds.get_image = orig_get
            rnd = [v for n, v in rec["draws"] if n == "random"]
            rn = [v for n, v in rec["draws"] if n == "randn"]
            mixed = int(out["mixed"])
            flip = rec["flipP2"] is not None
            crop = len(rn) > 0
            center, crop_size, trans, trans_inv = rec["affine"]
            img_size = np.array(out["info"]["img_size"])
            scale = float(np.clip(rn[0] * (args.max_scale - args.min_scale) / 2 + (args.max_scale + args.min_scale) / 2,
                                  args.min_scale, args.max_scale)) if crop else 1.0
            assert np.array_equal(crop_size, img_size * scale if crop else img_size)
            assert flip == (mode == "train" and rnd[1] < args.fliplr)
            P2 = rec["flipP2"] if flip else KU.Calibration(os.path.join(root, "training/calib", f"{item:06d}.txt")).P2
            samples.append(dict(argset=name, item=item, mixed=mixed, flip=int(flip), crop=int(crop), scale=scale, center=center,
                                partner=opened[-1] if mixed else -1, trans=trans, trans_inv=trans_inv, P2=np.asarray(P2, np.float32),
                                min_depth=args.min_depth_threshold, max_depth=args.max_depth_threshold, n_draws=len(rec["draws"])))
            outs.append(out)
        batches[name] = K.KITTIDataset.collate_fn(outs)
    return samples, batches


def main():
    R.import_reference()
    from ultralytics.data.datasets import kitti as K
    from ultralytics.data.datasets import kitti_utils as KU
    rec = {}
    install_hooks(K, KU, rec)
    rng = np.random.default_rng(20261016)
    labels = [[label_line(rng, FRAME_GROUP[i], empty=(i == EMPTY_FRAME)) for _ in range(N_LINES[i])] for i in range(len(FRAME_GROUP))]
    root = tempfile.mkdtemp(prefix="y3d_kitti_labels_")
    try:
        for attempt in range(40):
            write_tree(root, labels)
            samples, batches = run(K, KU, root, rec, labels)
            bad = margin_violations(KU, root, labels, samples)
            if not bad:
                break
            for frame, i in sorted(bad):
                labels[frame][i] = label_line(rng, FRAME_GROUP[frame], empty=(frame == EMPTY_FRAME))
        else:
            raise RuntimeError("no label set clear of the decision margins")
        assert not margin_violations(KU, root, labels, samples)
        out = {"label_text": np.array(["".join(s + "\n" for s in lab) for lab in labels]),
               "calib_text": np.array([calib_text(g) for g in FRAME_GROUP]),
               "frame_wh": np.array([GROUPS[g][:2] for g in FRAME_GROUP], np.int64),
               "resolution": np.array(RES, np.int64),
               "argsets": np.array(list(ARGSETS))}
        out.update(parsed_records(KU, root))
        # the flipped calibration of every frame, for flip_calib
        fl = []
        for i, g in enumerate(FRAME_GROUP):
            c = KU.Calibration(os.path.join(root, "training/calib", f"{i:06d}.txt"))
            c.flip(np.array(GROUPS[g][:2]))
            fl.append((np.asarray(c.P2, np.float32), np.array([c.cu, c.cv, c.fu, c.fv, c.tx, c.ty], np.float64)))
        out["flip_P2"] = np.stack([a for a, _ in fl])
        out["flip_c6"] = np.stack([b for _, b in fl])
        for name, (mode, over, seed, items) in ARGSETS.items():
            ss = [s for s in samples if s["argset"] == name]
            out[f"{name}/mode"] = np.array(mode)
            out[f"{name}/cam_dis"] = np.array(int(bool(over.get("cam_dis", False))))
            out[f"{name}/mixup"] = np.array(float(over.get("mixup", R.model_args().mixup)))
            out[f"{name}/seed"] = np.array(seed)
            out[f"{name}/items"] = np.array(items, np.int64)
            for k in ("mixed", "flip", "crop", "partner"):
                out[f"{name}/{k}"] = np.array([s[k] for s in ss], np.int64)
            out[f"{name}/scale"] = np.array([s["scale"] for s in ss], np.float64)
            for k in ("center", "trans", "trans_inv", "P2"):
                out[f"{name}/{k}"] = np.stack([s[k] for s in ss])
            b = batches[name]
            for k in PERBOX + ("calib", "ratio_pad", "mixed"):
                out[f"{name}/c/{k}"] = b[k].numpy()
        kept = sum(int(np.asarray(batches[n]["batch_idx"]).shape[0]) for n in ARGSETS)
        combos = sorted({(s["mixed"], s["flip"], s["crop"]) for s in samples})
        np.savez_compressed(OUT, **out)
        print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(samples)} samples, {kept} boxes kept, (mixed, flip, crop) {combos}, "
              f"partner tries rejected somewhere: {any(s['n_draws'] > 4 + 3 * s['crop'] for s in samples)}")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
