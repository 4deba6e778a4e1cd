"""Mints tests/golden/yolo2d_labels.npz from the REFERENCE's 2D sample pipeline, run on the CPU.

    python tools/make_golden_yolo2d.py [--cv2]     # needs the reference checkout (oracle.ref_shim.import_reference)

The reference's own `Mosaic`, `MixUp`, `RandomPerspective`, `RandomHSV`, `RandomFlip` and `Format` are composed by its
`v8_transforms` / `YOLODataset.build_transforms`, and its `collate_fn` collates each argument set.  The dataset is a `YOLODataset`
instance created without `__init__` (which would scan and cache labels with a thread pool) and given the attributes `__init__` sets, so
`load_image`, `get_image_and_label`, `update_labels_info` and with them the mosaic buffer logic are the reference's own, not a
restatement.  The tree (tests/yolo2d_tree.py) has twelve frames of up to 100 px: landscape, portrait, square, smaller and larger than
imgsz = 64, one without boxes, seven with 25-40 boxes.

OpenCV, torchvision and albumentations are absent here.  For the duration of the run the `cv2` stub gets these stand-ins:
  * `getRotationMatrix2D`: its closed form, exact;
  * `imread`: PIL's decode, channels reversed to BGR (exact for PNG);
  * `resize`, `warpAffine`, `copyMakeBorder`, `cvtColor`, `split`, `merge`, `LUT`: SHAPES only — the labels never read a pixel; the
    images they return are not the reference's and are not recorded.
The reference's data/dataset.py calls `torch.stack` / `torch.cat` in `collate_fn` without importing torch; the module is handed the name.
Without albumentations the reference's `Albumentations` transform only normalises the boxes, as in the reference's own runs without it.

Every draw of `random` / `np.random` the reference makes is recorded through wrappers and compared, one by one and with ==, against
`yolo2d.sample_augment` replayed from the same seeds; the reference's M (returned by `affine_transform`) is recorded and compared too.
Asserted: each filter (zero area after the canvas clip, wh_thr, area_thr, ar_thr) both drops and keeps something; every decision lies
1e-4 from its edge (offending label rows are redrawn); some sample exceeds 64 rows and some exceeds 128.  The fixture holds data
only: label text, draws, matrices, the reference's collated outputs.

--cv2: where OpenCV can be imported, the run uses the real cv2 instead of the stand-ins and also records, per sample, the reference's
real image and its largest and mean absolute difference from tests/yolo2d_ref.py's arithmetic (keys `<set>/cv2/...`).  OpenCV is not
installed where this fixture was minted, so that switch has never been run and the distance is unmeasured.
"""
from __future__ import annotations

import json
import os
import random
import shutil
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_shim as R  # noqa: E402
import yolo2d_ref  # noqa: E402
import yolo2d_tree as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "yolo2d_labels.npz")
MARGIN = 1e-4
N_BOXES = [40, 40, 6, 0, 5, 40, 36, 32, 8, 30, 40, 40]
NC = 20


def label_row(rng):
    kind = rng.choice(["plain", "tiny", "thin", "edge", "big"], p=[0.7, 0.08, 0.06, 0.1, 0.06])
    if kind == "plain":
        w, h = rng.uniform(0.1, 0.32, 2)
    elif kind == "tiny":  # a few pixels: the wh threshold
        w, h = rng.uniform(0.015, 0.06, 2)
    elif kind == "thin":  # aspect ratios around and beyond 100
        w, h = (rng.uniform(0.6, 0.98), rng.uniform(0.004, 0.012))
        if rng.random() < 0.5:
            w, h = h, w
    elif kind == "big":
        w, h = rng.uniform(0.5, 0.9, 2)
    else:  # hugging an image edge: cut by the mosaic window, the area threshold
        w, h = rng.uniform(0.1, 0.3, 2)
    x, y = rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2)
    if kind == "edge":
        if rng.random() < 0.5:
            x = [w / 2, 1 - w / 2][rng.integers(2)]
        else:
            y = [h / 2, 1 - h / 2][rng.integers(2)]
    return f"{rng.integers(NC)} {x:.6f} {y:.6f} {w:.6f} {h:.6f}"


def install_cv2(real):
    cv2 = sys.modules["cv2"]
    if real:
        return cv2
    from PIL import Image

    def rot(angle, center, scale):
        import math
        a = angle * math.pi / 180
        al, be = math.cos(a) * scale, math.sin(a) * scale
        return np.array([[al, be, (1 - al) * center[0] - be * center[1]], [-be, al, be * center[0] + (1 - al) * center[1]]], np.float64)

    cv2.getRotationMatrix2D = lambda angle=0, center=(0, 0), scale=1: rot(angle, center, scale)
    cv2.imread = lambda f, *a: np.ascontiguousarray(np.array(Image.open(f).convert("RGB"))[..., ::-1])
    cv2.resize = lambda im, dsize, interpolation=None: np.zeros((dsize[1], dsize[0], 3), np.uint8)
    cv2.warpAffine = lambda img, M, dsize=None, borderValue=None: np.zeros((dsize[1], dsize[0], 3), np.uint8)
    cv2.copyMakeBorder = lambda img, t, b, l, r, kind, value=None: np.pad(img, ((t, b), (l, r), (0, 0)), constant_values=114)
    cv2.cvtColor = lambda img, code, dst=None: img
    cv2.split = lambda img: [img[..., c] for c in range(img.shape[-1])]
    cv2.merge = lambda chans: np.stack(chans, -1)
    cv2.LUT = lambda ch, lut: lut[ch]
    return cv2


def hyp_for(over):
    from yolov10_3d_amd import yolo2d
    return SimpleNamespace(**dict(yolo2d.DATA_ARGS, mask_ratio=4, overlap_mask=True, **over))


def make_dataset(YOLODataset, split, hyp, augment):
    """a YOLODataset without __init__: the attributes BaseDataset.__init__ / YOLODataset.__init__ set, labels as cache_labels lists them"""
    ds = object.__new__(YOLODataset)
    ds.use_segments = ds.use_keypoints = ds.use_obb = False
    ds.data = {"names": {i: str(i) for i in range(NC)}}
    ds.imgsz, ds.augment, ds.rect, ds.single_cls, ds.prefix = split.imgsz, augment, False, False, ""
    ds.im_files = list(split.im_files)
    ds.labels = [dict(im_file=f, shape=split.size(i), cls=lb[:, 0:1].copy(), bboxes=lb[:, 1:].copy(), segments=[], keypoints=None, normalized=True,
                      bbox_format="xywh") for i, (f, lb) in enumerate(zip(split.im_files, split.labels))]
    ds.ni = len(ds.labels)
    ds.batch_size, ds.stride, ds.pad = split.batch, 32, 0.5
    ds.buffer = []
    ds.max_buffer_length = min((ds.ni, ds.batch_size * 8, 1000)) if augment else 0
    ds.ims, ds.im_hw0, ds.im_hw = [None] * ds.ni, [None] * ds.ni, [None] * ds.ni
    ds.npy_files = [Path(f).with_suffix(".npy") for f in ds.im_files]
    ds.transforms = ds.build_transforms(hyp=hyp)
    return ds


class Recorder:
    """wraps the generator functions the reference calls, for the duration of a `with` block"""

    def __init__(self, A):
        self.draws, self.Ms, self.A = [], [], A

    def __enter__(self):
        self.saved = [(random, n, getattr(random, n)) for n in ("uniform", "random", "choices", "randint")]
        self.saved += [(np.random, n, getattr(np.random, n)) for n in ("beta", "uniform")]
        for mod, n, fn in self.saved:
            tag = ("np." + n) if (mod is np.random and n == "uniform") else n

            def wrap(*a, _fn=fn, _tag=tag, **k):
                v = _fn(*a, **k)
                self.draws.append((_tag, [float(x) for x in v] if isinstance(v, (list, np.ndarray)) else float(v)))
                return v

            setattr(mod, n, wrap)
        self.orig_affine = self.A.RandomPerspective.affine_transform

        def affine(this, img, border, _o=self.orig_affine):
            img, M, s = _o(this, img, border)
            self.Ms.append(np.array(M, np.float32))
            return img, M, s

        self.A.RandomPerspective.affine_transform = affine
        return self

    def __exit__(self, *exc):
        for mod, n, fn in self.saved:
            setattr(mod, n, fn)
        self.A.RandomPerspective.affine_transform = self.orig_affine


def run(A, YOLODataset, img_dir, real_cv2):
    """every argument set over its items -> {set: (samples, reference per-sample outputs, collated batch, M verdicts, cv2 records)}"""
    from yolov10_3d_amd import yolo2d
    out = {}
    for name, (mode, over, seed, items) in T.ARGSETS.items():
        train = mode == "train"
        split_ref = yolo2d.Split(img_dir, T.IMGSZ, T.BATCH, augment=train)
        ds = make_dataset(YOLODataset, split_ref, hyp_for(over), train)
        random.seed(seed)
        np.random.seed(seed)
        refs, draws, Ms = [], [], []
        for item in items:
            with Recorder(A) as rec:
                refs.append(ds[item])
            draws.append(rec.draws)
            Ms.append(rec.Ms)
        batch = YOLODataset.collate_fn([dict(r) for r in refs])
        # the replay, from the same seeds
        split = yolo2d.Split(img_dir, T.IMGSZ, T.BATCH, augment=train)
        args = yolo2d.data_args(**over)
        random.seed(seed)
        np.random.seed(seed)
        samples, m_equal = [], []
        for n, item in enumerate(items):
            s = yolo2d.sample_augment(split, item, args, mode)
            mine = [(t, [float(x) for x in v] if isinstance(v, list) else float(v)) for t, v in T.flat_draws(s)]
            assert mine == draws[n], f"{name} sample {n}: draws differ\n{mine}\n{draws[n]}"
            pres = [p for p in (s["pre"], s["pre2"]) if p is not None and p["warp"]]
            assert len(pres) == len(Ms[n])
            for p, M in zip(pres, Ms[n]):
                ulp = np.abs(p["M"].view(np.int32).astype(np.int64) - M.view(np.int32).astype(np.int64)).max()
                assert ulp <= 1, f"{name} sample {n}: M differs by {ulp} ulp"
                m_equal.append(bool(ulp == 0))
                p["M"] = M  # the fixture records the reference's matrix
            assert n < len(items) - 1 or split.buffer == list(ds.buffer), (name, n, split.buffer, list(ds.buffer))
            samples.append(s)
        cv = None
        if real_cv2:
            imgs = T.images()
            cv = []
            for s, r in zip(samples, refs):
                ref_img = r["img"].numpy().transpose(1, 2, 0)
                d = np.abs(ref_img.astype(np.int64) - yolo2d_ref.image(s, imgs, T.IMGSZ).astype(np.int64))
                cv.append((ref_img, int(d.max()), float(d.mean())))
        out[name] = (samples, refs, batch, m_equal, cv)
    return out


def violations(results, rows):
    """(frame, row) pairs a decision of which lies within MARGIN of its edge, and the filter statistics"""
    bad, stat = set(), {k: [0, 0] for k in ("area", "wh", "ratio", "ar")}
    for name, (samples, refs, _, _, _) in results.items():
        for s, r in zip(samples, refs):
            cls, box, diag = yolo2d_ref.labels(s, rows, T.IMGSZ)
            n_ref = int(r["bboxes"].shape[0])
            assert len(box) == n_ref and np.array_equal(cls.reshape(-1), r["cls"].numpy().reshape(-1)), f"{name}: survivors differ from the reference"
            for d in diag:
                key = (d["frame"], d["row"])
                if d["verdicts"] is None:  # dropped by the zero-area filter
                    stat["area"][0] += 1
                    continue
                if d["area"] >= 0:
                    stat["area"][1] += 1
                    if d["area"] < MARGIN:
                        bad.add(key)
                v = d["verdicts"]
                stat["wh"][int(v[0] and v[1])] += 1
                stat["ratio"][int(v[2])] += 1
                stat["ar"][int(v[3])] += 1
                edges = (abs(d["w2"] - 2), abs(d["h2"] - 2), abs(d["ratio"] - 0.1), abs(d["ar"] - 100) if np.isfinite(d["ar"]) else 1.0)
                if min(edges) < MARGIN:
                    bad.add(key)
    return bad, stat


def main():
    real = "--cv2" in sys.argv
    if real:
        import cv2  # noqa: F401  (fails here: OpenCV is not installed)
    R.import_reference()
    from ultralytics.data import augment as A
    from ultralytics.data import dataset as D
    from ultralytics.data.dataset import YOLODataset
    import torch
    D.torch = torch  # the reference's data/dataset.py uses torch in collate_fn without importing it
    install_cv2(real)
    rng = np.random.default_rng(20261018)
    labels = [[label_row(rng) for _ in range(n)] for n in N_BOXES]
    root = tempfile.mkdtemp(prefix="y3d_yolo2d_")
    try:
        for attempt in range(40):
            text = ["".join(s + "\n" for s in lab) for lab in labels]
            shutil.rmtree(os.path.join(root, "labels"), ignore_errors=True)
            img_dir = T.write_tree(root, text)
            results = run(A, YOLODataset, img_dir, real)
            rows = T.label_rows({"label_text": np.array(text)})
            bad, stat = violations(results, rows)
            if not bad:
                break
            for frame, i in sorted(bad):
                labels[frame][i] = label_row(rng)
        else:
            raise RuntimeError("no label set clear of the decision margins")
        assert all(lo > 0 and hi > 0 for lo, hi in stat.values()), f"a filter never drops or never keeps: {stat}"
        out = {"label_text": np.array(text), "frame_wh": np.array(T.FRAME_WH, np.int64), "imgsz": np.array(T.IMGSZ), "batch": np.array(T.BATCH),
               "argsets": np.array(list(T.ARGSETS)), "margin": np.array(MARGIN)}
        most, worst_box = 0, 0.0
        for name, (samples, refs, batch, m_equal, cv) in results.items():
            mode, over, seed, items = T.ARGSETS[name]
            out[f"{name}/mode"], out[f"{name}/seed"], out[f"{name}/items"] = np.array(mode), np.array(seed), np.array(items, np.int64)
            out[f"{name}/over"] = np.array(json.dumps(over))
            out[f"{name}/m_equal"] = np.array(m_equal, np.bool_)
            for n, s in enumerate(samples):
                for k, v in T.pack_sample(s).items():
                    out[f"{name}/s{n}/{k}"] = v
                _, box, _ = yolo2d_ref.labels(s, rows, T.IMGSZ)
                if len(box):
                    worst_box = max(worst_box, float(np.abs(box - refs[n]["bboxes"].numpy()).max()))
            counts = np.array([int(r["bboxes"].shape[0]) for r in refs], np.int64)
            most = max(most, int(counts.max()))
            out[f"{name}/counts"] = counts
            for k in ("cls", "bboxes", "batch_idx"):
                out[f"{name}/c/{k}"] = batch[k].numpy()
            if cv is not None:
                out[f"{name}/cv2/img"] = np.stack([c[0] for c in cv])
                out[f"{name}/cv2/max_abs"] = np.array([c[1] for c in cv], np.int64)
                out[f"{name}/cv2/mean_abs"] = np.array([c[2] for c in cv], np.float64)
        allc = np.concatenate([out[f"{n}/counts"] for n in T.ARGSETS])
        assert (allc > 64).any() and (allc > 128).any(), f"no sample over 64 / 128 rows (largest {most})"
        np.savez_compressed(OUT, **out)
        eq = np.concatenate([out[f"{n}/m_equal"] for n in T.ARGSETS])
        print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(allc)} samples, counts up to {most}, {int((allc > 64).sum())} over 64, "
              f"{int((allc > 128).sum())} over 128; filters (dropped, kept) {stat}; M equal to the reference's in {int(eq.sum())} of {len(eq)} "
              f"(the rest 1 ulp); float32 emulation vs reference boxes: max abs {worst_box:.3g}; redraw rounds {attempt}")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
