"""The inputs and the calls of the bit pin of the 3D label and plan kernels (tests/golden/label3d_pin.npz, recorded by
tools/make_golden_label3d_pin.py, compared by tests/test_hip_label3d_pin.py): `y3d_kitti_encode_labels`, `y3d_json3d_encode_labels`
for Waymo and Omni3D, `y3d_kitti_plan_batch` and `y3d_json3d_plan_batch`, each through its Python wrapper.  Everything is drawn from
`np.random.RandomState`, the legacy generator, whose stream does not change between numpy versions; every value is finite.  No
reference is involved: the pin records what one build computes so that another can be held to the same bytes.

Encoders: six images with 0, 1, 50, 64, 70 and 40 candidate lines; the last one's partner has 30, so at max_objs = 50 it is clipped to
10.  The image without primary lines has a partner of 70: wave 1 alone holds its candidates, and at max_objs = 64 all 64 of its lanes are
live (the full ballot mask, rank under lane 63), as wave 0's are for the images with 64 and 70 lines; the line lane 63 takes survives.
Every field is drawn on both sides of the filter that reads it (class ids -1 .. n_cls; KITTI's truncation, occlusion and box heights
around 25 and 40; depths around min_depth and max_depth; projected centres around -1, 0, out_w and out_h; Waymo's lidar
counts around 50 and 100; Omni3D's flags), ry includes +-pi, and every 17th line has px = 0.0, which a flip turns into -0.0.
Plan kernels: five frames of different sizes in a 4 KB arena that is never read, 65 draws (two blocks), and for json3d the three
placements n_dev = 5, 2, 0."""
import hashlib

import numpy as np

SEED = 20261020
KINDS = ("kitti", "waymo", "omni3d")
COUNTS = (0, 1, 50, 64, 70, 40)   # candidate lines of the six primaries
PARTNERS = (70, 70, 5, 2, 0, 30)  # ... of their partners in the runs with partners (image 4 has none)
FLIPS = {"a": (1, 0, 1, 0, 1, 0), "b": (0, 1, 0, 1, 0, 1)}
# (max_objs, flip pattern, use_camera_dis, partners): every pair of settings occurs at max_objs = 50.  At 64 with partners lane 63 of
# wave 0 is live in images 3 and 4 (n0 = 64) and lane 63 of wave 1 in image 0 (n0 = 0, n1 = min(70, 64 - 0)); `wave_lanes` states it
ENCODER_RUNS = ((50, "a", 0, 1), (50, "b", 1, 1), (50, "a", 1, 0), (50, "b", 0, 0), (64, "a", 0, 1), (64, "b", 1, 0), (1, "b", 0, 1),
                (1, "a", 1, 0))
MIN_DEPTH, MAX_DEPTH, N_CLS = 1.0, 120.0, 3
SCALES = (1.0, 0.8, 1.2, 0.9, 1.0, 1.1)
# out (W, H); the two frame sizes (W, H); fu, cu, cv; the fourth column (P03, P13, P23) of the images that have one
GEOMETRY = {"kitti": ((1280, 384), ((1242, 375), (1224, 370)), (721.5377, 609.5593, 172.854), (44.85728, 0.2163791, 0.002745884)),
            "json3d": ((960, 640), ((1920, 1280), (1600, 1066)), (2055.556149, 939.657724, 641.072097), (1.3177, -0.2113, 0.00271))}
LABEL_KEYS = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res", "batch_idx", "counts",
              "calib", "ratio_pad")
PLAN_KEYS = ("src", "src2", "hw", "flip", "trans_inv", "img_i", "img_f", "mixed")
PLAN_HW = ((4, 6), (8, 8), (5, 7), (10, 12), (3, 3))  # (h, w) of the five frames
PLAN_LINES = (3, 0, 7, 2, 5)
PLAN_B, ARENA_BYTES = 65, 4096
PLACEMENTS = (5, 2, 0)  # n_dev of the json3d plan runs
PLAN_RUNS = (("kitti", 5),) + tuple(("waymo", n) for n in PLACEMENTS)


def f32(a):
    """float32 values held in float64, as the records and a mirrored calibration hold them"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def mean_size(kind):
    from yolov10_3d_amd import json3d, kitti
    return np.asarray(kitti.CLS_MEAN_SIZE if kind == "kitti" else json3d.CLS_MEAN_SIZE[kind], np.float64).reshape(-1, 3)


def encoder_tables(kind):
    """-> rec (R, 16 or 24) float64, and per image: (first row, primary lines, partner lines), (W, H), P2 as read and mirrored (12 each),
    trans (6), scale.  A line's 3D centre is placed so that it lands at a drawn point of the OUTPUT image when the image is not
    mirrored; the mirrored calibration is the mirror image of the other, so the mirrored run lands at about out_w - x."""
    rng = np.random.RandomState(SEED + KINDS.index(kind))
    (out_w, out_h), sizes, (fu0, cu0, cv0), col4 = GEOMETRY["kitti" if kind == "kitti" else "json3d"]
    ms = mean_size(kind)
    recs, images, row = [], [], 0
    for b, (n0, n1) in enumerate(zip(COUNTS, PARTNERS)):
        W, H = sizes[b % 2]
        fu, cu, cv = fu0 * (1 + 0.01 * b), cu0 * W / sizes[0][0] + b, cv0 * H / sizes[0][1] - b
        p03, p13, p23 = col4 if b % 3 != 2 else (0.0, 0.0, 0.0)
        P = np.array([fu, 0.0, cu, p03, 0.0, fu, cv, p13, 0.0, 0.0, 1.0, p23])
        Pm = np.array([fu * (1 + 3e-7), 0.0, W - cu, -p03 * (1 - 2e-7), 0.0, fu * (1 + 3e-7), cv, p13, 0.0, 0.0, 0.0, p23])
        P, Pm = (f32(P) if kind == "kitti" else P), f32(Pm)
        s = SCALES[b]
        r = out_w / (W * s)
        cx, cy = W / 2 + (7.0 if s != 1.0 else 0.0), H / 2 - (3.0 if s != 1.0 else 0.0)
        trans = np.array([r, 0.001 * (b % 2), out_w / 2 - r * cx, -0.0005 * (b % 2), r, out_h / 2 - r * cy])
        n = n0 + n1
        edge = lambda size: np.where(rng.rand(n) < 0.7, rng.uniform(0, size, n),
                                     np.array([rng.uniform(-2, 1, n), rng.uniform(size - 1, size + 2, n), rng.uniform(-60, -2, n),
                                               rng.uniform(size + 2, size + 60, n)])[rng.randint(4, size=n), np.arange(n)])
        X, Y = edge(out_w), edge(out_h)
        X = np.where(rng.rand(n) < 0.5, X, r * W + 2 * trans[2] - X)  # half of the lines are aimed in the mirrored image
        cls = rng.choice([-1, 0, 1, 2, 3], n, p=[0.06, 0.3, 0.3, 0.28, 0.06])
        pz = np.where(rng.rand(n) < 0.7, rng.uniform(4, 90, n), rng.choice([-5.0, 0.85, 0.95, 1.0, 1.05, 1.2, 99.0, 101.0, 109.0, 119.0, 121.0, 140.0], n))
        # the lines that lane 0 and lane 63 of either wave take pass every filter (max_objs = 1 keeps one; lane 63 ranks under a full mask)
        first = sorted(i for i in {0, n0, 63, n0 + 63} if i < n)
        X[first], Y[first], cls[first], pz[first] = 0.4 * out_w, 0.6 * out_h, b % 3, 20.0
        u, v = (X - trans[2]) / r, (Y - trans[5]) / r
        dims = ms[np.clip(cls, 0, 2)] * rng.uniform(0.9, 1.1, (n, 3))
        pz = f32(pz) if kind == "kitti" else pz
        px = ((u - cu) * pz - p03) / fu
        py = ((v - cv) * pz - p13) / fu + dims[:, 0] / 2
        px[(row + np.arange(n)) % 17 == 0] = 0.0
        ry = np.where(rng.rand(n) < 0.9, rng.uniform(-np.pi, np.pi, n), rng.choice([np.pi, -np.pi, 0.0], n))
        bw, bh = rng.uniform(10, 200, n), rng.choice([23.5, 24.0, 25.0, 26.0, 39.0, 40.0, 41.0, 60.0, 90.0], n) - 1.0
        bh[first] = 59.0
        x1, y1 = u - bw / 2 + rng.uniform(-4, 4, n), v - bh / 2 + rng.uniform(-4, 4, n)
        box = f32(np.stack([x1, y1, x1 + bw, f32(y1) + bh], 1))
        rec = np.zeros((n, 16 if kind == "kitti" else 24))
        if kind == "kitti":
            rec[:, 0], rec[:, 1], rec[:, 2] = cls, rng.choice([-1, 0, 0.15, 0.3, 0.5, 0.6], n, p=[0.1, 0.4, 0.15, 0.15, 0.1, 0.1]), rng.choice(4, n, p=[0.5, 0.2, 0.2, 0.1])
            rec[first, 1:3] = 0.0
            rec[:, 3:7], rec[:, 7:10], rec[:, 13] = box, dims, ry
            rec[:, 10], rec[:, 11], rec[:, 12] = f32(px), f32(py), pz
        else:
            rec[:, 0], rec[:, 1:5], rec[:, 5:8], rec[:, 11] = cls, box, dims, ry
            rec[:, 8], rec[:, 9], rec[:, 10] = px, py, pz
            rec[:, 12] = rng.choice([0, 30, 49, 50, 51, 99, 100, 101, 400, 900], n, p=[0.04, 0.03, 0.03, 0.05, 0.05, 0.05, 0.05, 0.1, 0.3, 0.3])
            rec[:, 13], rec[:, 14] = rng.rand(n) < 0.06, rng.rand(n) >= 0.06
            rec[:, 15] = rng.choice([0.0, 0.1, 0.49, 0.5, 0.51, 2.0], n, p=[0.3, 0.4, 0.1, 0.07, 0.07, 0.06])
            rec[:, 16] = rng.choice([0.0, 0.2, 0.74, 0.75, 0.76, 1.0], n, p=[0.4, 0.3, 0.1, 0.07, 0.07, 0.06])
            rec[:, 17] = rng.choice([-1.0, 0.2, 0.25, 0.3, 0.7, 1.0], n, p=[0.2, 0.06, 0.06, 0.1, 0.28, 0.3])
            rec[first, 12:18] = (900, 0, 1, 0.1, 0.2, 1.0)
        recs.append(rec)
        images.append(((row, n0, n1), (W, H), P, Pm, trans, s))
        row += n
    assert np.isfinite(np.concatenate(recs)).all()
    return np.concatenate(recs), images


def wave_lanes(max_objs, partners):
    """per image the live lanes (wave 0, wave 1) of a run, by the encoders' rule n0 = min(n, max_objs), n1 = min(n2, max_objs - n0)"""
    return [(min(n, max_objs), min(n2 if partners else 0, max_objs - min(n, max_objs))) for n, n2 in zip(COUNTS, PARTNERS)]


def encoder_case(images, flips, partners):
    """-> img_i (6, 7) int32, img_f (6, 19) float64 of one run"""
    img_i, img_f = np.zeros((len(images), 7), np.int32), np.zeros((len(images), 19), np.float64)
    for b, ((row, n0, n1), (W, H), P, Pm, trans, s) in enumerate(images):
        img_i[b] = (row, n0, row + n0, n1 if partners else 0, flips[b], W, H)
        img_f[b, :12], img_f[b, 12:18], img_f[b, 18] = (Pm if flips[b] else P), trans, s
    return img_i, img_f


def plan_tables(kind, n_dev):
    """-> img_off (5) int64 (-1 behind n_dev), frame_hw (5, 2) int32, rec_span (5, 2) int32, P2 (5, 2, 12) float32 (kitti) or float64,
    padded (5) int64, draws (65, 16 or 18) float64, staging bytes"""
    from yolov10_3d_amd import resident
    rng = np.random.RandomState(SEED + 10 + KINDS.index(kind))
    N = len(PLAN_HW)
    hw = np.array(PLAN_HW, np.int64)
    padded = (hw[:, 0] * hw[:, 1] * 3 + 15) // 16 * 16
    starts = np.concatenate(([0], np.cumsum(padded)[:-1])).astype(np.int64)
    img_off = np.where(np.arange(N) < n_dev, starts, -1)
    P2 = rng.uniform(-800, 800, (N, 2, 12))
    P2 = P2.astype(np.float32) if kind == "kitti" else P2
    pos = np.concatenate((np.arange(N), [N - 1, N - 1, 0, 0], rng.randint(N, size=PLAN_B - N - 4)))  # every frame, repeats, then drawn
    par = np.where(rng.rand(PLAN_B) < 0.5, rng.randint(N, size=PLAN_B), -1)
    par[:3], par[-1] = (-1, 0, N - 1), N - 1  # the last draw (thread 0 of the second block) has a partner
    draws = np.empty((PLAN_B, 16 if kind == "kitti" else 18), np.float64)
    draws[:, 0], draws[:, 1], draws[:, 2], draws[:, 3] = pos, par, rng.randint(2, size=PLAN_B), rng.uniform(0.8, 1.2, PLAN_B)
    draws[:, 4:16] = rng.uniform(-700, 700, (PLAN_B, 12))
    nbytes = 0
    if kind != "kitti":
        at, nbytes = resident.stage_layout([p for pair in zip(pos, par) for p in pair], n_dev, padded)
        draws[:, 16], draws[:, 17] = [at.get(int(p), -1) for p in pos], [at.get(int(p), -1) for p in par]
        assert all(o % 16 == 0 for o in at.values()) and (n_dev == N) == (not at)
    assert int(starts[-1] + padded[-1]) <= ARENA_BYTES and (par >= 0).any() and (par < 0).any() and np.isfinite(draws).all()
    return img_off, hw.astype(np.int32), resident.span_table(PLAN_LINES), P2, padded, draws, nbytes


def inputs_digest():
    """SHA-256 over every input table of every run: a drift of the generator shows here, apart from a difference of the kernels"""
    h = hashlib.sha256()
    for kind in KINDS:
        rec, images = encoder_tables(kind)
        h.update(np.ascontiguousarray(rec).tobytes() + mean_size(kind).tobytes())
        for max_objs, fl, cam_dis, partners in ENCODER_RUNS:
            for t in encoder_case(images, FLIPS[fl], partners):
                h.update(t.tobytes())
            h.update(np.array([max_objs, cam_dis, MIN_DEPTH, MAX_DEPTH], np.float64).tobytes())
    for kind, n_dev in PLAN_RUNS:
        for t in plan_tables(kind, n_dev)[:6]:
            h.update(np.ascontiguousarray(t).tobytes())
    return h.hexdigest()


class _Split:
    """what `kitti.plan_batch` / `json3d.plan_batch` read of a DeviceSplit"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return len(PLAN_HW)


def _based(ptr, arena, stage):
    """pointers -> (B, 2) int64 (tag, offset): 0 null, 1 from the arena's base, 2 from the staging buffer's, 3 anything else (as it is)"""
    out = np.zeros((len(ptr), 2), np.int64)
    for b, p in enumerate(ptr.tolist()):
        for tag, t in ((1, arena), (2, stage)):
            if p and t is not None and t.data_ptr() <= p < t.data_ptr() + t.numel():
                out[b] = (tag, p - t.data_ptr())
        if p and not out[b, 0]:
            out[b] = (3, p)
    return out


def run(dev="cuda"):
    """every pinned call on the device -> {"<kind>/<key>": an encoder output of the eight ENCODER_RUNS, "plan/<key>": a plan output of
    the four PLAN_RUNS}, the runs laid end to end along the first axis (one array per key keeps the file small: the runs repeat much)"""
    import torch
    from yolov10_3d_amd import json3d, kitti
    from yolov10_3d_amd.resident import upload
    out, runs = {}, {}
    for kind in KINDS:
        rec, images = encoder_tables(kind)
        out_wh = GEOMETRY["kitti" if kind == "kitti" else "json3d"][0]
        packed = {"rec": upload(rec, dev, torch.float64), "mean_size": upload(mean_size(kind), dev, torch.float64), "dataset": kind}
        for max_objs, fl, cam_dis, partners in ENCODER_RUNS:
            img_i, img_f = encoder_case(images, FLIPS[fl], partners)
            packed.update(img_i=upload(img_i, dev, torch.int32), img_f=upload(img_f, dev, torch.float64))
            encode = kitti.encode_labels if kind == "kitti" else json3d.encode_labels
            lab = encode(packed, out_wh, MIN_DEPTH, MAX_DEPTH, bool(cam_dis), max_objs)
            for k in LABEL_KEYS:
                runs.setdefault(f"{kind}/{k}", []).append(lab[k].cpu().numpy())
    arena = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device=dev)
    for kind, n_dev in PLAN_RUNS:
        img_off, hw, span, P2, padded, draws, nbytes = plan_tables(kind, n_dev)
        sp = _Split(device=arena.device, img_off=upload(img_off, dev, torch.int64), frame_hw=upload(hw, dev, torch.int32),
                    rec_span=upload(span, dev, torch.int32), P2=upload(P2, dev), arena=arena, n_dev=n_dev,
                    _frame_bytes=np.array([h * w * 3 for h, w in PLAN_HW], np.int64))
        stage = torch.zeros(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        plan = kitti.plan_batch(sp, draws) if kind == "kitti" else json3d.plan_batch(sp, draws, spill=stage)
        for k in PLAN_KEYS:
            v = plan[k].cpu().numpy()
            runs.setdefault(f"plan/{k}", []).append(_based(v, arena if n_dev else None, stage) if k in ("src", "src2") else v)
    torch.cuda.synchronize()
    for k, v in runs.items():
        assert len({(a.dtype, a.shape[1:]) for a in v}) == 1, k
        out[k] = np.concatenate(v)
    return out


def run_of(key, row):
    """the run that wrote row `row` of `run()`'s array `key`, for a failure's message"""
    if key.startswith("plan/"):
        return "%s plan, n_dev = %d" % PLAN_RUNS[row // PLAN_B]
    per_image = key.split("/")[1] in ("counts", "calib", "ratio_pad")
    for max_objs, fl, cam_dis, partners in ENCODER_RUNS:
        n = len(COUNTS) * (1 if per_image else max_objs)
        if row < n:
            return f"max_objs {max_objs}, flips {fl}, use_camera_dis {cam_dis}, partners {partners}, image {row // (n // len(COUNTS))}"
        row -= n
