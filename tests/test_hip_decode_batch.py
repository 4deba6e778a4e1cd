"""GPU: the label decode (csrc/decode_labels.hip, `kitti.decode_labels`, `kitti.decode_batch_device`, `json3d.decode_batch_device`) and the
label pictures built on it (`plot.draw_labels3d`, `plot.label_pictures`, `val.Validator3d(pictures=...)`).

1. against the float64 restatement of tests/decode_batch_ref.py fed the same device inputs, with sentinel-filled guard space around every
   output; 2. against the reference's own `decode_batch` (tests/golden/decode_batch.npz) for KITTI, Waymo and Omni3D; 3. the round trip
   label_2 -> build_batch(mode="val") -> decode_batch(undo_augment=True); 4. a captured and replayed launch; 5. the pictures.

A box whose centre lies behind the camera is decoded like any other row (the reference does the same); its corners are written as
computed, and `corners_img` is compared only for boxes at least 0.5 m in front of the camera, as DESIGN 3.18 does for predictions
(`plot.box3d_segments` clips or drops such a box at the near plane, 3.22)."""
import functools
import os

import numpy as np
import pytest
import torch

import decode_batch_ref as D
import draw_ref as DR
from kitti_labels_tree import fixture as tree_fixture, write_tree

import yolov10_3d_amd as y3d
from yolov10_3d_amd import json3d, kitti, plot, predict, val
from yolov10_3d_amd import ops as P_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64          # sentinel elements on either side of every output
SENTINEL = -7.25e77
RES = (320, 256)


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    before = P_ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(shape, dtype):
    """-> (the whole sentinel-filled buffer, the view of `shape` in its middle)"""
    n = int(np.prod(shape))
    fill = SENTINEL if dtype == torch.float64 else -77
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def _guards_intact(whole, dtype):
    fill = SENTINEL if dtype == torch.float64 else -77
    h = whole.cpu()
    return bool((h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all())


def _launch(lab, counts_in, ori, c6, rp, inv, P2, ms, undo, cam, R):
    """one guarded launch through kitti.decode_labels -> numpy (rows, corners3d, corners_img or None, counts)"""
    B = len(ori)
    t = {k: _dev(v) for k, v in lab.items()}
    bufs = [_guarded((B, R, 14), torch.float64), _guarded((B, R, 8, 3), torch.float64),
            _guarded((B, R, 8, 2), torch.float64) if P2 is not None else (None, None), _guarded((B,), torch.int32)]
    out = kitti.decode_labels(t, None if counts_in is None else _dev(counts_in), _dev(ori), _dev(c6), _dev(rp), None if inv is None else _dev(inv),
                              None if P2 is None else _dev(P2), _dev(np.asarray(ms, np.float64)), undo, cam, R, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    for (whole, _), dt in zip(bufs, (torch.float64, torch.float64, torch.float64, torch.int32)):
        assert whole is None or _guards_intact(whole, dt), "an output's guard space was written"
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _compare(got, want, P2_given=True):
    rows, c3, ci, counts = got
    wrows, wc3, wci, wcounts = want
    assert counts.dtype == np.int32 and counts.tolist() == wcounts.tolist()
    B, R = rows.shape[:2]
    checked = 0
    for b in range(B):
        n = counts[b]
        assert not rows[b, n:].view(np.int64).any() and not c3[b, n:].view(np.int64).any(), b  # zeros behind the counts (+0.0 bits)
        assert np.array_equal(rows[b, :n, 0], wrows[b, :n, 0]) and (rows[b, :n, 13] == 1).all(), b   # class column and row order exact
        np.testing.assert_allclose(rows[b, :n], wrows[b, :n], rtol=0, atol=1e-9, equal_nan=True, err_msg=f"rows of image {b}")
        np.testing.assert_allclose(c3[b, :n], wc3[b, :n], rtol=0, atol=1e-9, equal_nan=True, err_msg=f"corners3d of image {b}")
        if P2_given:
            assert not ci[b, n:].view(np.int64).any(), b
            front = wc3[b, :n, :, 2].min(1) >= 0.5 if n else np.zeros(0, bool)
            np.testing.assert_allclose(ci[b, :n][front], wci[b, :n][front], rtol=1e-9, atol=1e-9, err_msg=f"corners_img of image {b}")
            checked += int(front.sum())
        else:
            assert ci is None
    return checked


# ---------------------------------------------------------------------------------------------------------------- 1. the restatement
# name -> (boxes per image, layout, undo_augment, trans_inv given, use_camera_dis, ratio_pad as (B, 2), six-class table, P2 given, R)
SHAPES = {
    "b1_empty": ((0,), "ragged", True, True, False, False, False, True, 50),
    "b1_empty_static": ((0,), "static", False, False, False, False, False, True, 50),
    "b1_one": ((1,), "ragged", True, True, False, False, False, True, 50),
    "b1_one_static": ((1,), "static", True, True, True, True, True, True, 50),
    "b3_ragged": ((0, 50, 7), "ragged", True, True, False, False, False, True, 50),
    "b3_static": ((0, 50, 7), "static", True, True, False, False, False, True, 50),
    "b3_ragged_plain": ((0, 50, 7), "ragged", False, False, False, True, False, True, 50),
    "b3_static_plain": ((0, 50, 7), "static", False, True, False, True, True, False, 50),
    "b3_camdis": ((0, 50, 7), "ragged", True, True, True, False, True, True, 50),
    "b3_camdis_plain": ((0, 50, 7), "static", False, False, True, False, False, True, 50),
    "middle_empty": ((5, 0, 3), "ragged", True, True, False, False, False, True, 8),
    "interleaved": ((9, 0, 70, 4), "shuffled", True, True, False, False, True, True, 64),   # 83 rows: two chunks, rows of images mixed
    "clamped": ((7, 3), "static", True, True, False, False, False, True, 5),               # R below an image's count
    "clamped_ragged": ((70, 3), "ragged", False, False, False, True, False, True, 50),
    "b70": (tuple(int(v) for v in np.random.default_rng(70).integers(0, 7, 70)), "ragged", True, True, False, False, False, True, 6),
    "b70_static": (tuple(int(v) for v in np.random.default_rng(71).integers(0, 7, 70)), "static", False, False, False, False, True, True, 6),
}


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    counts, layout, undo, inv_given, cam, rp2, six, p2_given, R = SHAPES[name]
    nc = 6 if six else 3
    lab, ori, c6, P2, rp, inv = D.synth(counts, 1000 + len(counts) * 7 + sum(counts), nc=nc, shuffle=(layout == "shuffled"))
    counts_in = None
    if layout == "static":
        M = max(max(counts), 1) if name.startswith("clamped") else 50
        lab, counts_in = D.to_static(lab, len(counts), M)
    rp = rp[:, 0].copy() if rp2 else rp
    ms = D.SIX_MEAN if six else D.KITTI_MEAN
    args = (lab, counts_in, ori, c6, rp, inv if inv_given else None, P2 if p2_given else None, ms, undo, cam, R)
    return args, _launch(*args), D.decode(*args)


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_the_restatement(name):
    args, got, want = _shape_case(name)
    counts = SHAPES[name][0]
    checked = _compare(got, want, SHAPES[name][7])
    assert got[3].tolist() == [min(c, SHAPES[name][8]) for c in counts]
    if SHAPES[name][7] and not SHAPES[name][4] and sum(counts):  # pinhole depth 3 .. 63 m: nearly every box lies in front
        assert checked >= 0.9 * got[3].sum()


def test_crafted_rows():
    """bin 11 with a residual that wraps, rotation_y one ulp on either side of +-pi, a centre behind the camera and one on its plane"""
    lab, ori, c6, P2, rp, inv, names, want_ry = D.crafted()
    for undo in (False, True):
        args = (lab, None, ori, c6, rp, inv, P2, D.KITTI_MEAN, undo, False, 16)
        got, want = _launch(*args), D.decode(*args)
        _compare(got, want)
        r = dict(zip(names, got[0][0]))
        assert r["bin11_wraps"][1] == (11 * (2 * np.pi / 12) + 0.2) - 2 * np.pi
        for name, ry in want_ry.items():
            assert r[name][12] == ry, (name, undo, r[name][12], ry)   # to the bit: a wrap is 2 pi away
        # behind the camera: the row is decoded as any other, the corners are the plain formulas' (z < 0), nothing is dropped here
        k = names.index("behind_camera")
        assert got[3][0] == len(names) and r["behind_camera"][11] == -7.5 and (got[1][0, k, :, 2] < 0).all() and np.isfinite(got[2][0, k]).all()


def test_class_outside_the_table_is_signalled_per_row():
    """as y3d_kitti_decode: the class column keeps the label, the size comes from the nearest table entry; decode_batch raises"""
    lab, ori, c6, P2, rp, inv = D.synth((4, 2), 9)
    lab["cls"][:] = [0, 7, -2, 2, 3, 1]
    args = (lab, None, ori, c6, rp, inv, P2, D.KITTI_MEAN, True, False, 8)
    got, want = _launch(*args), D.decode(*args)
    _compare(got, want)
    assert got[0][0, :4, 0].tolist() == [0, 7, -2, 2] and got[0][1, :2, 0].tolist() == [3, 1]
    ms = np.asarray(D.KITTI_MEAN)
    np.testing.assert_allclose(got[0][0, 1, 6:9], lab["size_3d"][1] + ms[2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[0][0, 2, 6:9], lab["size_3d"][2] + ms[0], rtol=0, atol=1e-12)
    batch = _batch_dict(lab, ori, rp, inv)
    with pytest.raises(y3d.Y3DError, match="outside the mean-size table"):
        kitti.decode_batch(batch, [tuple(c) for c in c6])
    lab["cls"][:] = [0, 1, 2, 2, 1, 1]
    res = kitti.decode_batch(_batch_dict(lab, ori, rp, inv), [tuple(c) for c in c6])
    assert [len(v) for v in res.values()] == [4, 2] and res["000000.txt"][3][0] == 2 and res["000001.txt"][0][13] == 1


def test_wrapper_refusals_on_the_device():
    lab, ori, c6, P2, rp, inv = D.synth((2, 1), 5)
    t = {k: _dev(v) for k, v in lab.items()}
    a = [_dev(ori), _dev(c6), _dev(rp), _dev(inv), _dev(P2), _dev(np.asarray(D.KITTI_MEAN))]
    ok = kitti.decode_labels(t, None, *a, True, False, 4)
    assert ok[3].tolist() == [2, 1]
    with pytest.raises(y3d.Y3DError, match="must be a contiguous int64"):
        kitti.decode_labels(dict(t, cls=t["cls"].double()), None, *a, True, False, 4)
    with pytest.raises(y3d.Y3DError, match="next to 3 rows"):
        kitti.decode_labels(dict(t, depth=t["depth"][:2].contiguous()), None, *a, True, False, 4)
    with pytest.raises(y3d.Y3DError, match="R = 0"):
        kitti.decode_labels(t, None, *a, True, False, 0)
    with pytest.raises(y3d.Y3DError, match="undo_augment needs trans_inv"):
        kitti.decode_labels(t, None, a[0], a[1], a[2], None, a[4], a[5], True, False, 4)
    with pytest.raises(y3d.Y3DError, match="does not divide"):
        kitti.decode_labels(t, torch.zeros(2, dtype=torch.int32, device=DEV), *a, True, False, 4)
    with pytest.raises(y3d.Y3DError, match="outputs must be"):
        kitti.decode_labels(t, None, *a, True, False, 4, out=(ok[0][:, :2], ok[1], ok[2], ok[3]))
    # an output that is a view into an input's memory, and two outputs sharing memory: refused by the entry
    big = torch.zeros(2 * 4 * 14 + 12, dtype=torch.float64, device=DEV)
    lab2 = dict(t, bboxes=big[:12].view(3, 4))
    with pytest.raises(y3d.Y3DError, match="overlaps an input"):
        kitti.decode_labels(lab2, None, *a, True, False, 4, out=(big[2:2 + 112].view(2, 4, 14), ok[1], ok[2], ok[3]))
    both = torch.zeros(2 * 4 * 24 + 2 * 4 * 14, dtype=torch.float64, device=DEV)
    with pytest.raises(y3d.Y3DError, match="overlap each other"):
        kitti.decode_labels(t, None, *a, True, False, 4, out=(both[:112].view(2, 4, 14), both[110:110 + 192].view(2, 4, 8, 3), ok[2], ok[3]))
    with pytest.raises(y3d.Y3DError, match="aligned"):
        kitti.decode_labels(t, None, *a, True, False, 4, out=(both[1:113].view(2, 4, 14), ok[1], ok[2], ok[3]))


# ---------------------------------------------------------------------------------------------------------------- 2. the reference
def _batch_dict(lab, ori, rp, inv, static_counts=None, im_files=None):
    """a batch dictionary as the builders return it, from numpy arrays in any of the reference's dtypes"""
    b = {k: _dev(np.ascontiguousarray(v)) for k, v in lab.items()}
    B = len(ori)
    b.update(ori_shape=[np.array(o) for o in ori], ratio_pad=_dev(np.asarray(rp, np.float64)), info=[{"trans_inv": np.asarray(t, np.float64)} for t in inv],
             im_file=im_files or [f"{i:06d}.txt" for i in range(B)])
    if static_counts is not None:
        b["counts"] = _dev(np.asarray(static_counts, np.int32))
    return b


REF_CASES = [(ds, run, undo) for ds, runs in D.RUNS.items() for run in runs for undo in (True, False)]


@pytest.mark.parametrize("dataset,run,undo", REF_CASES)
def test_decode_matches_the_reference(dataset, run, undo):
    I = D.fixture_inputs(dataset, run)
    batch = _batch_dict(I["lab"], I["ori_shape"], I["ratio_pad"], I["trans_inv"])  # the reference's own collated dtypes
    calibs = [tuple(c) for c in I["calib6"]]
    if dataset == "kitti":
        out = kitti.decode_batch_device(batch, calibs, I["P2"], undo, use_camera_dis=I["cam_dis"])
    else:
        out = json3d.decode_batch_device(batch, _dev(I["calib6"]), _dev(I["P2"]), undo, dataset=dataset, use_camera_dis=I["cam_dis"])
    rows, c3, ci, counts = (o.cpu().numpy() for o in out)
    want, want_counts = D.fixture_rows(dataset, run, undo)
    assert counts.tolist() == want_counts.tolist() and rows.shape[1] == min(len(I["lab"]["cls"]), 50)
    got = D.ragged(rows, counts)
    assert np.array_equal(got[:, 0], want[:, 0])
    print(f"{dataset}/{run} undo={undo}: max |rows - reference| per column {np.abs(got - want).max(0)}")
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    if run == "val" and undo:
        g = D.fixture()
        pick = g[f"{dataset}/val/corner_rows"]
        e3 = np.abs(D.ragged(c3, counts)[pick] - g[f"{dataset}/val/corners3d"]).max()
        ei = np.abs(D.ragged(ci, counts)[pick] - g[f"{dataset}/val/corners_img"]).max()
        print(f"{dataset}/val: max |corners3d - reference| {e3:.3g} m, |corners_img - reference| {ei:.3g} px over {len(pick)} boxes")
        assert e3 <= 1e-4 and ei <= 2e-2
    # the static layout of the same batch gives the same bits, and the host dictionary is the reference's
    if undo:
        st, cnt = D.to_static(I["lab"], I["B"], 50)
        sb = _batch_dict(st, I["ori_shape"], I["ratio_pad"], I["trans_inv"], static_counts=cnt)
        srows = kitti.decode_batch_device(sb, calibs, None, undo, I["mean_size"], I["cam_dis"])
        assert srows[2] is None and srows[3].cpu().tolist() == counts.tolist()
        assert np.array_equal(D.ragged(srows[0].cpu().numpy(), counts).view(np.int64), got.view(np.int64))
        files = [f"{n:02d}.txt" for n in range(I["B"])]
        res = (kitti.decode_batch(dict(batch, im_file=files), calibs, undo, I["mean_size"], I["cam_dis"]) if dataset == "kitti" else
               json3d.decode_batch(dict(batch, im_file=files), calibs, undo, dataset, I["cam_dis"]))
        assert list(res) == files and [len(res[f]) for f in files] == counts.tolist()
        flat = np.array([r for f in files for r in res[f]], np.float64).reshape(-1, 14)
        assert np.array_equal(flat.view(np.int64), got.view(np.int64)) and all(isinstance(r[0], int) for f in files for r in res[f])


# ---------------------------------------------------------------------------------------------------------------- 3. round trip
@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("kitti_decode_batch")), tree_fixture(), images=True)


def test_val_batch_round_trip(root):
    """label_2 -> build_batch(mode="val") -> decode_batch(undo_augment=True): every decoded row is one of its frame's first 50 label
    lines, in file order, with that line's dimensions, location and rotation_y.  Measured on an MI355X: see the printed maxima
    (DESIGN 3.23 records them)."""
    n = len(tree_fixture()["label_text"])
    idx = list(range(n))
    batch = kitti.build_batch(root, idx, kitti.data_args(), DEV, mode="val")
    calibs = [kitti.calib_params(kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt"))) for i in idx]
    res = kitti.decode_batch(batch, calibs, undo_augment=True)
    worst, total = np.zeros(7), 0
    for i in idx:
        anno = kitti.read_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
        truth = np.concatenate([np.stack([anno["h"], anno["w"], anno["l"]], 1), anno["pos"].astype(np.float64), anno["ry"][:, None]], 1)[:50]
        names = anno["type"][:50]
        last = -1
        for row in res[f"{i:06d}.txt"]:
            got = np.array(row[6:13])
            cand = [k for k in range(last + 1, len(truth)) if kitti.CLASS_IDS.get(names[k], -1) == row[0]]
            assert cand, (i, row)
            k = min(cand, key=lambda k: np.abs(truth[k] - got).max())
            worst = np.maximum(worst, np.abs(truth[k] - got))
            np.testing.assert_allclose(got, truth[k], rtol=1e-5, atol=1e-5, err_msg=f"frame {i}, label line {k}")
            last, total = k, total + 1
    print(f"round trip over {total} kept labels: max |decoded - label_2| h, w, l, x, y, z, ry = {worst}")
    assert total >= 40


# ---------------------------------------------------------------------------------------------------------------- 4. graph replay
def test_launch_replays_under_capture():
    """recorded once, replayed with new labels: bit-equal to the eager call (one kernel node, the default queue settings)"""
    counts = (0, 50, 7)
    first = D.to_static(D.synth(counts, 11)[0], 3, 50)
    second = D.to_static(D.synth((13, 2, 50), 12)[0], 3, 50)
    _, ori, c6, P2, rp, inv = D.synth(counts, 11)
    a = [_dev(ori), _dev(c6), _dev(rp), _dev(inv), _dev(P2), _dev(np.asarray(D.KITTI_MEAN))]
    st = {k: _dev(v) for k, v in first[0].items()}
    cnt = _dev(first[1])
    launch = lambda lab, c: kitti.decode_labels(lab, c, *a, True, False, 50)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(st, cnt)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = launch(st, cnt)
    for k, v in second[0].items():
        st[k].copy_(_dev(v))
    cnt.copy_(_dev(second[1]))
    graph.replay()
    torch.cuda.synchronize()
    want = launch({k: _dev(v) for k, v in second[0].items()}, _dev(second[1]))
    before = launch({k: _dev(v) for k, v in first[0].items()}, _dev(first[1]))
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for got, w in zip(out, want):
        assert torch.equal(bits(got), bits(w))
    assert out[3].tolist() == [13, 2, 50] and before[3].tolist() == [0, 50, 7]
    graph.reset()


# ---------------------------------------------------------------------------------------------------------------- 5. pictures
FRAMES = [0, 2, 6, 7, 9]


@pytest.fixture(scope="module")
def val_root(tmp_path_factory):
    r = write_tree(str(tmp_path_factory.mktemp("kitti_pictures")), tree_fixture(), images=True)
    open(os.path.join(r, "ImageSets", "val.txt"), "w").write("".join(f"{i:06d}\n" for i in FRAMES))
    return r


@pytest.fixture(scope="module")
def model3d():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(y3d.yaml_model_load("yolov10n_3D.yaml")).to(DEV)
    y3d.set_compute_dtype(before)
    return m


def _calibs(root, frames):
    P2 = [kitti.read_calib(os.path.join(root, "training/calib", f"{i:06d}.txt")) for i in frames]
    return [kitti.calib_params(P) for P in P2], P2


def _label_picture_ref(batch, c6, P2s, n):
    """draw_ref fed the restatement's rows: the wireframes in green under the 2D rectangles, thickness 2, in the network frame"""
    lab = {k: batch[k].cpu().numpy() for k in D.KEYS}
    B = len(batch["ori_shape"])
    counts_in = batch["counts"].cpu().numpy() if "counts" in batch else None
    rp = batch["ratio_pad"].cpu().numpy()
    ori = np.array([[float(s[0]), float(s[1])] for s in batch["ori_shape"]])
    R = len(lab["cls"]) // B if counts_in is not None else max(1, min(len(lab["cls"]), 50))
    rows, c3, _, counts = D.decode(lab, counts_in, ori, np.array(c6), rp, None, None, D.KITTI_MEAN, False, False, R)
    img = batch["img"].cpu().numpy()
    out = []
    for b in range(n):
        A = np.array([rp[b, 0, 0], 0.0, 0.0, 0.0, rp[b, 0, 1], 0.0])
        wire, wire_rgb, _ = DR.box_segments(c3[b], None, counts[b], np.asarray(P2s[b], np.float64).reshape(12), A, [(0, 255, 0)], 0.1)
        x1, y1, x2, y2 = (rows[b, :, c] for c in (2, 3, 4, 5))
        pts = [((A[0] * u + A[1] * v) + A[2], (A[3] * u + A[4] * v) + A[5]) for u, v in ((x1, y1), (x2, y1), (x2, y2), (x1, y2))]
        rect = np.stack([np.stack([pts[e][0], pts[e][1], pts[(e + 1) % 4][0], pts[(e + 1) % 4][1]], -1) for e in range(4)], 1)  # (R, 4, 4)
        rect[counts[b]:] = np.nan
        rect_rgb = np.tile(np.array([255, 89, 89, 0], np.uint8), (R * 4, 1))
        out.append(DR.paint_segments(img[b], np.concatenate([rect.reshape(-1, 4), wire]), np.concatenate([rect_rgb, wire_rgb]), 2))
    return np.stack(out), counts


@pytest.mark.parametrize("compact", [False, True])
def test_label_pictures_equal_the_restated_drawing(val_root, compact):
    c6, P2 = _calibs(val_root, FRAMES)
    batch = kitti.build_batch(val_root, list(range(len(FRAMES))), kitti.data_args(), DEV, mode="val", compact=compact, resolution=RES)
    before = batch["img"].clone()
    pics = plot.label_pictures(batch, c6, P2, max_imgs=3)
    assert pics.shape == (3, RES[1], RES[0], 3) and pics.dtype == torch.uint8 and pics.is_cuda
    assert torch.equal(batch["img"], before)  # the batch's own images are not painted
    want, counts = _label_picture_ref(batch, c6, P2, 3)
    got = pics.cpu().numpy()
    assert counts[:3].sum() > 0 and (got != before[:3].cpu().numpy()).any(), "nothing was drawn"
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"
    assert (got == np.array([0, 255, 0], np.uint8)).all(-1).any() and (got == np.array([255, 89, 89], np.uint8)).all(-1).any()
    assert plot.label_pictures(batch, c6, P2).shape[0] == len(FRAMES)  # fewer images than max_imgs: all of them


def test_validator_pictures(val_root, model3d):
    y3d.set_compute_dtype(torch.float32)
    plain = val.Validator3d(model3d, val_root, batch=2, conf=0.001, resolution=RES)
    res0 = plain()
    v = val.Validator3d(model3d, val_root, batch=2, conf=0.001, resolution=RES, pictures=2)
    res2 = v()
    assert plain.pictures == [] and len(v.pictures) == 2
    assert list(res0) == list(res2) and [float(res0[k]) for k in res0] == [float(res2[k]) for k in res2]
    assert v.results == plain.results and v.confusion_matrix.matrix.tobytes() == plain.confusion_matrix.matrix.tobytes()
    ms = _dev(np.asarray(D.KITTI_MEAN))
    model3d.eval()
    for n, entry in enumerate(v.pictures):
        idx = [2 * n, 2 * n + 1]
        assert sorted(entry) == ["bev", "labels", "preds"]
        c6, P2 = _calibs(val_root, [FRAMES[p] for p in idx])
        batch = kitti.build_batch(val_root, idx, kitti.data_args(), DEV, mode="val", compact=True, resolution=RES)
        assert np.array_equal(entry["labels"], plot.label_pictures(batch, c6, P2).cpu().numpy())
        assert entry["labels"].shape == entry["preds"].shape == (2, RES[1], RES[0], 3) and entry["bev"].shape == (2, 600, 1200, 3)
        assert all(e.dtype == np.uint8 for e in entry.values())
        # the other two pictures, stitched by hand from the calls they are made of: predictions at 0.1 under the labels' wireframes
        with torch.no_grad():
            raw = predict.raw_rows3d(model3d, batch["img"].permute(0, 3, 1, 2), 50)
        P = kitti.p2_device(P2, 2, DEV)
        prow, pc3, _, pcounts = predict.predict3d_rows(raw, _dev(np.array(c6)), P, batch["ratio_pad"], None, 0.1, None, ms)
        lrows, lc3, _, lcounts = kitti.decode_batch_device(batch, c6, None, False)
        A = plot.ratio_affine(batch["ratio_pad"])
        want = plot.draw_boxes3d(batch["img"].clone(), pc3, prow, pcounts, P, A)
        plot.draw_labels3d(want, lrows, lc3, lcounts, P, A, box2d=False)
        assert np.array_equal(entry["preds"], want.cpu().numpy())
        assert np.array_equal(entry["bev"], plot.draw_bev(pc3, prow, pcounts, gt=(lc3, lcounts)).cpu().numpy())
        assert (entry["preds"] != batch["img"].cpu().numpy()).any() and (entry["bev"] != entry["bev"][:, :1, :1]).any()
    model3d.train()
