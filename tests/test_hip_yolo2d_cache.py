"""GPU: the 2D splits resident on the device (yolo2d.DeviceSplit / DeviceRectSplit, csrc/yolo2d_cache.hip).  The plan kernel against its
numpy restatement (tests/yolo2d_cache_ref.py) bit for bit with guard rows on both sides, and against the host functions it replaces;
the cached `build_batch` against the path-based one, tensor for tensor, over three consecutive batches for every recorded argument
set, both image modes, both label layouts and both capacities; no file access after the load; the byte budget; the pinned ring under
reuse; the three launches under graph capture; every rect batch and `val.Validator2d` on a resident rect split.  imgsz = 64, the
twelve-frame tree of tests/yolo2d_tree.py."""
import builtins
import os
import random
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yolo2d_cache_ref as R
import yolo2d_tree as T
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import ops as P_ops  # noqa: E402
from yolov10_3d_amd import val, yolo2d  # noqa: E402
from yolov10_3d_amd._lib import Y3DError  # noqa: E402

DEV = "cuda"
S = T.IMGSZ
NAMES = list(T.ARGSETS)
N = len(T.FRAME_WH)
GUARD, SENTINEL = 2, 0xA5
BLANK = 3  # the frame without a label file in the second tree
ZR = dict(np.load(os.path.join(GOLDEN, "yolo2d_rect.npz")))
R_IMGSZ, R_STRIDE, R_PAD = int(ZR["imgsz"]), int(ZR["stride"]), float(ZR["pad"])


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    before = P_ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


@pytest.fixture(scope="module")
def img_dir(tmp_path_factory):
    return T.write_tree(str(tmp_path_factory.mktemp("yolo2d_cache")), T.fixture()["label_text"])


@pytest.fixture(scope="module")
def blank_dir(tmp_path_factory):
    text = T.fixture()["label_text"].copy()
    text[BLANK] = ""
    d = T.write_tree(str(tmp_path_factory.mktemp("yolo2d_cache_blank")), text)
    assert not os.path.exists(yolo2d.img2label_path(os.path.join(d, f"{BLANK:06d}.png")))
    return d


@pytest.fixture(scope="module")
def split(img_dir):
    """a resident training split for the kernel tests (they do not go through its buffer)"""
    return yolo2d.DeviceSplit(img_dir, S, T.BATCH, device=DEV)


@pytest.fixture(scope="module")
def host(img_dir):
    """a plain Split with all twelve frames in its buffer, for scripted draws"""
    sp = yolo2d.Split(img_dir, S, T.BATCH)
    for i in range(N):
        sp.load(i)
    return sp


def need_bytes():
    return sum((w * h * 3 + 15) // 16 * 16 for w, h in T.FRAME_WH)


# ------------------------------------------------------------------------------------------------------------ the split's tables
def test_split_tables(img_dir, split):
    rows = T.label_rows()
    assert len(split) == N and split.nbytes == need_bytes() == split.arena.numel() and split.device == torch.device("cuda", torch.cuda.current_device())
    assert split.arena.dtype == torch.uint8 and split.arena.data_ptr() % 16 == 0
    off, hw, span, src = split.img_off.cpu().numpy(), split.frame_hw.cpu().numpy(), split.rec_span.cpu().numpy(), split.src.cpu().numpy()
    assert off.dtype == src.dtype == np.int64 and hw.dtype == span.dtype == np.int32 and (off % 16 == 0).all()
    assert (src == split.arena.data_ptr() + off).all() and split.rec.dtype == torch.float32 and split.rec.shape == (sum(len(r) for r in rows), 5)
    assert split.n_rec == split.rec.shape[0]
    rec, row = split.rec.cpu().numpy(), 0
    for pos, (W, H) in enumerate(T.FRAME_WH):
        assert tuple(hw[pos]) == (H, W) == split.size(pos) and (pos == 0 or off[pos] >= off[pos - 1] + hw[pos - 1].prod() * 3)
        assert tuple(span[pos]) == (row, len(rows[pos])) and rec[row:row + len(rows[pos])].tobytes() == rows[pos].tobytes()
        row += len(rows[pos])
        want = torch.from_numpy(T.frame_pixels(pos, W, H))
        assert torch.equal(split.frame(pos).cpu(), want) and torch.equal(split.decode(pos, DEV).cpu(), want)
        assert split.decode(pos, DEV).data_ptr() == src[pos]
    assert split.im_files == yolo2d.Split(img_dir, S, T.BATCH).im_files


def test_split_without_any_label(tmp_path):
    d = T.write_tree(str(tmp_path), [""] * 3, T.FRAME_WH[:3])
    sp = yolo2d.DeviceSplit(d, S, 4, augment=False, device=DEV)
    assert sp.n_rec == 0 and sp.rec.shape == (1, 5) and not sp.rec_span.cpu().numpy().any()
    random.seed(1)
    got = sp.build_batch([0, 1, 2], yolo2d.data_args(), mode="val")
    random.seed(1)
    same_batch(got, yolo2d.build_batch(yolo2d.Split(d, S, 4, augment=False), [0, 1, 2], yolo2d.data_args(), DEV, mode="val"))
    assert got["counts"].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ the plan kernel
def guarded_plan(split, draws):
    """the plan kernel into buffers with GUARD sentinel rows before and behind the B rows it may write -> (the B rows, the buffers)"""
    B = len(draws)
    bufs = {}
    for k, dt, s in yolo2d.PLAN_TABLES:
        bufs[k] = torch.empty(B + 2 * GUARD, *s, dtype=dt, device=DEV)
        bufs[k].view(torch.uint8).fill_(SENTINEL)
    views = {k: t[GUARD:] for k, t in bufs.items()}
    try:
        out = yolo2d.plan_batch(split, draws, out=views)
        assert all(out[k] is views[k] for k in views)
    finally:
        torch.cuda.synchronize()
        for k, t in bufs.items():
            for guard in (t[:GUARD], t[GUARD + B:]):
                assert bool((guard.contiguous().view(torch.uint8) == SENTINEL).all()), f"{k}: a guard row was written"
    return {k: t[GUARD:GUARD + B].cpu().numpy() for k, t in bufs.items()}, bufs


def check_plan(split, draws):
    got, _ = guarded_plan(split, draws)
    want = R.plan(split.frame_hw.cpu().numpy(), split.rec_span.cpu().numpy(), split.imgsz, draws)
    for k, dt, s in R.OUTPUTS:
        assert got[k].dtype == dt and got[k].shape == want[k].shape == (len(draws),) + s, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.argwhere(got[k] != want[k])[:8])
    return got


def check_samples(split, samples):
    """kernel == restatement == the host functions, slots and label rows split-wide"""
    got = check_plan(split, yolo2d.draw_table(samples))
    span = split.rec_span.cpu().numpy()
    ri, rf, lut = yolo2d.image_records(samples, {f: f for f in range(len(split))})
    li, lf = yolo2d.label_records(split, samples, {f: int(span[f, 0]) for f in range(len(split))})
    for k, w in (("rec_i", ri), ("rec_f", rf), ("lut", lut), ("lab_i", li), ("lab_f", lf)):
        assert got[k].tobytes() == w.tobytes(), (k, np.argwhere(got[k] != w)[:8])
    return got


def scripted_pre(sp, index, uniforms, others=None, args=None):
    """yolo2d._pre_transform with its `random.uniform` draws (and optionally the three other tiles) scripted"""
    it = iter(uniforms)
    orig_u, orig_c = random.uniform, random.choices
    random.uniform = lambda a, b: next(it)
    if others is not None:
        random.choices = lambda population, k: list(others)
    try:
        return yolo2d._pre_transform(sp, index, sp.load(index), args or yolo2d.data_args())
    finally:
        random.uniform, random.choices = orig_u, orig_c


def mosaic_pre(sp, index, others, yc, xc, angle=0.0, scale=1.0, args=None):
    pre = scripted_pre(sp, index, [0.0, yc, xc, 0.0, 0.0, angle, scale, 0.0, 0.0, 0.5, 0.5], others, args)
    assert pre["mosaic"] and (pre["yc"], pre["xc"]) == (int(yc), int(xc)) and [t["frame"] for t in pre["tiles"]] == [index] + list(others)
    return pre


def plain_pre(sp, index, scale=1.0):
    pre = scripted_pre(sp, index, [2.0, 0.0, 0.0, 0.0, scale, 0.0, 0.0, 0.45, 0.55])
    assert not pre["mosaic"] and len(pre["tiles"]) == 1 and pre["warp"]
    return pre


def sample_of(pre, pre2=None, r=1.0, gain=None, flipud=False, fliplr=False, rgb=True, mode="train"):
    return dict(mode=mode, index=pre["index"], pre=pre, pre2=pre2, mix=pre2 is not None, partner=-1 if pre2 is None else pre2["index"], r=r,
                hsv_u=None if gain is None else np.zeros(3), hsv_gain=None if gain is None else np.asarray(gain, np.float64), flipud=flipud,
                fliplr=fliplr, rgb=rgb)


def test_plan_letter_box_only(split, host):
    got = check_samples(split, [sample_of(plain_pre(host, 0))])
    assert got["rec_i"][0, 0] == 1 and got["rec_i"][0, 1] == S and got["rec_i"][0, 50] == 0 and not got["lut"].any()
    assert got["lab_i"][0, 16] == 5 and got["lab_i"][0, 17] == 0


def test_plan_mosaic_with_a_mosaic_partner(split, host):
    s = sample_of(mosaic_pre(host, 1, [5, 6, 10], 70.3, 51.9, 3.0, 1.2), mosaic_pre(host, 7, [0, 2, 9], 40.0, 90.5, -2.0, 0.8), r=0.4371,
                  gain=(1.01, 0.6, 1.3), fliplr=True)
    got = check_samples(split, [s])
    assert got["rec_i"][0, 0] == got["rec_i"][0, 50] == 4 and got["rec_i"][0, 1] == got["rec_i"][0, 51] == 2 * S
    assert got["rec_i"][0, [2, 14, 26, 38, 52, 64, 76, 88]].tolist() == [1, 5, 6, 10, 7, 0, 2, 9]
    assert got["lab_i"][0, 16:19].tolist() == [7, 7, 2] and got["rec_i"][0, 100:105].tolist() == [0, 1, 0, 1, 1]


def test_plan_mosaic_centre_on_and_next_to_the_canvas_edge(split, host):
    edge = sample_of(mosaic_pre(host, 4, [0, 5, 11], 0.0, 2.0 * S, 0.0, 0.5))
    t = edge["pre"]["tiles"]
    assert t[0]["y2a"] == t[0]["y1a"] and t[1]["x2a"] == t[1]["x1a"] and t[3]["x2a"] == t[3]["x1a"]  # three empty rectangles
    one = sample_of(mosaic_pre(host, 4, [0, 5, 11], 1.0, 1.0, 0.0, 0.5))
    t = one["pre"]["tiles"]
    assert t[0]["x2a"] - t[0]["x1a"] == 1 and t[0]["y2a"] - t[0]["y1a"] == 1  # a 1 x 1 tile
    far = sample_of(mosaic_pre(host, 10, [11, 0, 1], 2.0 * S - 1.0, 2.0 * S - 1.0))
    got = check_samples(split, [edge, one, far])
    assert got["rec_i"][1, 2 + 5:2 + 9].tolist() == [0, 0, 1, 1]


def test_plan_one_frame_in_several_tiles_and_the_last_frame(split, host):
    last = N - 1
    rep = sample_of(mosaic_pre(host, 4, [4, 4, last], 60.0, 66.0), mosaic_pre(host, last, [last, 4, last], 80.0, 30.0), r=0.5)
    got = check_samples(split, [rep, sample_of(plain_pre(host, last, 0.9)), rep])
    span = split.rec_span.cpu().numpy()
    assert got["rec_i"][0, [2, 14, 26, 38]].tolist() == [4, 4, 4, last] and got["rec_i"][1, 2] == last
    assert got["lab_i"][1, 0] + got["lab_i"][1, 1] == span[last].sum() == split.n_rec  # its rows are the last ones
    assert got["rec_i"][0].tobytes() == got["rec_i"][2].tobytes()


def test_plan_frame_without_label_rows(blank_dir):
    sb = yolo2d.DeviceSplit(blank_dir, S, T.BATCH, device=DEV)
    hb = yolo2d.Split(blank_dir, S, T.BATCH)
    for i in range(N):
        hb.load(i)
    span = sb.rec_span.cpu().numpy()
    assert span[BLANK, 1] == 0 and span[BLANK, 0] == span[BLANK + 1, 0] and len(sb.labels[BLANK]) == 0
    got = check_samples(sb, [sample_of(plain_pre(hb, BLANK)), sample_of(mosaic_pre(hb, 2, [BLANK, 8, BLANK], 64.0, 64.0))])
    assert got["lab_i"][0, 1] == 0 and got["lab_i"][1, 3] == 0 and got["lab_i"][1, 7] == 0 and got["lab_i"][1, 1] > 0


def test_plan_val_rows(img_dir, split):
    hv = yolo2d.Split(img_dir, S, T.BATCH, augment=False)
    samples = []
    for i in (0, 2, 3, 11):  # larger than, equal to and smaller than imgsz
        pre = yolo2d._letterbox_only(hv, i, hv.load(i))
        samples.append(sample_of(pre, mode="val"))
    got = check_samples(split, samples)
    assert (got["lab_i"][:, 16] == 1).all() and not got["lut"].any() and (got["rec_i"][:, 0] == 1).all()
    assert got["rec_i"][1, 2:13].tolist() == [2, 64, 64, 64, 64, 0, 0, 64, 64, 0, 0]


@pytest.mark.parametrize("sign", [1.0, -1.0, 0.0])
def test_plan_hsv_tables_at_the_ends_of_the_gains(split, host, sign):
    a = yolo2d.DATA_ARGS
    gain = 1.0 + sign * np.array([a["hsv_h"], a["hsv_s"], a["hsv_v"]])
    pre = plain_pre(host, 5)
    got = check_samples(split, [sample_of(pre, gain=gain), sample_of(pre), sample_of(pre, gain=gain * 0.999)])
    assert got["rec_i"][:, 103].tolist() == [1, 0, 1] and got["lut"][0].tobytes() == yolo2d.hsv_luts(gain).tobytes() and not got["lut"][1].any()
    assert got["lut"][0, 0, 255] == int((255 * gain[0]) % 180)


@pytest.mark.parametrize("name", NAMES)
def test_plan_recorded_samples(split, name):
    check_samples(split, [T.sample(name, n) for n in range(len(T.fixture()[f"{name}/counts"]))])


def test_plan_more_samples_than_one_workgroup_holds_of_anything(split):
    pool = [T.sample(name, n) for name in NAMES for n in range(len(T.fixture()[f"{name}/counts"]))]
    samples = [pool[(7 * i) % len(pool)] for i in range(130)]
    check_samples(split, samples)


def test_plan_refuses_bad_draws(split, host):
    ok = yolo2d.draw_table([sample_of(plain_pre(host, 0)), sample_of(mosaic_pre(host, 1, [5, 6, 10], 70.0, 51.0), mosaic_pre(host, 7, [0, 2, 9], 40.0, 90.0), r=0.5)])
    for row, col, value in ((0, 3, N), (0, 3, -1), (1, 3, 0.5), (1, 6, N), (1, 23 + 4, -1), (1, 23 + 3, N)):
        bad = ok.copy()
        bad[row, col] = value
        with pytest.raises(Y3DError, match="position"):
            guarded_plan(split, bad)  # (its guard check runs on the way out)
        bufs = {k: torch.full((2, *s), 0, dtype=dt, device=DEV) for k, dt, s in yolo2d.PLAN_TABLES}
        for t in bufs.values():
            t.view(torch.uint8).fill_(SENTINEL)
        with pytest.raises(Y3DError, match="position"):
            yolo2d.plan_batch(split, bad, out=bufs)
        torch.cuda.synchronize()
        assert all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in bufs.values())  # nothing was launched
    unused = ok.copy()
    unused[0, 4:7] = N  # tiles 1..3 of a letter-box sample are not read
    check_plan(split, unused)
    none = ok.copy()
    none[0, 0] = 0
    with pytest.raises(Y3DError, match="primary"):
        yolo2d.plan_batch(split, none)
    with pytest.raises(Y3DError, match="B = 0"):
        yolo2d.plan_batch(split, np.zeros((0, yolo2d._DRAW_W), np.float64))
    with pytest.raises(Y3DError):
        yolo2d.plan_batch(split, ok.astype(np.float32))
    with pytest.raises(Y3DError, match="null"):
        y3d.lib().yolo2d_plan_batch(None, None, N, S, None, None, 1, None, None, None, None, None, None)
    check_plan(split, ok)  # and the table itself is fine


def test_split_on_another_device_index_raises(split):
    args = yolo2d.data_args()
    with pytest.raises(Y3DError, match="lives on"):
        split.check_device(f"cuda:{split.device.index + 1}")
    with pytest.raises(Y3DError, match="lives on"):
        yolo2d.build_batch(split, [0], args, f"cuda:{split.device.index + 1}")
    with pytest.raises(Y3DError, match="lives on"):
        split.decode(0, f"cuda:{split.device.index + 1}")
    with pytest.raises(Y3DError):
        yolo2d.build_batch(split, [0], args, "cpu")
    split.check_device("cuda")
    split.check_device(split.device)


# ------------------------------------------------------------------------------------------------------------ end to end
def same_batch(got, want):
    assert list(got) == list(want)
    for k, w in want.items():
        g = got[k]
        if torch.is_tensor(w):
            assert torch.is_tensor(g) and g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (k, g.dtype, w.dtype, g.shape, w.shape)
            assert torch.equal(g, w), k
        else:
            assert type(g) is list and g == w and [type(v) for v in g] == [type(v) for v in w], k


def seed(n):
    random.seed(n)
    np.random.seed(n)


def rng_state():
    return random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2]


def three_batches(name):
    mode, over, sd, items = T.ARGSETS[name]
    return mode, yolo2d.data_args(**over), sd, [[int(i) for i in c] for c in np.array_split(np.array(items), 3)]


def both(img_dir, name, **kw):
    """three consecutive batches from a fresh path-based Split and from a fresh resident one, under the same seeds"""
    mode, args, sd, chunks = three_batches(name)
    plain = yolo2d.Split(img_dir, S, T.BATCH, augment=mode == "train")
    seed(sd)
    want = [yolo2d.build_batch(plain, c, args, DEV, mode=mode, **kw) for c in chunks]
    after = rng_state()
    res = yolo2d.DeviceSplit(img_dir, S, T.BATCH, augment=mode == "train", device=DEV)
    seed(sd)
    got = [res.build_batch(c, args, mode=mode, **kw) for c in chunks]
    now = rng_state()
    assert now[0] == after[0] and np.array_equal(now[1], after[1]) and now[2] == after[2]  # the same draws were consumed
    assert res.buffer == plain.buffer and res._held == plain._held
    return got, want


@pytest.mark.parametrize("max_boxes", [None, 128])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("img_mode", ["uint8", "float"])
@pytest.mark.parametrize("name", NAMES)
def test_cached_batch_equals_the_path_based_batch(img_dir, name, img_mode, compact, max_boxes):
    got, want = both(img_dir, name, img_mode=img_mode, compact=compact, max_boxes=max_boxes)
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        same_batch(g, w)
        assert g["img"].dtype == (torch.uint8 if img_mode == "uint8" else torch.float32)
        assert list(g) == ["img", "im_file", "ori_shape", "resized_shape", "counts", "cls", "bboxes", "batch_idx"]
    if name == "default" and not compact:
        assert got[0]["counts"].tolist() == [int(c) for c in T.fixture()["default/counts"][:len(got[0]["im_file"])]]


def test_build_batch_dispatches_and_the_host_built_path_runs_on_the_arena(img_dir):
    mode, args, sd, chunks = three_batches("default")
    a, b, c = (yolo2d.DeviceSplit(img_dir, S, T.BATCH, device=DEV) for _ in range(3))
    seed(sd)
    want = a.build_batch(chunks[0], args, mode=mode, compact=True, img_mode="float", max_boxes=128)
    seed(sd)
    same_batch(yolo2d.build_batch(b, chunks[0], args, DEV, mode=mode, compact=True, img_mode="float", max_boxes=128), want)
    seed(sd)
    same_batch(yolo2d._build_square_batch(c, chunks[0], args, DEV, mode, 128, True, "float"), want)
    with pytest.raises(Y3DError, match="augment"):
        a.build_batch([0], args, mode="val")
    with pytest.raises(IndexError):
        a.build_batch([N], args)
    with pytest.raises(Y3DError, match="empty"):
        a.build_batch([], args)
    with pytest.raises(ValueError):
        a.build_batch([0], args, img_mode="half")
    with pytest.raises(Y3DError, match="copy_paste"):
        a.build_batch([0], yolo2d.data_args(copy_paste=0.5))


def test_epoch_yields_every_frame_once(img_dir):
    from yolov10_3d_amd import kitti
    sp = yolo2d.DeviceSplit(img_dir, S, T.BATCH, augment=False, device=DEV)
    args = yolo2d.data_args()
    seed(1)
    seen = [f for b in sp.epoch(5, args, mode="val", shuffle=True, seed=2) for f in b["im_file"]]
    assert sorted(seen) == sp.im_files and seen == [sp.im_files[i] for idx in kitti.epoch_indices(N, 5, seed=2) for i in idx]
    assert [b["img"].shape[0] for b in sp.epoch(5, args, mode="val", drop_last=True, img_mode="float")] == [5, 5]


def test_no_file_access_after_the_load(tmp_path, img_dir, monkeypatch):
    from PIL import Image
    r = os.path.join(str(tmp_path), "tree")
    shutil.copytree(os.path.dirname(img_dir), r)
    d = os.path.join(r, "images")
    mode, args, sd, chunks = three_batches("default")
    vmode, vargs, vsd, vchunks = three_batches("val")
    plain, plain_val = yolo2d.Split(d, S, T.BATCH), yolo2d.Split(d, S, T.BATCH, augment=False)
    rect = yolo2d.RectSplit(d, R_IMGSZ, 5, R_STRIDE, R_PAD)
    seed(sd)
    wants = [yolo2d.build_batch(plain, c, args, DEV, mode=mode) for c in chunks]
    want_val = yolo2d.build_batch(plain_val, vchunks[0], vargs, DEV, mode="val", compact=True)
    want_rect = [yolo2d.build_batch(rect, items, vargs, DEV, mode="val") for items in rect.batches()]
    res = yolo2d.DeviceSplit(d, S, T.BATCH, device=DEV, workers=3)
    res_val = yolo2d.DeviceSplit(d, S, T.BATCH, augment=False, device=DEV)
    res_rect = yolo2d.DeviceRectSplit(d, R_IMGSZ, 5, R_STRIDE, R_PAD, device=DEV)
    yolo2d.DeviceSplit(d, S, T.BATCH, device=DEV).build_batch(chunks[0], args)  # every lazy import has happened
    shutil.rmtree(r)
    assert not os.path.exists(r)

    def refuse(*a, **k):
        raise AssertionError(f"a file was opened: {a[:1]}")

    with monkeypatch.context() as m:
        m.setattr(builtins, "open", refuse)
        m.setattr(Image, "open", refuse)
        seed(sd)
        gots = [res.build_batch(c, args, mode=mode) for c in chunks]
        got_val = yolo2d.build_batch(res_val, vchunks[0], vargs, DEV, mode="val", compact=True)
        got_rect = [yolo2d.build_batch(res_rect, items, vargs, DEV, mode="val") for items in res_rect.batches()]
        fallback = yolo2d._build_rect_batch(res_rect, res_rect.batches()[0], vargs, DEV, "val", None, False, "uint8")
    for g, w in zip(gots + [got_val] + got_rect + [fallback], wants + [want_val] + want_rect + [want_rect[0]]):
        same_batch(g, w)


def test_byte_budget(img_dir):
    need = need_bytes()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for cls, a in ((yolo2d.DeviceSplit, (S, T.BATCH)), (yolo2d.DeviceRectSplit, (R_IMGSZ, 5, R_STRIDE, R_PAD))):
        with pytest.raises(Y3DError, match=f"{need} bytes.* {need - 1} bytes"):
            cls(img_dir, *a, device=DEV, max_bytes=need - 1)
        assert torch.cuda.memory_allocated() == before
        sp = cls(img_dir, *a, device=DEV, max_bytes=need)  # exactly enough
        assert sp.nbytes == need == sp.arena.numel() and torch.cuda.memory_allocated() >= before + need
        del sp


def test_ring_reuse_without_synchronising(img_dir):
    mode, args, _, _ = three_batches("default")
    items = [0, 4, 9, 6, 11]
    n = 2 * yolo2d.DeviceSplit.RING + 1
    res = yolo2d.DeviceSplit(img_dir, S, T.BATCH, device=DEV)
    got = []
    for k in range(n):  # more builds in flight than the ring has buffers, nothing waits in between
        seed(1000 + k)
        got.append(res.build_batch(items, args, mode=mode))
    assert len({g["bboxes"].cpu().numpy().tobytes() for g in got}) > yolo2d.DeviceSplit.RING  # the draws differ, so a stale table would show
    plain = yolo2d.Split(img_dir, S, T.BATCH)
    for k in range(n):
        seed(1000 + k)
        same_batch(got[k], yolo2d.build_batch(plain, items, args, DEV, mode=mode))


def test_three_launches_replay_under_capture(split):
    """recorded once on static tensors, replayed with new draw tables copied in: each replay equals the eager build (default queue settings)"""
    groups = [[T.sample("default", n) for n in range(first, first + 4)] for first in (0, 4, 8)]
    tables = [yolo2d.draw_table(g) for g in groups]

    def eager(d):
        p = yolo2d.plan_batch(split, d)
        img = yolo2d.augment_images({"src": split.src, "rec_i": p["rec_i"], "rec_f": p["rec_f"], "lut": p["lut"], "imgsz": S}, "uint8")
        return img, yolo2d.encode_labels({"rec": split.rec, "n_rec": split.n_rec, "lab_i": p["lab_i"], "lab_f": p["lab_f"]}, S, 128)

    wants = [eager(d) for d in tables]
    # ... and the eager build is the path-based one: the host records over the same frames
    frames = [split.frame(f) for f in range(N)]
    ri, rf, lut = yolo2d.image_records(groups[1], {f: f for f in range(N)})
    assert torch.equal(wants[1][0], yolo2d.augment_images(yolo2d.pack_images(frames, ri, rf, lut, S, DEV), "uint8"))
    assert wants[1][1]["counts"].tolist() == [int(c) for c in T.fixture()["default/counts"][4:8]]
    host0 = torch.from_numpy(tables[0])
    static = host0.to(DEV)
    out = {k: torch.empty(4, *s, dtype=dt, device=DEV) for k, dt, s in yolo2d.PLAN_TABLES}

    def launches():
        p = yolo2d.plan_batch(split, host0, static, out)
        img = yolo2d.augment_images({"src": split.src, "rec_i": p["rec_i"], "rec_f": p["rec_f"], "lut": p["lut"], "imgsz": S}, "uint8")
        return img, yolo2d.encode_labels({"rec": split.rec, "n_rec": split.n_rec, "lab_i": p["lab_i"], "lab_f": p["lab_f"]}, S, 128)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        launches()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img, lab = launches()
    for d, (want_img, want_lab) in zip(tables[1:], wants[1:]):
        static.copy_(torch.from_numpy(d))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(img, want_img) and not torch.equal(img, wants[0][0])
        for k in want_lab:
            assert torch.equal(lab[k], want_lab[k]), k
    graph.reset()


# ------------------------------------------------------------------------------------------------------------ the rect split
@pytest.mark.parametrize("name", [str(n) for n in ZR["rect_sets"]])
def test_every_rect_batch_equals_the_path_based_one(img_dir, name):
    batch = int(ZR[f"{name}/batch"])
    plain = yolo2d.RectSplit(img_dir, R_IMGSZ, batch, R_STRIDE, R_PAD)
    state = random.getstate()
    res = yolo2d.DeviceRectSplit(img_dir, R_IMGSZ, batch, R_STRIDE, R_PAD, device=DEV)
    assert random.getstate() == state  # the load leaves the generator alone
    assert res.im_files == plain.im_files and res.batches() == plain.batches() and np.array_equal(res.batch_shapes, plain.batch_shapes)
    assert res.lb_rec.shape == (N, 8) and res.lb_lab_i.shape == (N, 2) and res.lb_lab_f.shape == (N, 4)
    args = yolo2d.data_args()
    for kw in (dict(), dict(compact=True, img_mode="float"), dict(max_boxes=128, img_mode="float"), dict(compact=True, max_boxes=128)):
        for items in plain.batches():
            random.seed(7)
            want = yolo2d.build_batch(plain, items, args, DEV, mode="val", **kw)
            after = random.getstate()
            random.seed(7)
            got = yolo2d.build_batch(res, items, args, DEV, mode="val", **kw)
            assert random.getstate() == after
            same_batch(got, want)
            assert list(got) == ["img", "im_file", "ori_shape", "resized_shape", "ratio_pad", "counts", "cls", "bboxes", "batch_idx"]
    # a part of a batch, and an order no run of positions gives (the host-built path over the arena)
    items = plain.batches()[0]
    for pick in (items[1:], items[::-1], [items[0], items[0]]):
        same_batch(yolo2d.build_batch(res, pick, args, DEV, mode="val"), yolo2d.build_batch(plain, pick, args, DEV, mode="val"))
    with pytest.raises(Y3DError, match="validation batches only"):
        res.build_batch(items, args, mode="train")
    if len(plain.batches()) > 1:
        with pytest.raises(Y3DError, match="one shape"):
            res.build_batch(items + plain.batches()[1], args)
    with pytest.raises(Y3DError, match="empty"):
        res.build_batch([], args)


def _prime(m, shape):
    """as tests/test_hip_validators.py: BatchNorm statistics of a random batch and wider random score projections"""
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    keep = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m.train()(torch.rand(*shape, device=DEV))
        for level in m.model[-1].one2one_cv3:
            level[-1].weight.normal_(0.0, 0.05)
            level[-1].bias.add_(torch.randn_like(level[-1].bias))
    for b, mom in zip(bns, keep):
        b.momentum = mom
    P_ops.bump_param_epoch()
    return m


def test_validator2d_on_a_resident_rect_split(img_dir):
    y3d.set_compute_dtype(torch.float32)
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=20, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    torch.manual_seed(3)
    model = _prime(y3d.YOLOv10DetectionModel(cfg).to(DEV), (4, 3, R_IMGSZ, R_IMGSZ)).train()
    plain = yolo2d.RectSplit(img_dir, R_IMGSZ, 5, R_STRIDE, R_PAD)
    res = yolo2d.DeviceRectSplit(img_dir, R_IMGSZ, 5, R_STRIDE, R_PAD, device=DEV)
    va, vb = val.Validator2d(model, res, max_det=40), val.Validator2d(model, plain, max_det=40)
    a, b = va(), vb()
    assert list(a) == list(b) and len(a) >= 6 and all(float(a[k]) == float(b[k]) for k in a), (a, b)
    assert va.seen == vb.seen == N and np.array_equal(va.nt_per_class, vb.nt_per_class) and va.nt_per_class.sum() > 0
    assert np.array_equal(np.asarray(va.confusion_matrix.matrix), np.asarray(vb.confusion_matrix.matrix))
