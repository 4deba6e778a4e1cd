"""GPU: 2D training batches (yolo2d, csrc/yolo2d_batch.hip).  Labels against the reference's collated batches of
tests/golden/yolo2d_labels.npz, the static layout and its capacity, images against tests/yolo2d_ref.py bit for bit, a batch through the
2D loss at max_boxes = 128, and both kernels under graph capture.  imgsz = 64 (canvas 128 x 128), frames of up to 100 px."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yolo2d_ref as YR
import yolo2d_tree as T
from conftest import load_golden

import yolov10_3d_amd as y3d
from yolov10_3d_amd import loss as PL
from yolov10_3d_amd import yolo2d

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = T.IMGSZ
NAMES = list(T.ARGSETS)


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    from yolov10_3d_amd import ops
    before = ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


@pytest.fixture(scope="module")
def world():
    """label rows, their table on one start index per frame, the frames' pixels on the host and on the device"""
    rows = T.label_rows()
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])])[:-1]
    imgs = T.images()
    return SimpleNamespace(rows=rows, table=np.concatenate(rows), start={f: int(s) for f, s in enumerate(start)}, imgs=imgs,
                           dev=[torch.from_numpy(imgs[f]).to(DEV) for f in range(len(imgs))], split=SimpleNamespace(labels=rows))


def _labels(world, samples, max_boxes):
    li, lf = yolo2d.label_records(world.split, samples, world.start)
    return yolo2d.encode_labels(yolo2d.pack_labels(world.table, li, lf, DEV), S, max_boxes)


def _images(world, samples, mode):
    ri, rf, lut = yolo2d.image_records(samples, {f: f for f in range(len(world.dev))})
    return yolo2d.augment_images(yolo2d.pack_images(world.dev, ri, rf, lut, S, DEV), mode)


@pytest.mark.parametrize("name", NAMES)
def test_labels_match_the_reference(world, name):
    z = T.fixture()
    counts = z[f"{name}/counts"]
    samples = [T.sample(name, n) for n in range(len(counts))]
    cap = next(c for c in (64,) + PL.CROWDED_CAPS if c >= counts.max())
    max_boxes = None if cap == 64 else cap
    st = _labels(world, samples, max_boxes)
    assert st["counts"].dtype == torch.int32 and st["counts"].tolist() == list(counts)
    out = yolo2d.compact_labels(st, st["counts"].tolist(), max_boxes)
    for k in ("cls", "bboxes", "batch_idx"):
        want = torch.from_numpy(z[f"{name}/c/{k}"])
        assert out[k].dtype == want.dtype == torch.float32 and out[k].shape == want.shape, k
    assert torch.equal(out["cls"].cpu(), torch.from_numpy(z[f"{name}/c/cls"]))  # survivors and their order
    assert torch.equal(out["batch_idx"].cpu(), torch.from_numpy(z[f"{name}/c/batch_idx"]))
    np.testing.assert_allclose(out["bboxes"].cpu().numpy(), z[f"{name}/c/bboxes"], rtol=1e-6, atol=1e-6)


def test_static_layout_and_capacity(world):
    z = T.fixture()
    counts = z["default/counts"]
    n = next(i for i, c in enumerate(counts) if 64 < c <= 128)
    pick = [n, 3, n, 2]  # the crowded sample twice and two smaller ones
    samples = [T.sample("default", i) for i in pick]
    true = [int(counts[i]) for i in pick]
    ref_c, ref_b, _ = YR.labels(samples[0], world.rows, S)
    lo = _labels(world, samples, None)
    hi = _labels(world, samples, 128)
    for st, cap in ((lo, 64), (hi, 128)):
        assert st["cls"].shape == (4 * cap, 1) and st["bboxes"].shape == (4 * cap, 4) and st["batch_idx"].shape == (4 * cap,)
        assert st["counts"].tolist() == true  # the true count, also past the capacity
        for b, c in enumerate(true):
            used = min(c, cap)
            blk = slice(b * cap + used, (b + 1) * cap)
            assert (st["batch_idx"][b * cap:b * cap + used] == b).all() and (st["batch_idx"][blk] == -1).all()
            assert not st["cls"][blk].any() and not st["bboxes"][blk].any()
        assert torch.equal(st["cls"][:min(true[0], cap)].cpu(), torch.from_numpy(ref_c[:cap]))
        np.testing.assert_allclose(st["bboxes"][:min(true[0], cap)].cpu().numpy(), ref_b[:cap], rtol=1e-6, atol=1e-6)
    assert true[0] > 64 and torch.equal(lo["bboxes"][:64], hi["bboxes"][:64])  # the first 64 of the complete list
    full = yolo2d.compact_labels(hi, true, 128)
    assert int((full["batch_idx"] == 0).sum()) == true[0] == len(ref_b)
    cut = yolo2d.compact_labels(lo, true, None)
    assert int((cut["batch_idx"] == 0).sum()) == 64


def _scripted_pre(world_split, index, uniforms, args):
    """yolo2d._pre_transform with its `random.uniform` draws scripted (the three other tiles still come from the seeded buffer)"""
    it = iter(uniforms)
    orig = random.uniform
    random.uniform = lambda a, b: next(it)
    try:
        return yolo2d._pre_transform(world_split, index, world_split.load(index), args)
    finally:
        random.uniform = orig


def _image_cases(tmp_path):
    """one sample of each kind from the fixture, and hand-placed mosaics whose centre sits at (or next to) the canvas edge"""
    z = T.fixture()

    def find(name, ok):
        for n in range(len(z[f"{name}/counts"])):
            s = T.sample(name, n)
            if ok(s):
                return s
        raise AssertionError(f"no such sample in {name}")

    plain = lambda s: dict(s, hsv_u=None, hsv_gain=None, fliplr=False, flipud=False, rgb=True)
    cases = {
        "mosaic+mixup+hsv+fliplr": find("default", lambda s: s["mix"] and s["fliplr"] and s["pre"]["mosaic"] and s["hsv_gain"] is not None),
        "mosaic only": plain(find("nomixup", lambda s: s["pre"]["mosaic"])),
        "letter-box only": plain(find("nomosaic", lambda s: not s["mix"])),
        "letter-box + mixup + hsv": find("nomosaic", lambda s: s["mix"]),
        "rotation+shear": find("rotshear", lambda s: True),
        "flipud": find("flipud", lambda s: s["flipud"]),
        "bgr": dict(find("default", lambda s: not s["mix"]), rgb=False),
        "val": find("val", lambda s: s["pre"]["tiles"][0]["h0"] != s["pre"]["tiles"][0]["h"]),
    }
    sp = yolo2d.Split(T.write_tree(str(tmp_path), z["label_text"]), S, T.BATCH)
    random.seed(5)
    for i in range(12):
        sp.load(i)
    args = yolo2d.data_args()
    edge = {"centre xc = s//2": (70.3, S // 2 + 0.9, 0.7), "centre one pixel in": (1.0, 1.0, 0.5), "centre on the edge": (0.0, 2.0 * S, 0.5)}
    for tag, (yc, xc, sc) in edge.items():
        # angle 0, translate 0.5; at scale 0.5 the whole canvas lands on the output, every second pixel of it
        pre = _scripted_pre(sp, 4, [0.0, yc, xc, 0.0, 0.0, 0.0, sc, 0.0, 0.0, 0.5, 0.5], args)
        assert pre["mosaic"] and (pre["yc"], pre["xc"]) == (int(yc), int(xc))
        cases[tag] = dict(mode="train", index=4, pre=pre, pre2=None, mix=False, partner=-1, r=1.0, hsv_u=None, hsv_gain=None, flipud=False,
                          fliplr=False, rgb=True)
    t = cases["centre one pixel in"]["pre"]["tiles"]
    assert t[0]["x2a"] - t[0]["x1a"] == 1 and t[0]["y2a"] - t[0]["y1a"] == 1
    t = cases["centre on the edge"]["pre"]["tiles"]
    assert t[0]["y2a"] == t[0]["y1a"] and t[1]["x2a"] == t[1]["x1a"] and t[3]["x2a"] == t[3]["x1a"]  # empty rectangles
    return cases


def test_images_equal_the_reference_arithmetic(world, tmp_path):
    cases = _image_cases(tmp_path)
    samples = list(cases.values())
    want = [YR.image(s, world.imgs, S) for s in samples]
    assert any((w != 114).any() for w in want)
    u8 = _images(world, samples, "uint8")
    fl = _images(world, samples, "float")
    assert u8.shape == (len(samples), S, S, 3) and u8.dtype == torch.uint8 and fl.shape == (len(samples), 3, S, S) and fl.dtype == torch.float32
    u8, fl = u8.cpu().numpy(), fl.cpu().numpy()
    for n, (tag, w) in enumerate(zip(cases, want)):
        diff = int((u8[n] != w).sum())
        print(f"{tag}: {diff} of {w.size} values differ" + (f", largest {int(np.abs(u8[n].astype(int) - w).max())}" if diff else ""))
    for n, (tag, w) in enumerate(zip(cases, want)):
        assert np.array_equal(u8[n], w), tag
        assert np.array_equal(fl[n], YR.image_float(w)), tag
    # a resized tile really is interpolated, and the stages leave their mark
    assert not np.array_equal(want[0], want[1]) and len({w.tobytes() for w in want}) == len(want)


def _build(tmp_path, n_batches, **kw):
    z = T.fixture()
    mode, over, seed, items = T.ARGSETS["default"]
    sp = yolo2d.Split(T.write_tree(str(tmp_path), z["label_text"]), S, T.BATCH)
    random.seed(seed)
    np.random.seed(seed)
    return [yolo2d.build_batch(sp, items[4 * k:4 * k + 4], yolo2d.data_args(**over), DEV, **kw) for k in range(n_batches)]


def test_build_batch_through_the_loss(world, tmp_path):
    z = T.fixture()
    counts = [int(c) for c in z["default/counts"]]
    assert 64 < max(counts[:4]) <= 128 < max(counts[4:8])
    static = _build(tmp_path, 1, max_boxes=128, img_mode="float")[0]
    ragged = _build(tmp_path, 1, max_boxes=128, img_mode="float", compact=True)[0]
    assert set(static) == {"img", "cls", "bboxes", "batch_idx", "counts", "im_file", "ori_shape", "resized_shape"} == set(ragged)
    assert static["counts"].tolist() == counts[:4] and ragged["cls"].shape == (sum(counts[:4]), 1) and static["cls"].shape == (4 * 128, 1)
    assert torch.equal(static["img"], ragged["img"]) and static["img"].shape == (4, 3, S, S)
    assert static["ori_shape"] == [tuple(T.FRAME_WH[i][::-1]) for i in range(4)] and static["resized_shape"] == [(S, S)] * 4
    want = torch.stack([torch.from_numpy(YR.image_float(YR.image(T.sample("default", n), world.imgs, S))) for n in range(4)])
    assert torch.equal(static["img"].cpu(), want)
    u8 = _build(tmp_path, 1, max_boxes=128)[0]["img"]
    want8 = np.stack([YR.image(T.sample("default", n), world.imgs, S) for n in range(4)])
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), want8)

    y3d.set_compute_dtype(torch.float32)
    g = load_golden("e2e_tiny2d")
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=20, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    model = y3d.YOLOv10DetectionModel(cfg)
    model.load(g["state"])
    model = model.to(DEV).train()
    crit = PL.v10DetectLoss(model, max_boxes=128)
    PL.check_target_overflow(wait=True)
    preds = model(static["img"])
    items = []
    for batch in (static, ragged):
        _, it = crit(preds, batch)
        items.append(it.detach().float().cpu())
    PL.check_target_overflow(wait=True)  # 110 boxes in one image: quiet at 128
    assert items[0].shape == (6,) and torch.isfinite(items[0]).all() and torch.equal(items[0], items[1])
    # the over-128 sample: the static layout keeps its first 128 rows and shows the surplus in counts; its complete ragged list
    # overflows a loss built for 128
    second = _build(tmp_path, 2, max_boxes=128, img_mode="float")[1]
    assert second["counts"].tolist() == counts[4:8] and int((second["batch_idx"] >= 0).sum()) == sum(min(c, 128) for c in counts[4:8])
    crit(preds, second)
    PL.check_target_overflow(wait=True)
    over = _build(tmp_path, 2, max_boxes=192, img_mode="float", compact=True)[1]
    assert over["cls"].shape[0] == sum(counts[4:8])
    crit(preds, over)
    with pytest.raises(y3d.Y3DError, match=rf"{max(counts[4:8])} ground-truth boxes.*128 per image"):
        PL.check_target_overflow(wait=True)
    PL.check_target_overflow(wait=True)


def test_both_kernels_replay_under_capture(world):
    """recorded once, replayed with new record contents: the replay equals the eager result (default queue settings)"""
    table = {f: f for f in range(len(world.dev))}
    packs = []
    for first in (0, 4):
        samples = [T.sample("default", n) for n in range(first, first + 4)]
        ri, rf, lut = yolo2d.image_records(samples, table)
        li, lf = yolo2d.label_records(world.split, samples, world.start)
        packs.append((yolo2d.pack_images(world.dev, ri, rf, lut, S, DEV), yolo2d.pack_labels(world.table, li, lf, DEV)))
    keys_i, keys_l = ("rec_i", "rec_f", "lut"), ("lab_i", "lab_f")
    st_i = dict(packs[0][0], **{k: packs[0][0][k].clone() for k in keys_i})
    st_l = dict(packs[0][1], **{k: packs[0][1][k].clone() for k in keys_l})
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        yolo2d.augment_images(st_i, "uint8")
        yolo2d.encode_labels(st_l, S, 128)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img = yolo2d.augment_images(st_i, "uint8")
        lab = yolo2d.encode_labels(st_l, S, 128)
    pi, pl = packs[1]
    for k in keys_i:
        st_i[k].copy_(pi[k])
    for k in keys_l:
        st_l[k].copy_(pl[k])
    graph.replay()
    torch.cuda.synchronize()
    want_img, want_lab = yolo2d.augment_images(pi, "uint8"), yolo2d.encode_labels(pl, S, 128)
    first_img = yolo2d.augment_images(packs[0][0], "uint8")
    assert torch.equal(img, want_img) and not torch.equal(img, first_img)
    for k in want_lab:
        assert torch.equal(lab[k], want_lab[k]), k
    assert lab["counts"].tolist() == [int(c) for c in T.fixture()["default/counts"][4:8]]
    graph.reset()
