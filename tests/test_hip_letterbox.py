"""GPU: rectangular letter-boxing (csrc/letterbox.hip) — the image kernel against tests/letterbox_ref.py bit for bit, the rect
validation labels against the reference's collated batches (tests/golden/yolo2d_rect.npz), the predictor's row kernel against the
reference's scale_boxes output and a float32 numpy restatement, and end to end: rect batches through a tiny v10 model and
`BoxStats.update_2d`, `predict.Predictor`, and the launches under graph capture.  imgsz = 64, canvases of at most 96 x 96."""
import os
import random

import numpy as np
import pytest
import torch

import letterbox_ref as LR
import yolo2d_tree as T
from conftest import GOLDEN

import yolov10_3d_amd as y3d
from yolov10_3d_amd import metrics, predict, yolo2d
from yolov10_3d_amd import ops as P_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z = dict(np.load(os.path.join(GOLDEN, "yolo2d_rect.npz")))
IMGSZ, STRIDE, PAD = int(Z["imgsz"]), int(Z["stride"]), float(Z["pad"])
NC = 20


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    before = P_ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


@pytest.fixture(scope="module")
def img_dir(tmp_path_factory):
    return T.write_tree(str(tmp_path_factory.mktemp("rect")), T.fixture()["label_text"])


@pytest.fixture(scope="module")
def model():
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=NC, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    torch.manual_seed(3)
    m = y3d.YOLOv10DetectionModel(cfg).to(DEV)
    # At the default initialisation (BatchNorm statistics 0 / 1) this narrow model's features die out with depth: the class logits are
    # the biases to float32 precision, every score of a level is the same number and no threshold separates them.  One training-mode
    # forward with momentum 1 gives every BatchNorm the statistics of a random batch, and wider random class projections (std 0.05, same seed)
    # spread the scores.
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert bns
    keep = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m.train()(torch.rand(4, 3, IMGSZ, IMGSZ, device=DEV))
        for head in m.model[-1].one2one_cv3:
            head[-1].weight.normal_(0.0, 0.05)
            head[-1].bias.add_(torch.randn_like(head[-1].bias))
    for b, mom in zip(bns, keep):
        b.momentum = mom
    P_ops.bump_param_epoch()
    return m.eval()


def _split(img_dir, name):
    return yolo2d.RectSplit(img_dir, IMGSZ, int(Z[f"{name}/batch"]), STRIDE, PAD)


# ---------------------------------------------------------------------------------------------------------------- the image kernel
def _src(i, h, w):
    return T.frame_pixels(i, w, h)


# canvas (H, W) -> sources [(h0, w0)] and records [src, h0, w0, new_h, new_w, top, left, swap_rb]
IMAGE_CASES = {
    # copy path with odd pads, left and new_w no multiples of 4 | down-scale, BGR -> RGB | up-scale x 1.6
    (64, 96): ([(59, 91), (100, 60), (20, 30)], [[0, 59, 91, 59, 91, 2, 3, 0], [1, 100, 60, 64, 38, 0, 29, 1], [2, 20, 30, 32, 48, 16, 24, 0]]),
    # zero pad: the image fills the canvas | a 1 x 7 source | a 7 x 1 source
    (96, 64): ([(96, 64), (1, 7), (7, 1)], [[0, 96, 64, 96, 64, 0, 0, 1], [1, 1, 7, 9, 63, 43, 0, 0], [2, 7, 1, 96, 14, 0, 25, 0]]),
    # down-scale with the image edge inside a thread's four pixels | a bad record (source index = n_src) | copy, swapped
    (32, 32): ([(40, 25), (32, 32)], [[0, 40, 25, 32, 20, 0, 6, 0], [2, 32, 32, 32, 32, 0, 0, 0], [1, 32, 32, 32, 32, 0, 0, 1]]),
}


@pytest.mark.parametrize("canvas", list(IMAGE_CASES))
def test_image_equals_the_reference_arithmetic(canvas):
    H, W = canvas
    sizes, rec = IMAGE_CASES[canvas]
    host = [_src(3 * n + H, h, w) for n, (h, w) in enumerate(sizes)]
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    rec = np.array(rec, np.int32)
    want = LR.canvas(host, rec, H, W)
    src = torch.tensor([t.data_ptr() for t in dev], dtype=torch.int64).to(DEV)
    # the bad record of the 32 x 32 case does not pass the host check: it goes to the kernel directly
    packed = {"imgs": dev, "src": src, "rec": torch.from_numpy(rec).to(DEV), "H": H, "W": W}
    if canvas != (32, 32):
        ok = yolo2d.pack_letterbox(dev, rec, H, W, DEV)
        assert torch.equal(ok["rec"], packed["rec"])
    else:
        with pytest.raises(y3d.Y3DError, match="does not match its image"):
            yolo2d.pack_letterbox(dev, rec, H, W, DEV)
        assert (want[1] == 114).all() and not (want[0] == 114).all()
    u8 = yolo2d.letterbox_images(packed, "uint8")
    fl = yolo2d.letterbox_images(packed, "float")
    assert u8.shape == (3, H, W, 3) and u8.dtype == torch.uint8 and fl.shape == (3, 3, H, W) and fl.dtype == torch.float32
    assert int((u8.cpu().numpy() != want).sum()) == 0
    assert int((fl.cpu().numpy() != LR.to_float(want)).sum()) == 0
    # three different images, so a mixed-up image index would show
    assert len({w.tobytes() for w in want}) == 3


def test_image_entry_refuses_bad_canvases():
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        y3d.lib().letterbox_image(t.data_ptr(), 1, t.data_ptr(), 1, 32, 30, 1, t.data_ptr(), P_ops.stream())
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        yolo2d.letterbox_images({"rec": torch.zeros(1, 8, dtype=torch.int32, device=DEV), "src": t, "H": 32, "W": 30})


# ---------------------------------------------------------------------------------------------------------------- the label kernel
@pytest.mark.parametrize("name", [str(n) for n in Z["rect_sets"]])
@pytest.mark.parametrize("cap", [64, 128])
def test_rect_labels_match_the_reference(img_dir, name, cap):
    sp = _split(img_dir, name)
    max_boxes = None if cap == 64 else cap
    empty = 0
    for k, items in enumerate(sp.batches()):
        random.seed(k)
        st = yolo2d.build_batch(sp, items, yolo2d.data_args(), DEV, mode="val", max_boxes=max_boxes)
        H, W = (int(v) for v in sp.batch_shapes[k])
        B = len(items)
        assert st["img"].shape == (B, H, W, 3) and st["resized_shape"] == [(H, W)] * B
        assert st["cls"].shape == (B * cap, 1) and st["bboxes"].shape == (B * cap, 4) and st["batch_idx"].shape == (B * cap,)
        counts = st["counts"].tolist()
        assert counts == [len(sp.labels[i]) for i in items] and max(counts) <= 64
        for b, c in enumerate(counts):
            blk = slice(b * cap + c, (b + 1) * cap)
            assert (st["batch_idx"][b * cap:b * cap + c] == b).all() and (st["batch_idx"][blk] == -1).all()
            assert not st["cls"][blk].any() and not st["bboxes"][blk].any()
            empty += c == 0
        out = yolo2d.compact_labels(st, counts, max_boxes)
        for key in ("cls", "bboxes", "batch_idx"):
            want = torch.from_numpy(Z[f"{name}/c{k}/{key}"])
            assert out[key].dtype == want.dtype == torch.float32 and out[key].shape == want.shape, key
        assert torch.equal(out["cls"].cpu(), torch.from_numpy(Z[f"{name}/c{k}/cls"]))
        assert torch.equal(out["batch_idx"].cpu(), torch.from_numpy(Z[f"{name}/c{k}/batch_idx"]))
        np.testing.assert_allclose(out["bboxes"].cpu().numpy(), Z[f"{name}/c{k}/bboxes"], rtol=1e-6, atol=1e-6)
        ragged = yolo2d.build_batch(sp, items, yolo2d.data_args(), DEV, mode="val", max_boxes=max_boxes, compact=True)
        assert set(ragged) == set(st) == {"img", "cls", "bboxes", "batch_idx", "counts", "im_file", "ori_shape", "resized_shape", "ratio_pad"}
        assert all(torch.equal(ragged[key], out[key]) for key in ("cls", "bboxes", "batch_idx"))
    assert empty == 1  # the frame without a label file: count 0, all rows -1


# ---------------------------------------------------------------------------------------------------------------- the row kernel
def _rows(preds, meta, conf, classes=None):
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int32).to(DEV)
    out, counts = predict.predict_rows(torch.from_numpy(preds).to(DEV), torch.from_numpy(meta).to(DEV), conf, cl)
    return out.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("name", [str(n) for n in Z["predict_sets"]])
def test_rows_equal_the_references_scale_boxes(name):
    shapes = [tuple(int(v) for v in s) for s in Z[f"{name}/shapes"]]
    canvas = tuple(int(v) for v in Z[f"{name}/canvas"])
    B, n = len(shapes), Z[f"{name}/boxes_in"].shape[1]
    meta = np.zeros((B, 5), np.float32)
    for b, s in enumerate(shapes):
        gain, pad = predict.scale_params(canvas, s)
        meta[b] = (s[0], s[1], gain, pad[0], pad[1])
    conf = np.linspace(0.9, 0.3, n, dtype=np.float32)
    preds = np.concatenate([Z[f"{name}/boxes_in"], np.broadcast_to(conf[None, :, None], (B, n, 1)), np.ones((B, n, 1), np.float32)], 2)
    out, counts = _rows(np.ascontiguousarray(preds, np.float32), meta, 0.25)
    assert counts.tolist() == [n] * B
    want = Z[f"{name}/boxes_out"]
    assert int((out[..., :4] != want).sum()) == 0  # bit equality with the reference's torch arithmetic
    assert np.array_equal(out[..., 4:], preds[..., 4:])
    for b, (h, w) in enumerate(shapes):  # clipped on each of the four sides
        assert (out[b, :, [0, 2]] == 0).any() and (out[b, :, [0, 2]] == w).any() and (out[b, :, [1, 3]] == 0).any() and (out[b, :, [1, 3]] == h).any()


@pytest.mark.parametrize("K", [300, 1])
def test_rows_equal_the_float32_restatement(K):
    rng = np.random.default_rng(K)
    B = 3
    meta = np.array([[60, 100, 0.64, 0, 13], [37, 53, 1.2075471698113207, 0, 10], [480, 640, 0.1, 0, 8]], np.float32)
    preds = np.zeros((B, K, 6), np.float32)
    preds[..., :2] = rng.uniform(-15, 70, (B, K, 2))
    preds[..., 2:4] = preds[..., :2] + rng.uniform(0.5, 40, (B, K, 2))
    preds[..., 4] = -np.sort(-rng.uniform(0.2, 1, (B, K)), axis=1)  # score order; rows past the first 256 still pass 0.25
    preds[..., 5] = rng.integers(0, 6, (B, K))
    thr = 0.25
    preds[:, K // 2, 4] = np.float32(thr)  # equal to the threshold: dropped, the test is a strict >
    preds[:, K // 3, 4] = np.nextafter(np.float32(thr), np.float32(1))  # one ulp above: kept
    for conf, classes in ((thr, None), (thr, [2]), (thr, [1, 3, 5]), (2.0, None), (-1.0, None), (0.3, [0, 4])):
        out, counts = _rows(preds, meta, conf, classes)
        want, wc = LR.predict_rows(preds, meta, conf, classes)
        assert counts.dtype == np.int32 and counts.tolist() == wc.tolist(), (conf, classes)
        assert int((out != want).sum()) == 0, (conf, classes)
        for b in range(B):
            keep = preds[b, :, 4] > np.float32(conf)
            if classes is not None:
                keep &= np.isin(preds[b, :, 5], classes)
            assert counts[b] == keep.sum() and not out[b, counts[b]:].any()  # exact counts, tail rows are zeros
            assert np.array_equal(out[b, :counts[b], 4:], preds[b, keep, 4:])  # order preserved
    assert _rows(preds, meta, 2.0)[1].tolist() == [0] * B and _rows(preds, meta, -1.0)[1].tolist() == [K] * B
    if K > 256:  # more than one 256-row chunk, survivors in both
        out, counts = _rows(preds, meta, thr)
        for b in range(B):
            kept = preds[b, :, 4] > np.float32(thr)
            assert not kept[K // 2] and kept[K // 3] and kept[:256].any() and kept[256:].any()
        assert _rows(preds, meta, -1.0)[0][0, K - 1, 4] == preds[0, K - 1, 4]


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_rect_batches_through_the_model_and_the_metrics(img_dir, model):
    y3d.set_compute_dtype(torch.float32)
    sp = _split(img_dir, "b4")
    pixels = T.images()
    order = [int(i) for i in sp.irect]
    stats = metrics.BoxStats(nc=NC, device=DEV)
    tcls, seen_shapes = [], set()
    for k, items in enumerate(sp.batches()):
        random.seed(11)
        batch = yolo2d.build_batch(sp, items, yolo2d.data_args(), DEV, mode="val")
        H, W = batch["resized_shape"][0]
        seen_shapes.add((H, W))
        # the same canvases from the numpy yardstick
        samples = [yolo2d.rect_sample(sp, i) for i in items]
        rec = np.array([[n, s["h0"], s["w0"], s["h"], s["w"], s["top"], s["left"], 0] for n, s in enumerate(samples)], np.int32)
        want = LR.canvas([pixels[order[i]] for i in items], rec, H, W)
        assert int((batch["img"].cpu().numpy() != want).sum()) == 0
        assert batch["ori_shape"] == [pixels[order[i]].shape[:2] for i in items]
        with torch.no_grad():
            a = predict.raw_rows(model, batch["img"].permute(0, 3, 1, 2), 50)
            b = predict.raw_rows(model, torch.from_numpy(LR.to_float(want)).to(DEV), 50)
        assert a.shape == (len(items), 50, 6) and torch.isfinite(a).all() and torch.equal(a, b)
        # predictions made from the batch's own labels, image by image: a perfect detector in the letter-boxed frame
        counts = batch["counts"].tolist()
        cap = yolo2d.BASE_CAP
        scale = torch.tensor([W, H, W, H], dtype=torch.float32, device=DEV)
        for n, c in enumerate(counts):
            if not c:
                continue
            rows = slice(n * cap, n * cap + c)
            xywh = batch["bboxes"][rows] * scale
            xyxy = torch.cat([xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, :2] + xywh[:, 2:] / 2], 1)
            preds = torch.cat([xyxy, torch.full((c, 1), 0.9, device=DEV), batch["cls"][rows]], 1)[None]
            one = {"cls": batch["cls"][rows], "bboxes": batch["bboxes"][rows], "batch_idx": torch.zeros(c, device=DEV),
                   "ori_shape": batch["ori_shape"][n:n + 1], "ratio_pad": batch["ratio_pad"][n:n + 1], "imgsz": (H, W)}
            stats.update_2d(preds, one)
            tcls.append(batch["cls"][rows].reshape(-1).cpu().numpy())
    assert seen_shapes == {(64, 96), (96, 96), (96, 64)}
    m = metrics.DetMetrics(names={i: str(i) for i in range(NC)})
    stats.get_stats(m)
    tcls = torch.from_numpy(np.concatenate(tcls)).to(DEV)
    n = len(tcls)
    # what a perfect detector gets from the same ap_per_class: (tp, fp, p, r, f1, ap, classes, ...)
    perfect = metrics.ap_per_class(torch.ones(n, 10, dtype=torch.bool, device=DEV), torch.full((n,), 0.9, device=DEV), tcls, tcls)
    assert np.array_equal(m.box.ap_class_index, perfect[6]) and len(perfect[6]) > 5
    np.testing.assert_allclose(m.box.p, 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.box.r, 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(m.box.p, perfect[2]) and np.array_equal(m.box.r, perfect[3])
    np.testing.assert_allclose(m.box.all_ap, perfect[5], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.box.ap, perfect[5].mean(1), rtol=0, atol=1e-12)


def test_predictor_equals_the_hand_chained_calls(model):
    y3d.set_compute_dtype(torch.float32)
    for shapes in ([(60, 100), (100, 60), (32, 48)], [(48, 100), (48, 100)]):
        rgb = [T.frame_pixels(n + 5, w, h) for n, (h, w) in enumerate(shapes)]
        bgr = [np.ascontiguousarray(a[..., ::-1]) for a in rgb]
        # a threshold inside the scores of the random model, so that the filter does something
        probe = predict.Predictor(model, IMGSZ, conf=0.0, max_det=40, stride=STRIDE)
        rows0, counts0 = probe(bgr, static=True)
        assert counts0.tolist() == [40] * len(shapes)
        flat = rows0.reshape(-1, 6)
        flat = flat[flat[:, 4].argsort(descending=True)]
        conf = float(flat[:, 4].median())
        print(f"scores {float(flat[-1, 4]):.6g} .. {float(flat[0, 4]):.6g}, threshold {conf:.6g}, top classes {flat[:2, 5].tolist()}")
        assert flat[0, 4] > conf and len(flat[:, 4].unique()) > len(flat) // 2  # the scores are not tied
        # the class list holds the classes of the two best rows of the batch, which pass the threshold whichever image they are in
        for classes in (None, [int(flat[0, 5]), int(flat[1, 5])]):
            pr = predict.Predictor(model, IMGSZ, conf=conf, classes=classes, max_det=40, stride=STRIDE)
            rec, meta, (H, W) = pr.plan(shapes)
            assert (H, W) == ((64, 64) if len(set(shapes)) > 1 else (32, 64))
            dev = [torch.from_numpy(a).to(DEV) for a in bgr]
            img = yolo2d.letterbox_images(yolo2d.pack_letterbox(dev, rec, H, W, DEV), "uint8")
            assert int((img.cpu().numpy() != LR.canvas(bgr, rec, H, W)).sum()) == 0
            lbs, _ = predict.pre_transform_params(shapes, IMGSZ, STRIDE)
            by_hand = np.stack([LR.letterbox(a, lb["new_unpad"][1], lb["new_unpad"][0], lb["top"], lb["left"], H, W) for a, lb in zip(rgb, lbs)])
            assert np.array_equal(img.cpu().numpy(), by_hand)  # BGR in, RGB out
            with torch.no_grad():
                raw = predict.raw_rows(model, img.permute(0, 3, 1, 2), 40)
            cl = None if classes is None else torch.tensor(classes, dtype=torch.int32).to(DEV)
            want, wc = predict.predict_rows(raw, torch.from_numpy(meta).to(DEV), conf, cl)
            rows, counts = pr(bgr, static=True)
            assert torch.equal(rows, want) and torch.equal(counts, wc)
            ref, rc = LR.predict_rows(raw.cpu().numpy(), meta, conf, classes)
            assert np.array_equal(rows.cpu().numpy(), ref) and counts.tolist() == rc.tolist()
            assert 0 < sum(counts.tolist()) < 40 * len(shapes)
            lst = pr(dev)  # device tensors in, the list form out
            assert [tuple(t.shape) for t in lst] == [(c, 6) for c in counts.tolist()]
            assert all(torch.equal(t, rows[b, :c]) for b, (t, c) in enumerate(zip(lst, counts.tolist())))
            for b, (h, w) in enumerate(shapes):
                t = lst[b]
                assert (t[:, [0, 2]] >= 0).all() and (t[:, [0, 2]] <= w).all() and (t[:, [1, 3]] >= 0).all() and (t[:, [1, 3]] <= h).all()
    with pytest.raises(y3d.Y3DError, match="not on a HIP device"):
        predict.Predictor(model, IMGSZ)([torch.zeros(8, 8, 3, dtype=torch.uint8)])


def test_launches_replay_under_capture(img_dir):
    """recorded once, replayed with new record contents: the replay equals the eager result (default queue settings)"""
    sp = _split(img_dir, "b4")
    packs = []
    for items in sp.batches()[:2]:  # 64 x 96 and 96 x 96 canvases; the capture is recorded at 96 x 96 and both are replayed into it
        random.seed(5)
        samples = [yolo2d.rect_sample(sp, i) for i in items]
        slot = {i: n for n, i in enumerate(items)}
        start = np.concatenate([[0], np.cumsum([len(sp.labels[i]) for i in items])])
        rec, li, lf = yolo2d.rect_records(sp, samples, slot, {i: int(start[n]) for n, i in enumerate(items)})
        imgs = [sp.decode(i, DEV) for i in items]
        table = np.zeros((200, 5), np.float32)  # one table size for both batches
        rows = np.concatenate([sp.labels[i] for i in items])
        table[:len(rows)] = rows
        packs.append((yolo2d.pack_letterbox(imgs, rec, 96, 96, DEV), yolo2d.pack_letterbox_labels(table, li, lf, DEV)))
    rng = np.random.default_rng(0)
    raws = [torch.from_numpy(rng.uniform(0, 90, (4, 70, 6)).astype(np.float32)).to(DEV) for _ in range(2)]
    metas = [torch.tensor([[60, 100, g, 3, 5]] * 4, dtype=torch.float32).to(DEV) for g in (0.64, 1.6)]
    st_i = dict(packs[0][0], rec=packs[0][0]["rec"].clone(), src=packs[0][0]["src"].clone())
    st_l = dict(packs[0][1], **{k: packs[0][1][k].clone() for k in ("rec", "lab_i", "lab_f")})
    st_r, st_m = raws[0].clone(), metas[0].clone()

    def launch():
        return yolo2d.letterbox_images(st_i, "uint8"), yolo2d.letterbox_labels(st_l, 96, 96, 128), predict.predict_rows(st_r, st_m, 45.0)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        launch()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        img, lab, (rows, counts) = launch()
    pi, pl = packs[1]
    st_i["rec"].copy_(pi["rec"])
    st_i["src"].copy_(pi["src"])
    for k in ("rec", "lab_i", "lab_f"):
        st_l[k].copy_(pl[k])
    st_r.copy_(raws[1])
    st_m.copy_(metas[1])
    graph.replay()
    torch.cuda.synchronize()
    want_img, want_lab = yolo2d.letterbox_images(pi, "uint8"), yolo2d.letterbox_labels(pl, 96, 96, 128)
    want_rows, want_counts = predict.predict_rows(raws[1], metas[1], 45.0)
    first_img = yolo2d.letterbox_images(packs[0][0], "uint8")
    assert torch.equal(img, want_img) and not torch.equal(img, first_img)
    for k in want_lab:
        assert torch.equal(lab[k], want_lab[k]), k
    assert lab["counts"].tolist() == [len(sp.labels[i]) for i in sp.batches()[1]]
    assert torch.equal(rows, want_rows) and torch.equal(counts, want_counts) and 0 < int(counts.sum()) < 4 * 70
    graph.reset()
