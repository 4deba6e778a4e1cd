"""GPU: the KITTI label encoder (csrc/kitti_labels.hip, kitti.encode_labels / build_batch) against the reference's own
`KITTIDataset.__getitem__` + `collate_fn` (tests/golden/kitti_labels.npz, minted by tools/make_golden_kitti_labels.py): survivors, order,
counts, classes and heading bins exactly, every float within 1e-6, calib / ratio_pad within 1e-9; the compact form in collate_fn's
shapes and dtypes; the 3D loss's padded targets; build_batch end to end; a captured-and-replayed launch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from kitti_labels_tree import argset, fixture, per_image, write_tree

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import kitti  # noqa: E402
from yolov10_3d_amd import loss as PL  # noqa: E402

DEV = "cuda"
M = kitti.MAX_OBJS
KEYS = ("cls", "bboxes", "center_2d", "size_2d", "center_3d", "size_3d", "depth", "heading_bin", "heading_res")


def packed_run(z, root, name, device=DEV):
    """the run's batch packed from the rebuilt tree and the recorded draws"""
    mode, args, seed, items = argset(z, name)
    lab = lambda i: kitti.read_label(os.path.join(root, "training/label_2", f"{i:06d}.txt"))
    partners = [lab(int(p)) if p >= 0 else None for p in z[f"{name}/partner"]]
    return kitti.pack_labels([lab(i) for i in items], partners, list(z[f"{name}/P2"]), list(z[f"{name}/trans"]),
                             list(z[f"{name}/flip"]), list(z[f"{name}/scale"]), [z["frame_wh"][i] for i in items], device), args


def check_static(out, z, name):
    items = argset(z, name)[3]
    B = len(items)
    counts = out["counts"].cpu().numpy()
    want_n = np.bincount(z[f"{name}/c/batch_idx"].astype(np.int64), minlength=B)
    assert np.array_equal(counts, want_n), (name, counts, want_n)
    got = {k: out[k].cpu().numpy() for k in KEYS + ("batch_idx",)}
    for k in KEYS:
        want = per_image(z, name, k)
        for b in range(B):
            g = got[k][b * M:b * M + counts[b]]
            w = want[b].astype(np.float64).reshape(g.shape)
            if k in ("cls", "heading_bin"):
                assert np.array_equal(g, w), (name, b, k, g, w)
            else:
                np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6, err_msg=f"{name} image {b} {k}")
    for b in range(B):
        assert (got["batch_idx"][b * M:b * M + counts[b]] == b).all()
        pad = slice(b * M + counts[b], (b + 1) * M)
        assert (got["batch_idx"][pad] == -1).all()
        for k in KEYS:
            assert not got[k][pad].any(), (name, b, k)
    np.testing.assert_allclose(out["calib"].cpu().numpy(), z[f"{name}/c/calib"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(out["ratio_pad"].cpu().numpy(), z[f"{name}/c/ratio_pad"], rtol=1e-9, atol=0)


def encode_run(z, root, name):
    packed, args = packed_run(z, root, name)
    return kitti.encode_labels(packed, kitti.RESOLUTION, args.min_depth_threshold, args.max_depth_threshold, args.cam_dis)


@pytest.mark.parametrize("name", ["default", "camdis", "val", "nomix"])
def test_encode_labels_matches_the_reference(tmp_path, name):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    assert len(argset(z, name)[3]) >= 8
    check_static(encode_run(z, root, name), z, name)


def check_compact(c, z, name):
    for k in KEYS + ("batch_idx",):
        want = z[f"{name}/c/{k}"]
        g = c[k]
        assert tuple(g.shape) == want.shape, (name, k, tuple(g.shape), want.shape)
        assert str(g.dtype).replace("torch.", "") == str(want.dtype), (name, k, g.dtype, want.dtype)
        g = g.cpu().numpy()
        if k in ("cls", "heading_bin", "batch_idx"):
            assert np.array_equal(g, want), (name, k)
        else:
            np.testing.assert_allclose(g, want, rtol=1e-6, atol=1e-6, err_msg=f"{name} {k}")


@pytest.mark.parametrize("name", ["default", "camdis", "val", "nomix"])
def test_compact_has_the_collated_shapes_and_dtypes(tmp_path, name):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    out = encode_run(z, root, name)
    counts = out["counts"].tolist()
    c = kitti.compact_labels(out, counts, [bool(v) for v in z[f"{name}/crop"]], bool(int(z[f"{name}/cam_dis"])))
    check_compact(c, z, name)
    rows = torch.cat([torch.arange(b * M, b * M + n) for b, n in enumerate(counts)]).to(DEV)
    for k in KEYS:  # the same values as the static form
        assert torch.equal(c[k], out[k].index_select(0, rows).to(c[k].dtype).reshape(c[k].shape)), k


def loss_model():
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=3, no=38)
    return SimpleNamespace(model=[head], args=SimpleNamespace(**y3d.tasks.DEFAULT_HYP))


@pytest.mark.parametrize("name", ["default", "camdis"])
def test_loss_targets_from_the_static_layout(tmp_path, name):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    out = encode_run(z, root, name)
    B = len(argset(z, name)[3])
    ref = {k: torch.from_numpy(z[f"{name}/c/{k}"]) for k in KEYS + ("batch_idx",)}
    crit = PL.DDDetectionLoss(loss_model(), tal_topk=10)
    H, W = kitti.RESOLUTION[1] // 8, kitti.RESOLUTION[0] // 8
    g_s, n_s = crit.targets(out, B, H, W, DEV)
    g_r, n_r = crit.targets(ref, B, H, W, DEV)
    assert int(n_s) == int(n_r) > 0
    torch.testing.assert_close(g_s, g_r, rtol=1e-6, atol=1e-6)


def loss_items(batch, B, seed=0):
    """one eager DetectLoss3d step on fixed random head maps"""
    y3d.set_compute_dtype(torch.float32)
    g = torch.Generator(device=DEV).manual_seed(seed)
    o2m, o2o = [], []
    for s in (8, 16, 32):
        for dst in (o2m, o2o):
            t = torch.randn(B, 38, kitti.RESOLUTION[1] // s, kitti.RESOLUTION[0] // s, device=DEV, generator=g)
            t[:, 36] = 10 + 30 * torch.rand(t[:, 36].shape, device=DEV, generator=g)
            dst.append(y3d.ops._dense_any(t, torch.float32))
    crit = PL.DetectLoss3d(loss_model())
    loss, items = crit({"one2many": o2m, "one2one": o2o}, batch)
    return loss.detach(), items.detach()


def test_build_batch_end_to_end(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z, images=True)
    name = "default"
    mode, args, seed, items = argset(z, name)
    np.random.seed(seed)
    bs = kitti.build_batch(root, items, args, DEV, mode=mode, img_mode="float")
    check_static(bs, z, name)
    assert torch.equal(bs["mixed"].cpu(), torch.from_numpy(z[f"{name}/c/mixed"]))
    assert bs["mean_sizes"].shape == (3, 3) and bs["mean_sizes"].dtype == torch.float64
    assert bs["im_file"] == [f"{i:06d}.txt" for i in items]
    for b, i in enumerate(items):
        np.testing.assert_allclose(bs["info"][b]["trans_inv"], z[f"{name}/trans_inv"][b], rtol=1e-12, atol=1e-12)
        assert tuple(bs["ori_shape"][b]) == tuple(z["frame_wh"][i][::-1])
    # the image half: augment_images with the recorded draws
    from kitti_labels_tree import frame_pixels
    px = lambda i: torch.from_numpy(frame_pixels(i, *(int(v) for v in z["frame_wh"][i]))).to(DEV)
    img = kitti.augment_images([px(i) for i in items], [px(int(p)) if p >= 0 else None for p in z[f"{name}/partner"]],
                               [bool(f) for f in z[f"{name}/flip"]], list(z[f"{name}/trans_inv"]), kitti.RESOLUTION, mode="float")
    assert torch.equal(bs["img"], img)
    # the same draws again, compact: collate_fn's ragged batch
    np.random.seed(seed)
    bc = kitti.build_batch(os.path.join(root, "ImageSets", "train.txt"), items, args, DEV, mode=mode, compact=True)
    check_compact(bc, z, name)
    assert bc["img"].dtype == torch.uint8 and tuple(bc["img"].shape) == (len(items), kitti.RESOLUTION[1], kitti.RESOLUTION[0], 3)
    ls, is_ = loss_items(bs, len(items))
    lc, ic = loss_items(bc, len(items))
    torch.testing.assert_close(is_, ic, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(ls, lc, rtol=1e-6, atol=1e-6)
    assert float(is_.abs().sum()) > 0


def test_val_mode_draws_nothing(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z, images=True)
    mode, args, seed, items = argset(z, "val")
    np.random.seed(seed)
    state = np.random.get_state()[1].copy()
    b = kitti.build_batch(root, items, args, DEV, mode=mode)
    assert np.array_equal(np.random.get_state()[1], state)
    check_static(b, z, "val")


def test_captured_encode_replays_new_inputs(tmp_path):
    z = fixture()
    root = write_tree(str(tmp_path), z)
    pa, args = packed_run(z, root, "camdis")
    pb, _ = packed_run(z, root, "nomix")
    assert pa["img_i"].shape == pb["img_i"].shape
    cap = max(pa["rec"].shape[0], pb["rec"].shape[0])
    static = {k: v.clone() for k, v in pa.items()}
    static["rec"] = torch.zeros(cap, 16, dtype=torch.float64, device=DEV)
    static["rec"][:pa["rec"].shape[0]] = pa["rec"]
    kw = dict(out_wh=kitti.RESOLUTION, min_depth=1.0, max_depth=120.0, use_camera_dis=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kitti.encode_labels(static, **kw)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = kitti.encode_labels(static, **kw)
    for src in (pb, pa):
        static["rec"].zero_()
        static["rec"][:src["rec"].shape[0]] = src["rec"]
        for k in ("img_i", "img_f", "mean_size"):
            static[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        want = kitti.encode_labels(src, **kw)
        for k in want:
            assert torch.equal(out[k], want[k]), k
    graph.reset()
