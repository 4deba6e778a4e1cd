"""GPU: the Waymo / Omni3D label encoder (csrc/json3d_labels.hip, json3d.encode_labels / build_batch) against the reference's own
`WaymoDataset` / `Omni3Dataset` `__getitem__` + `collate_fn` (tests/golden/waymo_labels.npz, omni3d_labels.npz, minted by
tools/make_golden_json3d_labels.py): survivors, order, counts, classes and heading bins exactly, every float within 1e-6, calib /
ratio_pad within 1e-9; build_batch end to end; compact against static loss targets; val mode; a captured-and-replayed launch.

Waymo's recomputed box passes through the float32 sin / cos of torch's CPU kernels.  The kernel takes them in float64 and rounds,
so no column needs a wider bound: everything is held to 1e-6, the recomputed box included."""
import numpy as np
import pytest
import torch

from json3d_tree import DATASETS, KEYS, RUNS, argset, fixture, frame_pixels, per_image, write_tree

pytestmark = pytest.mark.gpu

import yolov10_3d_amd as y3d  # noqa: E402
from yolov10_3d_amd import json3d, kitti  # noqa: E402
from yolov10_3d_amd import loss as PL  # noqa: E402

DEV = "cuda"
M = json3d.MAX_OBJS
# tx, ty of a mirrored calibration whose fourth column is zero (Omni3D's K, two of the fixture's three Waymo cameras) are zero in
# exact arithmetic; what either side holds is the float64 rounding of its fit over values up to fu * z = 515 * 78 = 4e4 (2^-52 * 4e4 =
# 1e-11 in P2[:, 3]), divided by fu and scaled by the resolution ratio: 4e-14.  A relative bound cannot compare two such residues
# (the reference's are 3e-15 here), so these two columns also get an absolute 1e-12, a thousandth of 1e-9 of any real tx (>= 1e-3 m).
TXY_ATOL = 1e-12


def split_of(z, dataset, tmp):
    return json3d.Split(write_tree(str(tmp), z, dataset), dataset)


def pack(z, sp, dataset, name):
    mode, args, seed, items = argset(z, name)
    rec = lambda pos: sp.records(sp.ids[pos])
    partners = [rec(int(p)) if p >= 0 else None for p in z[f"{name}/partner"]]
    return json3d.pack_labels([rec(i) for i in items], partners, list(z[f"{name}/P2"]), list(z[f"{name}/trans"]), list(z[f"{name}/flip"]),
                              list(z[f"{name}/scale"]), [z["frame_wh"][i] for i in items], DEV, dataset), args


def check_static(out, z, dataset, name):
    items = argset(z, name)[3]
    B = len(items)
    assert B <= 8
    counts = out["counts"].cpu().numpy()
    want_n = np.bincount(z[f"{name}/c/batch_idx"].astype(np.int64), minlength=B)
    assert np.array_equal(counts, want_n), (name, counts, want_n)
    got = {k: out[k].cpu().numpy() for k in KEYS + ("batch_idx",)}
    worst = {}
    for k in KEYS:
        want = per_image(z, name, k)
        for b in range(B):
            g = got[k][b * M:b * M + counts[b]]
            w = want[b].astype(np.float64).reshape(g.shape)
            if k in ("cls", "heading_bin"):
                assert np.array_equal(g, w), (name, b, k, g, w)
            elif g.size:
                worst[k] = max(worst.get(k, 0.0), float(np.abs(g - w).max()))
    print(f"{dataset} {name}: largest deviations {worst}")
    for k in KEYS:
        want = per_image(z, name, k)
        for b in range(B):
            g = got[k][b * M:b * M + counts[b]]
            w = want[b].astype(np.float64).reshape(g.shape)
            if k not in ("cls", "heading_bin"):
                np.testing.assert_allclose(g, w, rtol=1e-6, atol=1e-6, err_msg=f"{dataset} {name} image {b} {k}")
    for b in range(B):
        assert (got["batch_idx"][b * M:b * M + counts[b]] == b).all()
        pad = slice(b * M + counts[b], (b + 1) * M)
        assert (got["batch_idx"][pad] == -1).all()
        for k in KEYS:
            assert not got[k][pad].any(), (name, b, k)
    calib = out["calib"].cpu().numpy()
    np.testing.assert_allclose(calib[:, :4], z[f"{name}/c/calib"][:, :4], rtol=1e-9, atol=0)
    np.testing.assert_allclose(calib[:, 4:], z[f"{name}/c/calib"][:, 4:], rtol=1e-9, atol=TXY_ATOL)
    np.testing.assert_allclose(out["ratio_pad"].cpu().numpy(), z[f"{name}/c/ratio_pad"], rtol=1e-9, atol=0)


def encode_run(z, sp, dataset, name):
    packed, args = pack(z, sp, dataset, name)
    return json3d.encode_labels(packed, json3d.RESOLUTION, args.min_depth_threshold, args.max_depth_threshold, args.cam_dis)


@pytest.mark.parametrize("name", RUNS)
@pytest.mark.parametrize("dataset", DATASETS)
def test_encode_labels_matches_the_reference(tmp_path, dataset, name):
    z = fixture(dataset)
    sp = split_of(z, dataset, tmp_path)
    check_static(encode_run(z, sp, dataset, name), z, dataset, name)


def check_compact(c, z, name):
    """collate_fn's ragged shapes and dtypes"""
    for k in KEYS + ("batch_idx",):
        want = z[f"{name}/c/{k}"]
        assert tuple(c[k].shape) == want.shape, (name, k, tuple(c[k].shape), want.shape)
        assert str(c[k].dtype).replace("torch.", "") == str(want.dtype), (name, k, c[k].dtype, want.dtype)


def loss_model():
    from types import SimpleNamespace
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=3, no=38)
    return SimpleNamespace(model=[head], args=SimpleNamespace(**y3d.tasks.DEFAULT_HYP))


@pytest.mark.parametrize("dataset", DATASETS)
def test_compact_and_static_give_the_same_loss_targets(tmp_path, dataset):
    z = fixture(dataset)
    sp = split_of(z, dataset, tmp_path)
    name = "default"
    out = encode_run(z, sp, dataset, name)
    B = len(argset(z, name)[3])
    counts = out["counts"].tolist()
    c = json3d.compact_labels(out, counts, dataset=dataset)
    assert c["cls"].shape[0] == sum(counts) == z[f"{name}/c/batch_idx"].shape[0] > 0
    check_compact(c, z, name)
    # a run without an empty image: no promotion to float64 by torch.cat
    o2 = encode_run(z, sp, dataset, "more")
    check_compact(json3d.compact_labels(o2, o2["counts"].tolist(), dataset=dataset), z, "more")
    assert str(z["more/c/center_2d"].dtype) == "float32" and str(z[f"{name}/c/center_2d"].dtype) == "float64"
    crit = PL.DDDetectionLoss(loss_model(), tal_topk=10)
    H, W = json3d.RESOLUTION[1] // 8, json3d.RESOLUTION[0] // 8
    g_s, n_s = crit.targets(out, B, H, W, DEV)
    g_c, n_c = crit.targets(c, B, H, W, DEV)
    assert int(n_s) == int(n_c) > 0
    assert torch.equal(g_s, g_c)


@pytest.mark.parametrize("dataset", DATASETS)
def test_build_batch_end_to_end(tmp_path, dataset):
    z = fixture(dataset)
    path = write_tree(str(tmp_path), z, dataset, images=True)
    name = "default"
    mode, args, seed, items = argset(z, name)
    np.random.seed(seed)
    bs = json3d.build_batch(path, items, args, DEV, dataset=dataset, mode=mode, img_mode="float")
    check_static(bs, z, dataset, name)
    assert torch.equal(bs["mixed"].cpu(), torch.from_numpy(z[f"{name}/c/mixed"])) and int(bs["mixed"].sum()) > 0
    assert bs["mean_sizes"].dtype == torch.float64 and np.array_equal(bs["mean_sizes"].cpu().numpy(), z[f"{name}/c/mean_sizes"])
    assert bs["im_file"] == ["%06d.txt" % int(z["img_id"][i]) for i in items]
    for b, i in enumerate(items):
        np.testing.assert_allclose(bs["info"][b]["trans_inv"], z[f"{name}/trans_inv"][b], rtol=1e-12, atol=1e-12)
        assert bs["info"][b]["img_id"] == int(z["img_id"][i])
        assert tuple(bs["ori_shape"][b]) == tuple(z["frame_wh"][i][::-1])
    # the image half: augment_images with the recorded draws
    px = lambda i: torch.from_numpy(frame_pixels(i, *(int(v) for v in z["frame_wh"][i]))).to(DEV)
    img = kitti.augment_images([px(i) for i in items], [px(int(p)) if p >= 0 else None for p in z[f"{name}/partner"]],
                               [bool(f) for f in z[f"{name}/flip"]], list(z[f"{name}/trans_inv"]), json3d.RESOLUTION, mode="float")
    assert torch.equal(bs["img"], img)
    # the same draws again, compact and uint8
    np.random.seed(seed)
    bc = json3d.build_batch(path, items, args, DEV, dataset=dataset, mode=mode, compact=True)
    assert bc["img"].dtype == torch.uint8 and tuple(bc["img"].shape) == (len(items), json3d.RESOLUTION[1], json3d.RESOLUTION[0], 3)
    assert "counts" not in bc
    check_compact(bc, z, name)
    assert np.array_equal(bc["batch_idx"].cpu().numpy(), z[f"{name}/c/batch_idx"])


@pytest.mark.parametrize("dataset", DATASETS)
def test_val_mode_draws_nothing(tmp_path, dataset):
    z = fixture(dataset)
    path = write_tree(str(tmp_path), z, dataset, images=True)
    mode, args, seed, items = argset(z, "val")
    np.random.seed(seed)
    state = np.random.get_state()[1].copy()
    b = json3d.build_batch(path, items, args, DEV, dataset=dataset, mode=mode)
    assert np.array_equal(np.random.get_state()[1], state)
    check_static(b, z, dataset, "val")


@pytest.mark.parametrize("dataset", DATASETS)
def test_captured_encode_replays_new_inputs(tmp_path, dataset):
    z = fixture(dataset)
    sp = split_of(z, dataset, tmp_path)
    pa, args = pack(z, sp, dataset, "more")
    pb, _ = pack(z, sp, dataset, "nomix")
    assert pa["img_i"].shape == pb["img_i"].shape
    cap = max(pa["rec"].shape[0], pb["rec"].shape[0])
    static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in pa.items()}
    static["rec"] = torch.zeros(cap, json3d.REC_W, dtype=torch.float64, device=DEV)
    static["rec"][:pa["rec"].shape[0]] = pa["rec"]
    kw = dict(out_wh=json3d.RESOLUTION, min_depth=1.0, max_depth=120.0, use_camera_dis=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        json3d.encode_labels(static, **kw)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = json3d.encode_labels(static, **kw)
    for src in (pb, pa):
        static["rec"].zero_()
        static["rec"][:src["rec"].shape[0]] = src["rec"]
        for k in ("img_i", "img_f", "mean_size"):
            static[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        want = json3d.encode_labels(src, **kw)
        for k in want:
            assert torch.equal(out[k], want[k]), k
    graph.reset()
