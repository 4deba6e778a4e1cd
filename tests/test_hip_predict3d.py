"""GPU: the 3D predictor's row pass (csrc/predict3d.hip, predict.predict3d_rows) — rows and counts bit for bit against the decode kernel
compacted on the host, corners against the float64 restatement of tests/predict3d_ref.py and against the reference's own
(tests/golden/predict3d.npz), a captured-and-replayed launch, and end to end: `Predictor3d` on a tiny 3D model, `build_test_batch`
against `build_batch(mode="val")`, `predict_split` through `save_results` and back.

Measured maxima of the comparison with the reference (test_rows_and_corners_match_the_reference prints them): see DESIGN §3.18."""
import functools
import os

import numpy as np
import pytest
import torch

import predict3d_ref as PR
from kitti_labels_tree import fixture as tree_fixture, frame_pixels, write_tree

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, kitti_eval, predict
from yolov10_3d_amd import loss as PL
from yolov10_3d_amd import ops as P_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
Z = PR.fixture()
G = PR.decode_fixture()
CLASS_LISTS = {"none": None, "c0": [0], "c12": [1, 2], "c2": [2]}
RES = (320, 256)  # (W, H) of the end-to-end model: 80 cells on the coarsest level for max_det = 50


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    before = P_ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


# ---------------------------------------------------------------------------------------------------------------- inputs, shared
@functools.lru_cache(maxsize=None)
def _inputs(source):
    """source -> (preds (B, K, 37) float32 numpy, calib6, P2 float32, ratio, inv_trans)"""
    if source == "fixture":
        return G["preds"], G["calib"], Z["P2"], G["ratio"], G["inv_trans"]
    B, K = source
    preds = PR.synth(torch.Generator().manual_seed(100 * B + K), B, K).numpy()
    return (preds,) + PR.synth_camera(B)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _run(source, conf, cls_tag, inv, cam):
    """one launch of the new kernel and the two-step path it replaces -> numpy (rows, corners3d, corners_img, counts, want_rows list)"""
    preds, calib6, P2, ratio, inv_trans = _inputs(source)
    classes = CLASS_LISTS[cls_tag]
    cl = None if classes is None else torch.tensor(classes, dtype=torch.int32).to(DEV)
    p = _dev(preds)
    rows, c3, ci, counts = predict.predict3d_rows(p, _dev(calib6), _dev(P2), _dev(ratio), _dev(inv_trans) if inv else None, conf, cl,
                                                  use_camera_dis=cam)
    old, keep = kitti.decode_preds_device(p, _dev(calib6), _dev(ratio), list(inv_trans), undo_augment=inv, threshold=conf, use_camera_dis=cam)
    old, keep = old.cpu().numpy(), keep.cpu().numpy()
    if classes is not None:
        keep = keep & np.isin(preds[..., 36].astype(np.int32), classes)
    return rows.cpu().numpy(), c3.cpu().numpy(), ci.cpu().numpy(), counts.cpu().numpy(), [old[b][keep[b]] for b in range(len(old))]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _scores(source):
    preds, calib6, _, ratio, inv_trans = _inputs(source)
    return kitti.decode_preds_device(_dev(preds), _dev(calib6), _dev(ratio), list(inv_trans), threshold=0.0)[0][..., 13].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _cases(source):
    """(conf, class tag, inv_trans given, use_camera_dis) of a source"""
    if source == "fixture":
        return [(conf, tag, inv, cam) for conf in (0.001, 0.25) for tag in CLASS_LISTS for inv in (True, False) for cam in (False, True)]
    sc = _scores(source)
    b, k = sc.shape[0] - 1, sc.shape[1] // 2
    equal = float(sc[b, k])  # a threshold equal to one row's score: that row is kept
    return [(0.25, "none", True, False), (0.25, "c12", False, False), (0.25, "c2", True, True), (equal, "none", True, False),
            (float(np.nextafter(equal, np.inf)), "none", True, False), (1e30, "none", True, False), (-1.0, "none", True, False)]


SOURCES = ["fixture", (1, 1), (2, 257), (3, 300)]


# ---------------------------------------------------------------------------------------------------------------- 1. the decode kernel
@pytest.mark.parametrize("source", SOURCES, ids=str)
def test_rows_and_counts_equal_the_decode_kernel(source):
    preds = _inputs(source)[0]
    B, K = preds.shape[:2]
    kept_total = 0
    for case in _cases(source):
        rows, c3, ci, counts, want = _run(source, *case)
        assert counts.dtype == np.int32 and rows.shape == (B, K, 14) and c3.shape == (B, K, 8, 3) and ci.shape == (B, K, 8, 2)
        assert counts.tolist() == [len(w) for w in want], case
        for b in range(B):
            n = counts[b]
            assert np.array_equal(_bits(rows[b, :n]), _bits(want[b])), (case, b)  # bit equality, NaN (camera distance) included
            assert not _bits(rows[b, n:]).any() and not _bits(c3[b, n:]).any() and not _bits(ci[b, n:]).any(), (case, b)
        kept_total += int(counts.sum())
    assert kept_total > 0
    if source == "fixture":
        for tag in CLASS_LISTS:  # the counts the reference's filter leaves
            assert _run(source, 0.25, tag, True, False)[3].tolist() == Z[f"class_counts_t25/{tag}"].tolist()
        assert _run(source, 0.25, "c0", True, False)[3][0] == 0
        return
    sc = _scores(source)
    b, k = B - 1, K // 2
    eq, above, nothing, everything = (_run(source, *c) for c in _cases(source)[3:])
    assert eq[3][b] == (sc[b] >= sc[b, k]).sum() and above[3][b] == eq[3][b] - 1  # the row at the threshold is kept, one ulp above it is not
    assert nothing[3].tolist() == [0] * B and everything[3].tolist() == [K] * B
    assert np.array_equal(_bits(everything[0][B - 1, K - 1]), _bits(everything[4][B - 1][K - 1]))
    if K > 256:  # survivors in both chunks, so the running base is used, and rows dropped in the first
        keep = ~(sc < 0.25)
        assert keep[:, :256].any(1).all() and keep[:, 256:].any(1).all() and (~keep[:, :256]).any(1).all()


# ---------------------------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("source", SOURCES, ids=str)
def test_corners_equal_the_float64_restatement(source):
    P2 = _inputs(source)[2]
    total = 0
    for case in _cases(source):
        rows, c3, ci, counts, _ = _run(source, *case)
        checked = 0
        for b, n in enumerate(counts):
            front = c3[b, :n, :, 2].min(1) >= 0.5 if n else np.zeros(0, bool)  # NaN rows (camera distance) compare False
            if not front.any():
                continue
            w3, wi = PR.corners(rows[b, :n][front], P2[b])
            np.testing.assert_allclose(c3[b, :n][front], w3, rtol=0, atol=1e-9, err_msg=str((case, b)))
            np.testing.assert_allclose(ci[b, :n][front], wi, rtol=1e-9, atol=1e-9, err_msg=str((case, b)))
            checked += int(front.sum())
        if not case[3]:  # pinhole depth: a row whose centre lies half a box diagonal + 0.5 m in front is certainly compared
            sure = sum(int((rows[b, :n, 11] - np.hypot(rows[b, :n, 8] / 2, rows[b, :n, 7] / 2) >= 0.5).sum()) for b, n in enumerate(counts))
            assert checked >= sure and sure >= 0.9 * counts.sum(), (case, checked, sure, counts)
            if source == "fixture":  # its nearest corner lies 7.8 m in front: every kept row
                assert checked == counts.sum(), (case, checked, counts)
        total += checked
    assert total > 0


# ---------------------------------------------------------------------------------------------------------------- 3. the reference
@pytest.mark.parametrize("tag,conf", [("t001", 0.001), ("t25", 0.25)])
def test_rows_and_corners_match_the_reference(tag, conf):
    rows, c3, ci, counts, _ = _run("fixture", conf, "none", True, False)
    assert counts.tolist() == Z[f"{tag}/counts"].tolist()
    err = np.zeros(3)
    for b, n in enumerate(counts):
        err = np.maximum(err, [np.abs(rows[b, :n] - Z[f"{tag}/rows"][b, :n]).max(), np.abs(c3[b, :n] - Z[f"{tag}/corners3d"][b, :n]).max(),
                               np.abs(ci[b, :n] - Z[f"{tag}/corners_img"][b, :n]).max()])
    print(f"{tag}: max |rows - ref| {err[0]:.3g}, corners3d {err[1]:.3g} m, corners_img {err[2]:.3g} px")
    for b, n in enumerate(counts):
        np.testing.assert_allclose(rows[b, :n], Z[f"{tag}/rows"][b, :n], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(c3[b, :n], Z[f"{tag}/corners3d"][b, :n], rtol=0, atol=1e-4)
        np.testing.assert_allclose(ci[b, :n], Z[f"{tag}/corners_img"][b, :n], rtol=0, atol=2e-2)
    if tag == "t25":  # the class lists drop what the reference's mask drops
        for ctag, classes in CLASS_LISTS.items():
            got = _run("fixture", conf, ctag, True, False)
            for b in range(3):
                ref = Z[f"{tag}/rows"][b, :Z[f"{tag}/counts"][b]]
                ref = ref[Z[f"class_keep_t25/{ctag}"][b, :len(ref)]]  # what the reference's predictor keeps of the 0.25 set
                assert got[3][b] == len(ref)
                np.testing.assert_allclose(got[0][b, :len(ref)], ref, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- 4. graph replay
def test_row_pass_replays_under_capture():
    """recorded once, replayed with new predictions: the replay equals the eager result (a single-branch graph, default queue settings)"""
    B, K = 3, 300
    first, calib6, P2, ratio, inv = _inputs((B, K))
    second = PR.synth(torch.Generator().manual_seed(7), B, K)
    st = _dev(first).clone()
    args = (_dev(calib6), _dev(P2).double(), _dev(ratio), _dev(inv))
    cl = torch.tensor([0, 2], dtype=torch.int32).to(DEV)
    launch = lambda x: predict.predict3d_rows(x, *args, 0.25, cl)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture (uploads the mean-size table)
        launch(st)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = launch(st)
    st.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    want = launch(second.to(DEV))
    before = launch(_dev(first))
    for got, w in zip(out, want):
        assert torch.equal(got.view(torch.int64) if got.dtype == torch.float64 else got, w.view(torch.int64) if w.dtype == torch.float64 else w)
    assert not torch.equal(out[3], before[3]) or not torch.equal(out[0], before[0])
    assert 0 < int(out[3].sum()) < B * K
    graph.reset()


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
FRAMES = [2, 7]  # 1242 x 375 and 1224 x 370


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    z = tree_fixture()
    root = write_tree(str(tmp_path_factory.mktemp("kitti3d")), z, images=True)
    return PR.add_testing_split(root, FRAMES), z


@pytest.fixture(scope="module")
def model():
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(cfg).to(DEV)
    # As in tests/test_hip_letterbox.py: at the default initialisation the features of a random model die out with depth and every
    # score of a level is the same number.  One training-mode forward with momentum 1 gives every BatchNorm the statistics of a random
    # batch; wider random projections of the two branches the score is made of (class, depth uncertainty) spread the scores.
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    keep = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 1.0
    with torch.no_grad():
        m.train()(torch.rand(2, 3, RES[1], RES[0], device=DEV))
        head = m.model[-1]
        for branch in (head.cls, head.dep_un):
            for level in branch:
                level[-1].weight.normal_(0.0, 0.05)
                level[-1].bias.add_(torch.randn_like(level[-1].bias))
    for b, mom in zip(bns, keep):
        b.momentum = mom
    P_ops.bump_param_epoch()
    y3d.set_compute_dtype(before)
    return m.eval()


def _frames(tree):
    root, z = tree
    rgb = [frame_pixels(i, *(int(v) for v in z["frame_wh"][i])) for i in FRAMES]
    P2s = [kitti.read_calib(os.path.join(root, "testing/calib", f"{i:06d}.txt")) for i in FRAMES]
    return rgb, P2s


def _threshold(model, rgb, P2s):
    """a threshold inside the scores of the random model, so that the filter does something"""
    rows, _, _, counts = predict.Predictor3d(model, conf=-1.0, resolution=RES)(rgb, P2s, static=True)
    assert counts.tolist() == [50] * len(rgb)
    sc = rows[..., 13].reshape(-1)
    conf = float(sc.median())
    print(f"scores {float(sc.min()):.6g} .. {float(sc.max()):.6g}, threshold {conf:.6g}, {len(sc.unique())} distinct")
    return conf


def test_predictor_equals_the_hand_chained_calls(tree, model):
    y3d.set_compute_dtype(torch.float32)
    rgb, P2s = _frames(tree)
    conf = _threshold(model, rgb, P2s)
    for classes in (None, [0, 2]):
        pr = predict.Predictor3d(model, conf=conf, classes=classes, resolution=RES)
        p = pr.plan([a.shape[:2] for a in rgb], P2s)
        dev = [torch.from_numpy(a).to(DEV) for a in rgb]
        img = kitti.augment_images(dev, [None, None], [False, False], list(p["trans_inv"]), RES, "uint8")
        assert tuple(img.shape) == (2, RES[1], RES[0], 3)
        with torch.no_grad():
            y = model(img.permute(0, 3, 1, 2))["one2one"][0]
            reg, sc, lab = PL.v10_3Dpostprocess(y.permute(0, 2, 1), 50, 3)
        raw = torch.cat((reg, sc.unsqueeze(-1), lab.unsqueeze(-1)), -1)
        assert tuple(raw.shape) == (2, 50, 37) and torch.isfinite(raw).all()
        cl = None if classes is None else torch.tensor(classes, dtype=torch.int32).to(DEV)
        want = predict.predict3d_rows(raw, _dev(p["calib6"]), _dev(p["P2"]), _dev(p["ratio"]), _dev(p["trans_inv"]), conf, cl)
        got = pr(rgb, P2s, static=True)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        counts = got[3].tolist()
        if classes is None:
            assert 0 < sum(counts) < 100
        lst = pr(dev, P2s)  # device tensors in, the list form out
        assert [set(d) for d in lst] == [{"rows", "corners3d", "corners_img"}] * 2
        for b, (d, n) in enumerate(zip(lst, counts)):
            assert tuple(d["rows"].shape) == (n, 14) and tuple(d["corners3d"].shape) == (n, 8, 3) and tuple(d["corners_img"].shape) == (n, 8, 2)
            assert torch.equal(d["rows"], got[0][b, :n]) and torch.equal(d["corners3d"], got[1][b, :n]) and torch.equal(d["corners_img"], got[2][b, :n])
            if classes is not None:
                assert np.isin(d["rows"][:, 0].cpu().numpy(), classes).all()
    with pytest.raises(y3d.Y3DError, match="not on a HIP device"):
        predict.Predictor3d(model, resolution=RES)([torch.zeros(8, 8, 3, dtype=torch.uint8)], P2s[:1])


def test_test_batch_equals_the_val_batch(tree):
    root, z = tree
    test = kitti.build_test_batch(root, [0, 1], DEV, resolution=RES)
    val = kitti.build_batch(root, FRAMES, kitti.data_args(), DEV, mode="val", resolution=RES)
    assert set(test) == {"img", "calib", "info", "im_file", "ori_shape", "ratio_pad", "P2"}
    assert test["img"].dtype == torch.uint8 and torch.equal(test["img"], val["img"])
    assert torch.equal(test["ratio_pad"], val["ratio_pad"]) and torch.equal(test["calib"], val["calib"])
    assert test["calib"].dtype == torch.float64 and tuple(test["calib"].shape) == (2, 6)
    assert test["im_file"] == val["im_file"] == [f"{i:06d}.txt" for i in FRAMES]
    for a, b in zip(test["info"], val["info"]):
        assert np.array_equal(a["trans_inv"], b["trans_inv"]) and a["img_id"] == b["img_id"] and np.array_equal(a["img_size"], b["img_size"])
    assert all(np.array_equal(a, b) for a, b in zip(test["ori_shape"], val["ori_shape"]))
    assert test["P2"].dtype == torch.float32 and tuple(test["P2"].shape) == (2, 3, 4)
    assert np.array_equal(test["P2"].cpu().numpy(), np.stack(_frames(tree)[1]))
    by_file = kitti.build_test_batch(os.path.join(root, "ImageSets", "test.txt"), [1], DEV, img_mode="float", resolution=RES)
    assert by_file["img"].dtype == torch.float32 and tuple(by_file["img"].shape) == (1, 3, RES[1], RES[0]) and by_file["im_file"] == ["000007.txt"]


def test_predict_split_writes_what_it_returns(tree, model, tmp_path):
    y3d.set_compute_dtype(torch.float32)
    root, z = tree
    rgb, P2s = _frames(tree)
    conf = _threshold(model, rgb, P2s)
    pr = predict.Predictor3d(model, conf=conf, resolution=RES)
    results = pr.predict_split(root, [0, 1], out_dir=str(tmp_path))
    files = [f"{i:06d}.txt" for i in FRAMES]
    assert list(results) == files and 0 < sum(len(r) for r in results.values()) < 100
    # the split's frames are the frames the predictor was given directly
    rows, _, _, counts = pr(rgb, P2s, static=True)
    assert results == predict.kitti_results(rows, counts, files)
    assert pr.predict_split(root, [0, 1]) == results and sorted(os.listdir(str(tmp_path))) == ["preds"]
    # read back: the returned results rounded to two decimals, as save_results writes them
    _, annos = kitti_eval.results_to_annos(results)
    for f, want in zip(files, annos):
        got = kitti_eval.read_label_file(os.path.join(str(tmp_path), "preds", f), det=True)
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (f, k)
