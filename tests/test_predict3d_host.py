"""Host: the 3D predictor's host arithmetic (`Predictor3d.plan`), the numpy restatement of the box corners (tests/predict3d_ref.py),
`kitti.save_results`, `predict.kitti_results` and the refusals against the reference's recorded numbers (tests/golden/predict3d.npz,
tools/make_golden_predict3d.py); the new entry in the ABI and the kernel's resource report."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import predict3d_ref as PR
from conftest import ROOT

import yolov10_3d_amd as y3d
from yolov10_3d_amd import kitti, predict
from yolov10_3d_amd._lib import parse_header

Z = PR.fixture()
FILES = [str(f) for f in Z["files"]]


def _model3d():
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    torch.manual_seed(0)
    return y3d.YOLOv10_3DDetectionModel(cfg)


@pytest.fixture(scope="module")
def model3d():
    return _model3d()


def test_fixture_has_what_the_tests_rely_on():
    assert Z["t25/counts"].tolist() == [7, 3, 9] and Z["class_counts_t25/c0"].tolist() == [0, 1, 5]
    assert (Z["t001/counts"] >= Z["t25/counts"]).all() and (Z["t001/counts"] < 12).all()
    assert Z["P2"].dtype == np.float32 and (Z["P2"][:, 2, 3] == np.float32(0.004981016)).all()
    for tag in ("t001", "t25"):
        for b, n in enumerate(Z[f"{tag}/counts"]):
            assert Z[f"{tag}/corners3d"][b, :n, :, 2].min() >= 1.0 and not Z[f"{tag}/rows"][b, n:].any()
    g = PR.decode_fixture()  # the class masks are over the decode fixture's label column
    for tag in ("c0", "c12", "c2"):
        assert np.array_equal(Z[f"class_mask/{tag}"], np.isin(g["preds"][..., 36].astype(np.int64), Z[f"classes/{tag}"]))
    assert Z["class_mask/none"].all()


@pytest.mark.parametrize("res", [(1280, 384), (320, 256)])
def test_plan_is_the_references_unaugmented_sample(model3d, res):
    pr = predict.Predictor3d(model3d, resolution=res)
    sizes = [tuple(int(v) for v in s) for s in Z["plan_sizes"]]  # (W, H)
    P2s = [Z["P2"][i % 3] for i in range(len(sizes))]
    p = pr.plan([(h, w) for w, h in sizes], P2s)
    name = f"plan_{res[0]}x{res[1]}"
    assert p["trans_inv"].dtype == p["ratio"].dtype == p["calib6"].dtype == np.float64 and p["P2"].dtype == np.float32
    assert np.array_equal(p["trans_inv"], Z[f"{name}/trans_inv"])
    assert np.array_equal(p["ratio"], Z[f"{name}/ratio"])
    for (w, h), t in zip(sizes, Z[f"{name}/trans"]):
        assert np.array_equal(kitti.get_affine_transform(np.array([w, h]) / 2, np.array([w, h]), res), t)
    g = PR.decode_fixture()
    assert np.array_equal(p["calib6"], g["calib"][[i % 3 for i in range(len(sizes))]])  # Calibration's own six numbers
    assert np.array_equal(p["P2"], np.stack(P2s))


@pytest.mark.parametrize("tag", ["t001", "t25"])
def test_restatement_gives_the_references_corners(tag):
    seen = 0
    for b, n in enumerate(Z[f"{tag}/counts"]):
        c3, ci = PR.corners(Z[f"{tag}/rows"][b, :n], Z["P2"][b])
        np.testing.assert_allclose(c3, Z[f"{tag}/corners3d"][b, :n], rtol=0, atol=1e-9)
        np.testing.assert_allclose(ci, Z[f"{tag}/corners_img"][b, :n], rtol=1e-9, atol=1e-9)
        seen += n
    assert seen == Z[f"{tag}/counts"].sum() > 0
    # by hand: a 2 x 4 x 6 (h, w, l) box at (1, 2, 10), heading 0 and pi / 2, through P = [[2, 0, 3, 4], [0, 2, 5, 6], [0, 0, 1, 0.5]]
    row = np.zeros((2, 14))
    row[:, 6:12] = (2, 4, 6, 1, 2, 10)
    row[1, 12] = np.pi / 2
    c3, ci = PR.corners(row, [[2, 0, 3, 4], [0, 2, 5, 6], [0, 0, 1, 0.5]])
    assert c3[0].tolist() == [[4, 2, 12], [4, 2, 8], [-2, 2, 8], [-2, 2, 12], [4, 0, 12], [4, 0, 8], [-2, 0, 8], [-2, 0, 12]]
    np.testing.assert_allclose(c3[1], [[3, 2, 7], [-1, 2, 7], [-1, 2, 13], [3, 2, 13], [3, 0, 7], [-1, 0, 7], [-1, 0, 13], [3, 0, 13]], atol=1e-14)
    assert ci[0, 0].tolist() == [(2 * 4 + 3 * 12 + 4) / 12.5, (2 * 2 + 5 * 12 + 6) / 12.5]


def _results(tag):
    return {f: Z[f"{tag}/rows"][b, :n].tolist() for b, (f, n) in enumerate(zip(FILES, Z[f"{tag}/counts"]))}


def test_save_results_writes_the_references_bytes(tmp_path):
    out = kitti.save_results(_results("t25"), str(tmp_path))
    assert out == os.path.join(str(tmp_path), "preds") and sorted(os.listdir(out)) == FILES
    for f, text in zip(FILES, Z["save_text"]):
        assert open(os.path.join(out, f), "rb").read() == str(text).encode()
    assert str(Z["save_text"][1]).count("\n") == 3 and str(Z["save_text"][0]).split(" ")[1:3] == ["0.0", "0"]
    # an image without detections gets an empty file; an existing directory is reused
    kitti.save_results({"000009.txt": []}, str(tmp_path))
    assert open(os.path.join(out, "000009.txt")).read() == ""


def test_kitti_results_round_trips():
    rows, counts = torch.from_numpy(Z["t25/rows"]), torch.from_numpy(Z["t25/counts"]).int()
    res = predict.kitti_results(rows, counts, FILES)
    assert res == _results("t25")
    assert predict.kitti_results([rows[b, :n] for b, n in enumerate(counts.tolist())], None, FILES) == res
    assert list(res) == FILES and [len(res[f]) for f in FILES] == [7, 3, 9]
    # what kitti.decode_preds returns is what kitti_eval.results_to_annos takes
    from yolov10_3d_amd import kitti_eval
    files, annos = kitti_eval.results_to_annos(res)
    assert files == FILES and [len(a["name"]) for a in annos] == [7, 3, 9]
    with pytest.raises(y3d.Y3DError, match="file names"):
        predict.kitti_results(rows, counts, FILES[:2])
    with pytest.raises(y3d.Y3DError, match="counts"):
        predict.kitti_results(rows, torch.tensor([13, 0, 0]), FILES)


def test_refusals(model3d, tmp_path):
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=20, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    with pytest.raises(y3d.Y3DError, match="3D model"):  # a 2D model
        predict.Predictor3d(y3d.YOLOv10DetectionModel(cfg))
    with pytest.raises(y3d.Y3DError, match="stride"):  # 1242 x 375: the raw KITTI size
        predict.Predictor3d(model3d, resolution=(1242, 375))
    with pytest.raises(y3d.Y3DError, match="stride"):
        predict.Predictor3d(model3d, resolution=(320, 250))
    pr = predict.Predictor3d(model3d, resolution=(320, 256))
    im, P = np.zeros((61, 97, 3), np.uint8), Z["P2"][0]
    with pytest.raises(y3d.Y3DError, match="HIP device"):  # a model on the host: no fallback
        pr([im], [P])
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        pr.predict_split(str(tmp_path), [0])
    with pytest.raises(y3d.Y3DError, match="P2 matrices"):  # a length mismatch
        pr([im, im], [P])
    with pytest.raises(y3d.Y3DError, match="P2 matrices"):
        pr.plan([(61, 97)], [P, P])
    with pytest.raises(y3d.Y3DError, match=r"\(3, 4\)"):
        pr.plan([(61, 97)], [P[:, :3]])
    with pytest.raises(y3d.Y3DError, match="non-empty list"):
        pr([], [])
    # the row pass: host tensors, shapes, classes
    good = torch.zeros(3, 12, 37)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        predict.predict3d_rows(good, Z["P2"][:, :2, :3].reshape(3, 6), Z["P2"], np.ones((3, 2)), None, 0.25)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        predict.predict3d_rows(torch.zeros(3, 12, 36), None, None, None, None, 0.25)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        kitti.build_test_batch(str(tmp_path), [0], "cpu")
    # the entry refuses outputs that overlap an input or each other, at an offset too (checked before anything is launched)
    M = 1 << 20
    ptr = dict(preds=1 * M, calib=2 * M, P2=3 * M, ratio=4 * M, inv=5 * M, ms=6 * M, cls=7 * M, rows=8 * M, c3=9 * M, ci=10 * M, counts=11 * M)
    call = lambda **o: (lambda q: y3d.lib().predict3d_rows(q["preds"], 3, 12, q["calib"], q["P2"], q["ratio"], q["inv"], q["ms"], 3, 0, 0.25,
                                                           q["cls"], 2, q["rows"], q["c3"], q["ci"], q["counts"], None))(dict(ptr, **o))
    with pytest.raises(y3d.Y3DError, match="overlaps an input"):
        call(rows=ptr["preds"] + 3 * 12 * 37 * 4 - 16)  # the last 16 bytes of preds
    with pytest.raises(y3d.Y3DError, match="overlaps an input"):
        call(counts=ptr["cls"] + 4)
    with pytest.raises(y3d.Y3DError, match="overlap each other"):
        call(c3=ptr["rows"] + 3 * 12 * 14 * 8 - 16)
    with pytest.raises(y3d.Y3DError, match="16-byte aligned"):
        call(ci=ptr["ci"] + 8)
    # the 2D predictor still refuses 3D models, and the labelled builder the test split
    with pytest.raises(y3d.Y3DError, match="3D models"):
        predict.Predictor(model3d)
    with pytest.raises(y3d.Y3DError, match="no labels"):
        kitti.build_batch(str(tmp_path), [0], kitti.data_args(), "cuda", mode="test")


def test_abi_declares_the_entry_and_the_kernel_has_no_scratch():
    protos = parse_header()
    assert "y3d_predict3d_rows" in protos and len(protos["y3d_predict3d_rows"][1]) == 18
    assert hasattr(y3d.lib()._dll, "y3d_predict3d_rows")
    spec = importlib.util.spec_from_file_location("y3d_build", os.path.join(ROOT, "yolov10-3d_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    usage = mod.resource_usage()
    assert "predict3d.hip" in usage
    k = {n: u for n, u in usage["predict3d.hip"].items() if "predict3d_rows_kernel" in n}
    assert len(k) == 1
    u = next(iter(k.values()))
    print(f"predict3d_rows_kernel: {u}")
    assert u["scratch"] == 0 and u["lds"] == 16 and u["vgprs"] <= 256
    # the decode kernel shares the row function and stays without scratch too
    d = [u for n, u in usage["post.hip"].items() if "kitti_decode_kernel" in n]
    assert len(d) == 1 and d[0]["scratch"] == 0
