"""Host: the rect validation split (`yolo2d.RectSplit`) and the predictor's letter-box / scale-back parameters against the reference's
recorded numbers (tests/golden/yolo2d_rect.npz, tools/make_golden_rect.py), the numpy yardstick of the letter-box kernel
(tests/letterbox_ref.py) against hand-computed cases, and the refusals."""
import os

import numpy as np
import pytest
import torch

import letterbox_ref as LR
import yolo2d_tree as T
from conftest import GOLDEN

import yolov10_3d_amd as y3d
from yolov10_3d_amd import predict, yolo2d
from yolov10_3d_amd._lib import parse_header

Z = dict(np.load(os.path.join(GOLDEN, "yolo2d_rect.npz")))
IMGSZ, STRIDE, PAD = int(Z["imgsz"]), int(Z["stride"]), float(Z["pad"])


@pytest.fixture(scope="module")
def img_dir(tmp_path_factory):
    return T.write_tree(str(tmp_path_factory.mktemp("rect")), T.fixture()["label_text"])


def _split(img_dir, name):
    return yolo2d.RectSplit(img_dir, IMGSZ, int(Z[f"{name}/batch"]), STRIDE, PAD)


@pytest.mark.parametrize("name", [str(n) for n in Z["rect_sets"]])
def test_rect_split_replays_set_rectangle(img_dir, name):
    sp = _split(img_dir, name)
    assert np.array_equal(sp.irect, Z[f"{name}/irect"])
    assert np.array_equal(sp.batch_shapes, Z[f"{name}/batch_shapes"]) and sp.batch_shapes.dtype.kind == "i"
    assert [os.path.basename(f) for f in sp.im_files] == [str(f) for f in Z[f"{name}/files"]]
    assert [sp.batch_of(i) for i in range(len(sp))] == [int(k) for k in Z[f"{name}/batch_of"]]
    want = [[i for i in range(len(sp)) if Z[f"{name}/batch_of"][i] == k] for k in range(len(sp.batch_shapes))]
    assert sp.batches() == want and sum(len(b) for b in want) == 12
    plain = yolo2d.Split(img_dir, IMGSZ, 4, augment=False)
    for n, i in enumerate(sp.irect):  # files, labels and sizes move together
        assert sp.im_files[n] == plain.im_files[i] and sp.size(n) == plain.size(i) and np.array_equal(sp.labels[n], plain.labels[i])


def test_rect_sets_cover_the_branches():
    assert [tuple(r) for r in Z["b4/batch_shapes"]] == [(64, 96), (96, 96), (96, 64)]
    assert np.bincount(Z["b5/batch_of"]).tolist() == [5, 5, 2]


@pytest.mark.parametrize("name", [str(n) for n in Z["rect_sets"]])
def test_rect_samples_are_exact(img_dir, name):
    sp = _split(img_dir, name)
    for i in range(len(sp)):
        s = yolo2d.rect_sample(sp, i)
        assert (s["h0"], s["w0"]) == tuple(Z[f"{name}/ori_shape"][i])
        assert (s["h"], s["w"]) == tuple(Z[f"{name}/hw"][i])  # new_unpad: the letter-box ratio is 1
        assert s["canvas"] == tuple(Z[f"{name}/resized_shape"][i]) == tuple(sp.batch_shapes[sp.batch_of(i)])
        assert s["ratio_pad"][0] == tuple(Z[f"{name}/ratio"][i])  # float64, ==
        assert s["ratio_pad"][1] == (s["left"], s["top"]) == tuple(Z[f"{name}/left_top"][i])
        assert s["rgb"]


@pytest.fixture(scope="module")
def tiny2d():
    cfg = y3d.yaml_model_load("yolov10n.yaml")
    cfg.update(nc=20, scales={"n": [0.33, 0.125, 1024]}, scale="n")
    torch.manual_seed(0)
    return y3d.YOLOv10DetectionModel(cfg)


@pytest.mark.parametrize("name", [str(n) for n in Z["predict_sets"]])
def test_predict_parameters_are_the_references(tiny2d, name):
    shapes = [tuple(int(v) for v in s) for s in Z[f"{name}/shapes"]]
    lbs, canvas = predict.pre_transform_params(shapes, IMGSZ, STRIDE)
    assert canvas == tuple(Z[f"{name}/canvas"])
    assert [lb["new_unpad"] for lb in lbs] == [tuple(v) for v in Z[f"{name}/new_unpad"]]
    assert [(lb["top"], lb["bottom"], lb["left"], lb["right"]) for lb in lbs] == [tuple(v) for v in Z[f"{name}/borders"]]
    rec, meta, hw = predict.Predictor(tiny2d, IMGSZ, stride=STRIDE).plan(shapes)
    assert hw == canvas and rec.dtype == np.int32 and meta.dtype == np.float32
    for b, shape in enumerate(shapes):
        gain, pad = predict.scale_params(canvas, shape)
        assert gain == Z[f"{name}/gain"][b] and tuple(pad) == tuple(Z[f"{name}/pad"][b])
        nw, nh = Z[f"{name}/new_unpad"][b]
        top, _, left, _ = Z[f"{name}/borders"][b]
        assert rec[b].tolist() == [b, shape[0], shape[1], nh, nw, top, left, 1]
        assert meta[b].tolist() == [shape[0], shape[1], float(np.float32(gain)), pad[0], pad[1]]
    # the numpy restatement of the row kernel reproduces the reference's scale_boxes + clip_boxes bit for bit
    for b in range(len(shapes)):
        rows = np.concatenate([Z[f"{name}/boxes_in"][b], np.full((24, 1), 0.9, np.float32), np.zeros((24, 1), np.float32)], 1)
        out, counts = LR.predict_rows(rows[None], meta[b:b + 1], 0.25)
        assert counts.tolist() == [24] and np.array_equal(out[0, :, :4], Z[f"{name}/boxes_out"][b])


def test_round_half_even_and_odd_pads():
    lb = yolo2d.letterbox_params((128, 37), 64)
    assert lb["new_unpad"] == (18, 64) and (lb["left"], lb["right"]) == (23, 23)  # 18.5 -> 18
    lb = yolo2d.letterbox_params((48, 32), 64)
    assert lb["new_unpad"] == (43, 64) and (lb["left"], lb["right"]) == (10, 11) and lb["dw"] == 10.5
    lb = yolo2d.letterbox_params((32, 64), 64, auto=True)
    assert lb["canvas"] == (32, 64) and (lb["top"], lb["bottom"], lb["left"], lb["right"]) == (0, 0, 0, 0)
    lb = yolo2d.letterbox_params((32, 48), (64, 96), scaleup=False)
    assert lb["r"] == 1.0 and lb["new_unpad"] == (48, 32) and (lb["top"], lb["left"]) == (16, 24)


def test_letterbox_ref_by_hand():
    # copy + odd pads: 2 x 3 into 3 x 8 -> dh = 0.5 (top 0, bottom 1), dw = 2.5 (left 2, right 3)
    src = np.arange(18, dtype=np.uint8).reshape(2, 3, 3)
    lb = yolo2d.letterbox_params((2, 3), (3, 8), scaleup=False)
    assert (lb["top"], lb["bottom"], lb["left"], lb["right"]) == (0, 1, 2, 3)
    out = LR.letterbox(src, 2, 3, lb["top"], lb["left"], 3, 8)
    want = np.full((3, 8, 3), 114, np.uint8)
    want[0:2, 2:5] = src
    assert np.array_equal(out, want)
    assert np.array_equal(LR.letterbox(src, 2, 3, 0, 2, 3, 8, swap_rb=True)[0:2, 2:5], src[..., ::-1])
    # 2 x 2 -> 4 x 4: source coordinates -0.25, 0.25, 0.75, 1.25 -> weights (1, 0), (.75, .25), (.25, .75), (0, 1); x first, then y
    src = np.zeros((2, 2, 3), np.uint8)
    src[..., 0] = [[0, 100], [200, 40]]
    out = LR.letterbox(src, 4, 4, 0, 0, 4, 4)[..., 0]
    assert out.tolist() == [[0, 25, 75, 100], [50, 59, 76, 85], [150, 126, 79, 55], [200, 160, 80, 40]]  # 58.75, 76.25, 126.25, 78.75
    # a 1-pixel-wide source, 3 x 1 -> 6 x 2: the column is repeated, the rows are 10, 20, 40, 60, 80, 90
    src = np.array([10, 50, 90], np.uint8).reshape(3, 1, 1).repeat(3, 2)
    out = LR.letterbox(src, 6, 2, 1, 1, 8, 4)
    assert out[1:7, 1:3, 1].tolist() == [[v, v] for v in (10, 20, 40, 60, 80, 90)]
    assert (out[0] == 114).all() and (out[7] == 114).all() and (out[:, 0] == 114).all() and (out[:, 3] == 114).all()
    # canvas(): a bad record is an all-114 image
    cv = LR.canvas([src], np.array([[0, 3, 1, 6, 2, 1, 1, 0], [1, 3, 1, 6, 2, 1, 1, 0]]), 8, 4)
    assert np.array_equal(cv[0], out) and (cv[1] == 114).all()
    assert LR.to_float(cv).dtype == np.float32 and LR.to_float(cv)[1, 0, 0, 0] == np.float32(114) / np.float32(255)


def test_refusals(img_dir, tiny2d):
    sp = _split(img_dir, "b4")
    args = yolo2d.data_args()
    with pytest.raises(y3d.Y3DError, match="rect batches"):
        yolo2d.build_batch(sp, [3, 4], args, "cuda", mode="val")
    with pytest.raises(y3d.Y3DError, match="validation batches only"):
        yolo2d.build_batch(sp, [0, 1], args, "cuda", mode="train")
    with pytest.raises(y3d.Y3DError, match="validation batches only"):
        yolo2d.build_batch(sp, [0, 1], args, "cuda")  # the default mode is "train"
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        yolo2d.build_batch(sp, [0, 1], args, "cpu", mode="val")
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        yolo2d.RectSplit(img_dir, IMGSZ, 4, stride=6)
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        yolo2d.pack_letterbox([], np.zeros((1, 8), np.int32), 32, 30, "cuda")
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        predict.Predictor(tiny2d, imgsz=62)
    with pytest.raises(y3d.Y3DError, match="rect=True"):
        yolo2d.Split(img_dir, IMGSZ, 4, rect=True)


def test_predictor_refuses_3d_models_and_host_tensors(tiny2d):
    cfg = y3d.yaml_model_load("yolov10s_3D.yaml")
    cfg.update(scales={"n": [0.33, 0.125, 1024]}, scale="n",
               channels={k + "_c": 16 for k in ("cls", "o2d", "s2d", "o3d", "s3d", "hd", "dep", "dep_un")})
    with pytest.raises(y3d.Y3DError, match="3D models"):
        predict.Predictor(y3d.YOLOv10_3DDetectionModel(cfg))
    with pytest.raises(y3d.Y3DError, match="HIP device"):  # a model on the host: no fallback
        predict.Predictor(tiny2d, IMGSZ)([np.zeros((8, 8, 3), np.uint8)])


def test_abi_declares_the_three_entries():
    protos = parse_header()
    assert {"y3d_letterbox_image", "y3d_letterbox_labels", "y3d_predict_rows"} <= set(protos)
    assert len(protos["y3d_letterbox_image"][1]) == 9 and len(protos["y3d_letterbox_labels"][1]) == 13 and len(protos["y3d_predict_rows"][1]) == 10
