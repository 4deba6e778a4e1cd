"""CPU: the host side of the resident 2D splits (yolo2d.DeviceSplit / DeviceRectSplit).  The numpy restatement of the plan kernel
(tests/yolo2d_cache_ref.py) against the host functions it replaces (`image_records`, `label_records`, `hsv_luts`) with slots and label
rows taken split-wide, on every recorded sample of tests/yolo2d_tree.py; the draw table's round trip; the refusal of a host device
before any file is read; the byte budget from the headers alone; the kernel's declaration."""
import os
import re

import numpy as np
import pytest

import yolo2d_cache_ref as R
import yolo2d_tree as T
from conftest import ROOT

from yolov10_3d_amd import _lib, yolo2d
from yolov10_3d_amd._lib import Y3DError

S = T.IMGSZ
NAMES = list(T.ARGSETS)


def tables():
    """the frame tables of the twelve-frame tree as a resident split holds them, and the host functions' view of the same"""
    rows = T.label_rows()
    n = [len(r) for r in rows]
    span = np.zeros((len(rows), 2), np.int32)
    span[:, 1] = n
    span[1:, 0] = np.cumsum(n)[:-1]
    hw = np.array([(h, w) for w, h in T.FRAME_WH], np.int32)
    return hw, span, rows


def recorded(name):
    return [T.sample(name, n) for n in range(len(T.fixture()[f"{name}/counts"]))]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_host_records(name):
    hw, span, rows = tables()
    samples = recorded(name)
    assert len(samples) == len(T.ARGSETS[name][3])
    got = R.plan(hw, span, S, yolo2d.draw_table(samples))
    ri, rf, lut = yolo2d.image_records(samples, {f: f for f in range(len(hw))})
    from types import SimpleNamespace
    li, lf = yolo2d.label_records(SimpleNamespace(labels=rows), samples, {f: int(span[f, 0]) for f in range(len(hw))})
    want = {"rec_i": ri, "rec_f": rf, "lut": lut, "lab_i": li, "lab_f": lf}
    for k, dt, s in R.OUTPUTS:
        assert got[k].dtype == want[k].dtype == dt and got[k].shape == want[k].shape == (len(samples),) + s, k
        assert (got[k] == want[k]).all(), (name, k, np.argwhere(got[k] != want[k])[:5])
        assert got[k].tobytes() == want[k].tobytes(), (name, k)  # (also the sign of a zero)
    if name == "default":
        assert any(s["pre2"] is not None and s["pre2"]["mosaic"] for s in samples) and any(s["hsv_gain"] is not None for s in samples)
        assert (lut != 0).any()
    if name == "val":
        assert not lut.any() and (li[:, 16] == 1).all()


@pytest.mark.parametrize("gain", [(1.015, 1.7, 1.4), (0.985, 0.3, 0.6), (1.0, 1.0, 1.0), (1.0149999, 0.3000001, 1.3999), (1.5, 2.5, 0.0)])
def test_restated_tables_equal_hsv_luts(gain):
    got, want = R.luts(np.array(gain, np.float64)), yolo2d.hsv_luts(gain)
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape == (3, 256) and (got == want).all()


@pytest.mark.parametrize("name", NAMES)
def test_draw_table_round_trip(name):
    samples = recorded(name)
    d = yolo2d.draw_table(samples)
    assert d.dtype == np.float64 and d.shape == (len(samples), yolo2d._DRAW_W) and np.isfinite(d).all()
    for row, s in zip(d, samples):
        for l, pre in enumerate((s["pre"], s["pre2"])):
            L = row[l * R.LAYER:(l + 1) * R.LAYER]
            if pre is None:
                assert not L.any()
                continue
            frames = [t["frame"] for t in pre["tiles"]]
            assert L[:3].tolist() == [1.0, float(pre["mosaic"]), float(pre["warp"])]
            assert L[3:7].tolist() == [float(f) for f in frames] + [-1.0] * (4 - len(frames)) and len(frames) == (4 if pre["mosaic"] else 1)
            assert L[7:10].tolist() == [float(pre["yc"]), float(pre["xc"]), float(pre["canvas"])]
            M = np.asarray(pre["M"], np.float32)[:2].reshape(6)
            assert L[10:16].astype(np.float32).tobytes() == M.tobytes() and (L[10:16] == M.astype(np.float64)).all()
            assert L[16:22].tobytes() == np.asarray(pre["M_inv"], np.float64).tobytes()
            assert L[22] == pre["scale"] and type(pre["scale"]) is float
        t = row[R.TAIL:]
        hsv = s["hsv_gain"] is not None
        assert t[0] == float(s["pre2"] is not None) == float(s["mix"]) and t[1] == s["r"] and t[2] == float(hsv)
        assert t[3:6].tobytes() == (np.asarray(s["hsv_gain"], np.float64) if hsv else np.zeros(3)).tobytes()
        assert t[6:10].tolist() == [float(s["flipud"]), float(s["fliplr"]), float(not s["rgb"]), 0.0]


def test_draw_width_is_named_in_the_header():
    src = open(os.path.join(ROOT, "include", "y3d.h")).read()
    assert int(re.search(r"\bY3D_YOLO2D_DRAW_W\s*=\s*(\d+)", src).group(1)) == yolo2d._DRAW_W == R.DRAW_W == 2 * R.LAYER + 10
    protos = _lib.parse_header()
    assert "y3d_yolo2d_plan_batch" in protos
    assert len(protos["y3d_yolo2d_plan_batch"][1]) == 13  # 2 frame tables, N, imgsz, draws (host, device), B, 5 outputs, stream
    assert [k for k, _, _ in yolo2d.PLAN_TABLES] == [k for k, _, _ in R.OUTPUTS]
    assert [tuple(s) for _, _, s in yolo2d.PLAN_TABLES] == [s for _, _, s in R.OUTPUTS]


@pytest.mark.parametrize("cls", ["DeviceSplit", "DeviceRectSplit"])
def test_resident_split_refuses_a_host_device_before_reading(tmp_path, cls):
    nowhere = os.path.join(str(tmp_path), "no_such_tree")
    with pytest.raises(Y3DError, match="HIP device"):
        getattr(yolo2d, cls)(nowhere, S, 4, device="cpu")
    with pytest.raises(Y3DError, match="HIP device"):
        getattr(yolo2d, cls)(nowhere, S, 4, device="cpu", max_bytes=1)
    assert not os.path.exists(nowhere)
    assert issubclass(yolo2d.DeviceSplit, yolo2d.Split) and issubclass(yolo2d.DeviceRectSplit, yolo2d.RectSplit)


@pytest.mark.parametrize("cls", ["DeviceSplit", "DeviceRectSplit"])
def test_budget_is_checked_before_any_decode(tmp_path, monkeypatch, cls):
    from PIL import ImageOps
    img_dir = T.write_tree(str(tmp_path), T.fixture()["label_text"])
    calls = []
    monkeypatch.setattr(yolo2d, "_decode_rgb", lambda path: calls.append(path))
    monkeypatch.setattr(ImageOps, "exif_transpose", lambda im, **kw: calls.append(im))
    need = sum((w * h * 3 + 15) // 16 * 16 for w, h in T.FRAME_WH)
    with pytest.raises(Y3DError, match=f"{need} bytes.* 1 bytes"):
        getattr(yolo2d, cls)(img_dir, S, 4, device="cuda", max_bytes=1)
    assert calls == []
