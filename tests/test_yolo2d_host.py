"""CPU: the host side of yolo2d (2D training batches): the replay of the reference's recorded random draws and matrices
(tests/golden/yolo2d_labels.npz), a numpy float32 emulation of the label arithmetic against the reference's collated batches,
tests/yolo2d_ref.py (the image yardstick of the kernel) against hand-computed cases, and the refusals."""
import json
import random

import numpy as np
import pytest

import yolo2d_ref as YR
import yolo2d_tree as T

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib, yolo2d

NAMES = list(T.ARGSETS)


def test_header_lists_both_symbols():
    protos = _lib.parse_header()
    assert "y3d_yolo2d_image_aug" in protos and "y3d_yolo2d_encode_labels" in protos
    assert len(protos["y3d_yolo2d_image_aug"][1]) == 10 and len(protos["y3d_yolo2d_encode_labels"][1]) == 12
    assert y3d.yolo2d is yolo2d


def test_data_args_are_the_defaults():
    a = yolo2d.data_args()
    assert (a.mosaic, a.mixup, a.scale, a.translate, a.hsv_h, a.hsv_s, a.hsv_v, a.fliplr) == (1.0, 0.5, 0.4, 0.1, 0.015, 0.7, 0.4, 0.5)
    assert (a.degrees, a.shear, a.perspective, a.flipud, a.bgr, a.copy_paste) == (0.0,) * 6
    assert yolo2d.data_args(mixup=0.0).mixup == 0.0
    with pytest.raises(ValueError):
        yolo2d.data_args(mosiac=1.0)


def test_fixture_covers_what_it_must():
    z = T.fixture()
    assert list(z["argsets"]) == NAMES and int(z["imgsz"]) == T.IMGSZ and np.array_equal(z["frame_wh"], T.FRAME_WH)
    counts = np.concatenate([z[f"{n}/counts"] for n in NAMES])
    assert len(counts) == sum(len(v[3]) for v in T.ARGSETS.values()) >= 40
    assert (counts > 64).any() and (counts > 128).any() and (z["default/counts"] > 128).any()
    rows = T.label_rows()
    n = [len(r) for r in rows]
    assert 0 in n and sum(25 <= k <= 40 for k in n) >= 5 and len(n) == 12
    wh = np.array(T.FRAME_WH)
    assert (wh[:, 0] > wh[:, 1]).any() and (wh[:, 0] < wh[:, 1]).any() and (wh[:, 0] == wh[:, 1]).any()
    assert wh.max(1).min() < T.IMGSZ < wh.max(1).max() <= 100


@pytest.mark.parametrize("name", NAMES)
def test_sample_augment_replays_the_recorded_draws(tmp_path, name):
    """Seeded as the fixture was, every draw equals the reference's (float64, ==), the buffer picks included, and M equals the
    reference's float32 matrix bit for bit (observed: equal in all 59 recorded matrices; the bound is 1 ulp)"""
    z = T.fixture()
    mode, over, seed, items = T.ARGSETS[name]
    assert json.loads(str(z[f"{name}/over"])) == over and int(z[f"{name}/seed"]) == seed and list(z[f"{name}/items"]) == items
    split = yolo2d.Split(T.write_tree(str(tmp_path), z["label_text"]), T.IMGSZ, T.BATCH, augment=mode == "train")
    assert len(split) == 12 and split.max_buffer_length == (12 if mode == "train" else 0)
    assert all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(split.labels, T.label_rows()))
    args = yolo2d.data_args(**over)
    random.seed(seed)
    np.random.seed(seed)
    n_m = 0
    for n, item in enumerate(items):
        got, want = yolo2d.sample_augment(split, item, args, mode), T.sample(name, n)
        assert T.flat_draws(got) == T.flat_draws(want), f"sample {n}"
        for key in ("index", "mix", "partner", "flipud", "fliplr", "rgb"):
            assert got[key] == want[key], (n, key)
        for g, w in ((got["pre"], want["pre"]), (got["pre2"], want["pre2"])):
            assert (g is None) == (w is None)
            if g is None:
                continue
            assert g["tiles"] == w["tiles"] and (g["mosaic"], g["yc"], g["xc"], g["canvas"], g["warp"]) == (w["mosaic"], w["yc"], w["xc"], w["canvas"], w["warp"])
            if g["warp"]:
                ulp = np.abs(g["M"].view(np.int32).astype(np.int64) - w["M"].view(np.int32).astype(np.int64)).max()
                assert g["M"].dtype == np.float32 and ulp <= 1
                assert bool(ulp == 0) == bool(z[f"{name}/m_equal"][n_m])
                n_m += 1
                assert np.array_equal(g["M_inv"], yolo2d.invert_affine(g["M"])) and g["M_inv"].dtype == np.float64
                full = np.vstack([g["M_inv"].reshape(2, 3), [0, 0, 1]]) @ g["M"].astype(np.float64)
                np.testing.assert_allclose(full, np.eye(3), atol=1e-9)
    assert n_m == len(z[f"{name}/m_equal"]) and z[f"{name}/m_equal"].all()


@pytest.mark.parametrize("name", NAMES)
def test_label_arithmetic_in_numpy_matches_the_reference(name):
    """the float32 emulation, fed the recorded draws: survivors, order, counts and classes exact, boxes within the label bound"""
    z, rows = T.fixture(), T.label_rows()
    cls, box, bidx = [], [], []
    for n in range(len(T.ARGSETS[name][3])):
        c, b, _ = YR.labels(T.sample(name, n), rows, T.IMGSZ)
        assert len(b) == int(z[f"{name}/counts"][n])
        cls.append(c)
        box.append(b)
        bidx.append(np.full(len(b), n, np.float32))
    assert np.array_equal(np.concatenate(cls), z[f"{name}/c/cls"]) and np.array_equal(np.concatenate(bidx), z[f"{name}/c/batch_idx"])
    np.testing.assert_allclose(np.concatenate(box), z[f"{name}/c/bboxes"], rtol=1e-6, atol=1e-6)
    assert z[f"{name}/c/cls"].dtype == z[f"{name}/c/bboxes"].dtype == z[f"{name}/c/batch_idx"].dtype == np.float32
    assert z[f"{name}/c/cls"].shape[1:] == (1,) and z[f"{name}/c/bboxes"].shape[1:] == (4,) and z[f"{name}/c/batch_idx"].ndim == 1


def test_buffer_follows_load_image(tmp_path):
    z = T.fixture()
    sp = yolo2d.Split(T.write_tree(str(tmp_path), z["label_text"]), T.IMGSZ, batch=1)  # min(12, 8, 1000) = 8
    assert sp.max_buffer_length == 8
    for i in range(7):
        sp.load(i)
    assert sp.buffer == list(range(7))
    sp.load(3)  # held: no second entry
    assert sp.buffer == list(range(7))
    sp.load(7)  # the eighth entry drops the oldest at once
    assert sp.buffer == list(range(1, 8))
    sp.load(0)  # no longer held: loads again
    assert sp.buffer == [2, 3, 4, 5, 6, 7, 0]
    assert sp.load(0) == ((60, 100), (39, 64)) and sp.load(4) == ((48, 32), (64, 43)) and sp.load(2) == ((64, 64), (64, 64))
    assert yolo2d.img2label_path("/a/images/b/images/c.x.png") == "/a/images/b/labels/c.x.txt"


def test_exif_orientation_is_applied_as_imread_applies_it(tmp_path):
    from PIL import Image
    (tmp_path / "images").mkdir()
    px = T.frame_pixels(1, 12, 8)  # (8, 12, 3), stored with orientation 6: a viewer (and cv2.imread) turns it to 12 x 8
    exif = Image.Exif()
    exif[0x0112] = 6
    Image.fromarray(px, "RGB").save(tmp_path / "images" / "a.png", exif=exif)
    Image.fromarray(px, "RGB").save(tmp_path / "images" / "b.png")
    sp = yolo2d.Split(str(tmp_path / "images"), 16, augment=False)
    assert sp.size(0) == (12, 8) and sp.size(1) == (8, 12)
    a, b = sp.decode(0, "cpu").numpy(), sp.decode(1, "cpu").numpy()
    assert np.array_equal(b, px) and a.shape == (12, 8, 3) and np.array_equal(a, np.rot90(px, -1))
    assert sp.load(0) == ((12, 8), (16, 11))


# ---------------------------------------------------------------------------------------------------------------------------------
# yolo2d_ref against hand-computed cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _tile(frame, h0, w0, h, w, x1a, y1a):
    return dict(frame=frame, h0=h0, w0=w0, h=h, w=w, x1a=x1a, y1a=y1a, x2a=x1a + w, y2a=y1a + h, padw=x1a, padh=y1a, lab_padw=float(x1a),
                lab_padh=float(y1a))


def _pre(tiles, canvas, inv=(1.0, 0, 0, 0, 1.0, 0), mosaic=False):
    return dict(index=0, mosaic=mosaic, canvas=canvas, tiles=tiles, M=np.eye(3, dtype=np.float32), M_inv=np.array(inv, np.float64), warp=True, scale=1.0)


def _sample(pre, pre2=None, r=1.0, gain=None, flipud=False, fliplr=False, rgb=True):
    return dict(mode="train", pre=pre, pre2=pre2, r=r, hsv_gain=gain, flipud=flipud, fliplr=fliplr, rgb=rgb)


def test_ref_resize_2x2_to_4x4():
    src = np.zeros((2, 2, 3), np.uint8)
    src[..., 0] = [[0, 100], [200, 40]]
    src[..., 1] = 7
    got = YR.resize(src, 4, 4)
    # half-pixel centres: source coordinates -0.25, 0.25, 0.75, 1.25 -> weights (clamped) 0, .25, .75, 1 of the second sample
    w = np.array([0.0, 0.25, 0.75, 1.0])
    top, bot = 0 * (1 - w) + 100 * w, 200 * (1 - w) + 40 * w
    want = np.floor(top[None, :] * (1 - w[:, None]) + bot[None, :] * w[:, None] + 0.5)
    assert np.array_equal(got[..., 0], want.astype(np.uint8)) and (got[..., 1] == 7).all() and (got[..., 2] == 0).all()
    assert list(got[0, :, 0]) == [0, 25, 75, 100] and list(got[:, 0, 0]) == [0, 50, 150, 200] and got[1, 1, 0] == 59  # 25*.75 + 160*.25 = 58.75
    assert np.array_equal(YR.resize(src, 2, 2), src)


def test_ref_identity_returns_the_letterboxed_image():
    img = T.frame_pixels(3, 8, 4)  # (4, 8, 3): letter-boxed into 8 x 8 with two rows of 114 above and below
    out = YR.image(_sample(_pre([_tile(0, 4, 8, 4, 8, 0, 2)], 8)), {0: img}, 8)
    assert np.array_equal(out[2:6], img) and (out[:2] == 114).all() and (out[6:] == 114).all()


def test_ref_integer_translation_moves_pixels_exactly():
    img = T.frame_pixels(5, 8, 8)
    # forward map x' = x + 3, y' = y - 2: the inverse is x = x' - 3, y = y' + 2
    out = YR.image(_sample(_pre([_tile(0, 8, 8, 8, 8, 0, 0)], 8, inv=(1.0, 0, -3.0, 0, 1.0, 2.0))), {0: img}, 8)
    assert np.array_equal(out[:6, 3:], img[2:, :5]) and (out[:, :3] == 114).all() and (out[6:] == 114).all()
    assert np.array_equal(yolo2d.invert_affine(np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1]], np.float32)), [1.0, 0.0, -3.0, 0.0, 1.0, 2.0])


def test_ref_flips_bgr_and_mixup():
    a, b = T.frame_pixels(1, 8, 8), T.frame_pixels(2, 8, 8)
    pa, pb = _pre([_tile(0, 8, 8, 8, 8, 0, 0)], 8), _pre([_tile(1, 8, 8, 8, 8, 0, 0)], 8)
    im = {0: a, 1: b}
    assert np.array_equal(YR.image(_sample(pa, fliplr=True), im, 8), a[:, ::-1])
    assert np.array_equal(YR.image(_sample(pa, flipud=True), im, 8), a[::-1])
    assert np.array_equal(YR.image(_sample(pa, rgb=False), im, 8), a[..., ::-1])
    assert np.array_equal(YR.image(_sample(pa, pb, r=1.0), im, 8), a)  # r = 1 returns the first image
    half = YR.image(_sample(pa, pb, r=0.5), im, 8)
    assert np.array_equal(half, ((a.astype(np.int64) + b) // 2).astype(np.uint8))  # truncation, not rounding
    assert np.array_equal(YR.mixup(np.array([[[255, 0, 9]]], np.uint8), np.array([[[0, 255, 10]]], np.uint8), 0.25), [[[63, 191, 9]]])


def test_ref_mosaic_canvas_places_four_tiles():
    ims = {i: T.frame_pixels(i, 4, 4) for i in range(4)}
    # centre (xc, yc) = (4, 4) on an 8 x 8 canvas (S = 4): four whole tiles, one per quadrant
    tiles = [_tile(0, 4, 4, 4, 4, 0, 0), _tile(1, 4, 4, 4, 4, 4, 0), _tile(2, 4, 4, 4, 4, 0, 4), _tile(3, 4, 4, 4, 4, 4, 4)]
    cv = YR.canvas(_pre(tiles, 8, mosaic=True), ims)
    assert np.array_equal(cv[:4, :4], ims[0]) and np.array_equal(cv[:4, 4:], ims[1]) and np.array_equal(cv[4:, :4], ims[2]) and np.array_equal(cv[4:, 4:], ims[3])
    # the window of the untouched mosaic: C = -S moves the canvas centre to the origin, T = S / 2 puts it at the output's centre
    out = YR.image(_sample(_pre(tiles, 8, inv=(1.0, 0, 2.0, 0, 1.0, 2.0), mosaic=True)), ims, 4)
    assert np.array_equal(out, cv[2:6, 2:6])


def test_ref_zero_hsv_gains_skip_the_stage():
    img = T.frame_pixels(7, 8, 8)
    pre = _pre([_tile(0, 8, 8, 8, 8, 0, 0)], 8)
    assert np.array_equal(YR.image(_sample(pre, gain=None), {0: img}, 8), img)
    args = yolo2d.data_args(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, mosaic=0.0, mixup=0.0)
    assert not (args.hsv_h or args.hsv_s or args.hsv_v)
    lut = yolo2d.hsv_luts([1.0, 1.0, 1.0])
    assert np.array_equal(lut[0][:180], np.arange(180)) and np.array_equal(lut[1], np.arange(256)) and np.array_equal(lut[2], np.arange(256))
    lut = yolo2d.hsv_luts([1.01, 1.5, 0.5])
    assert lut.dtype == np.uint8 and lut[1][200] == 255 and lut[2][201] == 100 and lut[0][179] == int(179 * 1.01 % 180)


# The stated bound for the unit-gain round trip was 1 level, to be raised to what the sweep over all 256^3 colours shows.  It shows 4:
# a hue step of 2 degrees moves a channel of a saturated colour by up to 255 / 60 = 4.25 levels per degree, of which the rounding of H
# keeps at most one degree, and the 8-bit saturation and the final rounding add to it.  4 597 291 colours move a channel by more than 1.
HSV_ROUND_TRIP_BOUND = 4


def test_ref_hsv_round_trip_over_all_colours():
    """Unit gains: BGR -> HSV (hue in 0..179, 8-bit saturation) -> BGR over all 256^3 colours moves no channel by more than
    HSV_ROUND_TRIP_BOUND levels (the figure this sweep measured)"""
    lut = yolo2d.hsv_luts([1.0, 1.0, 1.0])
    worst, moved = 0, 0
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r in range(256):
        img = np.stack([np.full_like(g, r), g, b], -1)
        d = np.abs(YR.hsv(img, lut).astype(np.int16) - img.astype(np.int16))
        worst = max(worst, int(d.max()))
        moved += int((d.max(-1) > 1).sum())
    print(f"HSV round trip over 256^3 colours: largest channel move {worst} levels, {moved} colours move a channel by more than 1")
    assert worst <= HSV_ROUND_TRIP_BOUND
    grey = np.stack([np.arange(256, dtype=np.uint8)] * 3, -1)[None]
    assert np.array_equal(YR.hsv(grey, lut), grey)  # greys and the primaries survive exactly
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]], np.uint8)
    assert np.array_equal(YR.hsv(prim, lut), prim)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_out_of_scope_requests_raise(tmp_path):
    z = T.fixture()
    img_dir = T.write_tree(str(tmp_path), z["label_text"])
    with pytest.raises(y3d.Y3DError, match="rect"):
        yolo2d.Split(img_dir, T.IMGSZ, rect=True)
    for task in ("segment", "pose", "obb"):
        with pytest.raises(y3d.Y3DError, match="segments / keypoints / obb"):
            yolo2d.Split(img_dir, T.IMGSZ, task=task)
    sp = yolo2d.Split(img_dir, T.IMGSZ)
    for over, what in ((dict(copy_paste=0.1), "copy_paste"), (dict(perspective=0.0005), "perspective"), (dict(albumentations=True), "Albumentations"),
                       (dict(workers=4), "multi-worker"), (dict(mosaic_grid=9), "3 / 9"), (dict(mosaic_grid=3), "3 / 9")):
        with pytest.raises(y3d.Y3DError, match=what):
            yolo2d.sample_augment(sp, 0, yolo2d.data_args(**over))
        with pytest.raises(y3d.Y3DError, match=what):
            yolo2d.build_batch(sp, [0], yolo2d.data_args(**over), "cuda")
    assert sp.buffer == []  # refused before anything is loaded
    seg = tmp_path / "seg"
    (seg / "images").mkdir(parents=True)
    (seg / "labels").mkdir()
    from PIL import Image
    Image.fromarray(T.frame_pixels(0, 8, 8), "RGB").save(seg / "images" / "a.png")
    (seg / "labels" / "a.txt").write_text("0 0.1 0.1 0.5 0.1 0.5 0.5 0.1 0.5\n")
    with pytest.raises(y3d.Y3DError, match="segments / keypoints / obb"):
        yolo2d.Split(str(seg / "images"), T.IMGSZ)
    with pytest.raises(y3d.Y3DError, match="augment"):
        yolo2d.sample_augment(sp, 0, yolo2d.data_args(), "val")


def test_bad_capacity_and_host_device_raise(tmp_path):
    z = T.fixture()
    sp = yolo2d.Split(T.write_tree(str(tmp_path), z["label_text"]), T.IMGSZ)
    with pytest.raises(ValueError, match="max_boxes"):
        yolo2d.build_batch(sp, [0], yolo2d.data_args(), "cuda", max_boxes=100)
    with pytest.raises(ValueError, match="max_boxes"):
        yolo2d.encode_labels({}, T.IMGSZ, max_boxes=100)
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        yolo2d.build_batch(sp, [0], yolo2d.data_args(), "cpu")
    with pytest.raises(y3d.Y3DError, match="HIP device"):
        yolo2d.pack_labels(np.zeros((1, 5), np.float32), np.zeros((1, 20), np.int32), np.zeros((1, 48), np.float32), "cpu")
    with pytest.raises(y3d.Y3DError, match="multiple of 4"):
        yolo2d.Split(sp.im_files, 66)
