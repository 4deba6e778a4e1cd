"""GPU: the drawing kernels (csrc/draw3d.hip, plot.py) against the NumPy restatement of tests/draw_ref.py, bit for bit: every canvas a
slice along the batch axis of a larger sentinel-filled allocation whose guard images must stay untouched, uncovered pixels keeping
their prior bytes; the two prepare kernels' tables; `Predictor3d.annotate` and `draw_bev` end to end; one captured-and-replayed
`draw_boxes3d`.  tests/test_draw_ref_host.py shows that the case lists reach the situations they are there for."""
import functools

import numpy as np
import pytest
import torch

import draw_ref as DR
import predict3d_ref as PR

import yolov10_3d_amd as y3d
from yolov10_3d_amd import ops as P_ops
from yolov10_3d_amd import plot, predict

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANVASES = [(1, 1, 1), (2, 37, 53), (3, 64, 256)]
GUARD = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _start(B, H, W):
    """the prior bytes of a canvas: random, so that a stray store of any value shows"""
    return np.random.default_rng(B + H + W).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _guarded(start):
    """-> (the whole allocation, its inner slice): a guard image in front and behind"""
    B = start.shape[0]
    whole = torch.full((B + 2,) + start.shape[1:], GUARD, dtype=torch.uint8, device=DEV)
    whole[1:B + 1] = _dev(start)
    return whole, whole[1:B + 1]


def _check(whole, want, what):
    got = whole.cpu().numpy()
    assert (got[0] == GUARD).all() and (got[-1] == GUARD).all(), f"{what}: a guard image was written"
    bad = (got[1:-1] != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, the first at (b, y, x) = {tuple(np.argwhere(bad)[0])}"


def _nseg(B, S):
    return np.array([S // 2, 0, S + 3][:B], np.int32)  # below S, nothing, and above S (clamped)


# ---------------------------------------------------------------------------------------------------------------- draw_segments
@pytest.mark.parametrize("S", [0, 1, 257, 4200])
@pytest.mark.parametrize("shape", CANVASES, ids=str)
def test_draw_segments_equals_the_restatement(shape, S):
    B, H, W = shape
    segs, rgb, _ = DR.segment_cases(B, H, W, S)
    start = _start(B, H, W)
    d_segs, d_rgb = _dev(segs), _dev(rgb)
    n = _nseg(B, S)
    # (thickness, counts): every thickness, the counts given (garbage behind them: the other kinds, NaN among them) and NULL; the
    # 4200 segments (17 chunks of the kernel's list) meet all four on the two small canvases and two of the four on the largest, to
    # keep the restatement's time at a few seconds
    combos = ((1, None), (2, n), (5, n), (2.5, None))
    for t, counts in combos[1::2] if S > 1000 and H * W > 4000 else combos:
        whole, canvas = _guarded(start)
        out = plot.draw_segments(canvas, d_segs, d_rgb, None if counts is None else _dev(counts), thickness=t)
        assert out is canvas
        want = DR.paint_batch(DR.paint_segments, start, segs, rgb, counts, t=t)
        _check(whole, want, f"{shape}, S = {S}, t = {t}, counts {counts}")
        if S == 257 and H > 1:
            changed = (want != start).any(-1).mean()
            assert 0.02 < changed < 1.0, changed  # something was drawn, something was kept


@pytest.mark.parametrize("shape", CANVASES[1:], ids=str)
def test_the_lower_index_wins_a_stack_of_segments(shape):
    """257 segments over the same pixels, each in its own colour (two chunks of the kernel's list: the done bits carry over)"""
    B, H, W = shape
    segs, rgb, _ = DR.segment_cases(B, H, W, 257, stacked=True)
    start = _start(B, H, W)
    for t, counts in ((5, None), (2, np.array([257, 100, 1][:B], np.int32))):
        whole, canvas = _guarded(start)
        plot.draw_segments(canvas, _dev(segs), _dev(rgb), None if counts is None else _dev(counts), thickness=t)
        _check(whole, DR.paint_batch(DR.paint_segments, start, segs, rgb, counts, t=t), f"stack {shape}, t = {t}")
    # reversed order, the same pixels: now the former last one is on top
    whole, canvas = _guarded(start)
    plot.draw_segments(canvas, _dev(segs[:, ::-1]), _dev(rgb[:, ::-1]), thickness=5)
    got = whole.cpu().numpy()[1:-1]
    core = DR.segment_mask(H, W, [1.4, 1.4, W - 2.4, H - 2.4], 1)
    assert core.sum() > 30 and all((got[b][core] == rgb[b, -1, :3]).all() for b in range(B))


# ---------------------------------------------------------------------------------------------------------------- draw_quads
@pytest.mark.parametrize("Q", [0, 1, 300])
@pytest.mark.parametrize("shape", CANVASES, ids=str)
def test_draw_quads_equals_the_restatement(shape, Q):
    B, H, W = shape
    quads, rgb, _ = DR.quad_cases(B, H, W, Q)
    start = _start(B, H, W)
    for counts in (None, np.array([Q // 3, Q + 1, 0][:B], np.int32)):
        whole, canvas = _guarded(start)
        plot.draw_quads(canvas, _dev(quads), _dev(rgb), None if counts is None else _dev(counts))
        _check(whole, DR.paint_batch(DR.paint_quads, start, quads, rgb, counts), f"{shape}, Q = {Q}, counts {counts}")
    if Q:  # without the canvas-filling kinds something of the canvas is kept: both windings, edges, vertices, single pixels
        keep = DR.QUAD_KINDS.index("huge")
        q2 = quads.copy()
        q2[:, np.arange(Q) % len(DR.QUAD_KINDS) == keep] = np.nan
        whole, canvas = _guarded(start)
        plot.draw_quads(canvas, _dev(q2), _dev(rgb))
        want = DR.paint_batch(DR.paint_quads, start, q2, rgb)
        _check(whole, want, f"{shape}, Q = {Q}, no canvas-filling quads")
        if Q == 300 and H > 1:
            assert 0.05 < (want != start).any(-1).mean() < 1.0


# ---------------------------------------------------------------------------------------------------------------- the prepare kernels
def _same_table(got, want, what, one_ulp=None):
    """bit equality; NaN slots must be NaN in both (whatever their payload).  one_ulp: a mask of entries that may differ by one ulp."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype != np.float64:
        assert np.array_equal(got, want), what
        return 0
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN slots differ"
    diff = np.abs(got.view(np.int64) - want.view(np.int64))
    diff[nan] = 0
    if one_ulp is not None:
        loose = int((diff[one_ulp] != 0).sum())
        assert (diff[one_ulp] <= 1).all(), f"{what}: a clipped endpoint differs by {int(diff[one_ulp].max())} ulp"
        diff[one_ulp] = 0
    else:
        loose = 0
    assert not diff.any(), f"{what}: {int((diff != 0).sum())} values differ, the first at {tuple(np.argwhere(diff != 0)[0])}"
    return loose


def _fixture_boxes():
    """the reference's own boxes (tests/golden/predict3d.npz) with the rows' classes and the calibration of the fixture"""
    Z = PR.fixture()
    counts = Z["t001/counts"].astype(np.int32)
    return Z["t001/corners3d"].astype(np.float64), Z["t001/rows"].astype(np.float64), counts, Z["P2"].astype(np.float64).reshape(len(counts), 12)


@pytest.mark.parametrize("source", ["fixture", (1, 1), (2, 257), (3, 300)], ids=str)
def test_box_segments_and_bev_quads_equal_the_restatement(source):
    if source == "fixture":
        c3, rows, counts, P2 = _fixture_boxes()
        affine, nears = np.array([[0.5, 0.01, 3.0, -0.02, 0.25, 1.5]] * len(c3)), (0.1, 20.0)  # 20 m cuts through the fixture's boxes
    else:
        c3, rows, counts, P2, affine, near = DR.box_cases(*source)
        nears = (near,)
    B, K = c3.shape[:2]
    d = [_dev(a) for a in (c3, rows, counts, P2)]
    loose = total = 0
    for near in nears:
        for aff in (None, affine):
            for pal in (DR.PALETTE4, DR.PALETTE4[:1]):
                segs, rgb = plot.box3d_segments(*d, None if aff is None else _dev(aff), palette=pal, near=near)
                assert tuple(segs.shape) == (B, K * 14, 4) and tuple(rgb.shape) == (B, K * 14, 4)
                segs, rgb = segs.cpu().numpy(), rgb.cpu().numpy()
                for b in range(B):
                    ws, wc, clipped = DR.box_segments(c3[b], rows[b], counts[b], P2[b], None if aff is None else aff[b], pal, near)
                    # a clipped endpoint went through one more float64 division on each side: counted apart, and expected to be
                    # bit-equal as well (asserted below)
                    loose += _same_table(segs[b], ws, f"segs {source} image {b} near {near}", np.repeat(clipped, 2, 1))
                    _same_table(rgb[b], wc, f"seg_rgb {source} image {b}")
                    total += int(clipped.sum())
                    assert np.isnan(segs[b, counts[b] * 14:]).all() and not rgb[b, counts[b] * 14:].any()
    assert loose == 0, f"{loose} clipped endpoint values differ from the restatement in their last bit"
    if source != (1, 1):
        assert total > 0  # clipped endpoints were compared
    # rows = None: every box takes palette entry 0
    s0, r0 = plot.box3d_segments(d[0], None, d[2], d[3], palette=DR.PALETTE4, near=nears[0])
    for b in range(B):
        ws, wc, _ = DR.box_segments(c3[b], None, counts[b], P2[b], None, DR.PALETTE4, nears[0])
        _same_table(s0[b].cpu().numpy(), ws, "segs without rows")
        _same_table(r0[b].cpu().numpy(), wc, "seg_rgb without rows")
    for scale, cx, cy in ((10, 600, 600), (2.5, 15.0, 14.5)):
        quads, qrgb = plot.bev_quads(d[0], d[1], d[2], scale, cx, cy, palette=DR.PALETTE4)
        assert tuple(quads.shape) == (B, K, 4, 2) and tuple(qrgb.shape) == (B, K, 4)
        for b in range(B):
            wq, wc = DR.bev_quads(c3[b], rows[b], counts[b], DR.PALETTE4, scale, cx, cy)
            _same_table(quads[b].cpu().numpy(), wq, f"quads {source} image {b}")
            _same_table(qrgb[b].cpu().numpy(), wc, f"quad_rgb {source} image {b}")


def test_the_wrappers_refuse_on_the_device_too():
    canvas = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    segs, rgb = torch.zeros(1, 2, 4, dtype=torch.float64, device=DEV), torch.zeros(1, 2, 4, dtype=torch.uint8, device=DEV)
    for t in (0, -2, float("nan"), float("inf")):
        with pytest.raises(y3d.Y3DError, match="thickness"):
            plot.draw_segments(canvas, segs, rgb, thickness=t)
    with pytest.raises(y3d.Y3DError, match="contiguous"):
        plot.draw_segments(canvas[:, :, ::2], segs, rgb)
    with pytest.raises(y3d.Y3DError, match="float64"):
        plot.draw_segments(canvas, segs.float(), rgb)
    with pytest.raises(y3d.Y3DError, match="colours of shape"):
        plot.draw_segments(canvas, segs, rgb[:, :1])
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        plot.draw_segments(canvas, segs, canvas.reshape(-1)[8:16].reshape(1, 2, 4))
    assert not canvas.any()


# ---------------------------------------------------------------------------------------------------------------- BEV
@pytest.mark.parametrize("source", ["fixture", (3, 300)], ids=str)
def test_draw_bev_equals_the_restatement(source):
    if source == "fixture":
        c3, rows, counts, _ = _fixture_boxes()
    else:
        c3, rows, counts, _, _, _ = DR.box_cases(*source)
    B = len(c3)
    gt3 = [plot.corners3d_of(rows[b, : 2 + b] + np.array([0] * 9 + [1.5, 0, -2.0, 0.3, 0])) for b in range(B)]  # shifted copies of a few boxes
    g3, gn = plot.pack_boxes(gt3, DEV)
    args = (_dev(c3), _dev(rows), _dev(counts))
    kw = dict(max_dist=60, scale=10) if source == "fixture" else dict(max_dist=30, scale=4)  # 600 x 1200 and 120 x 240
    got = plot.draw_bev(*args, palette=DR.PALETTE4, **kw)
    R = kw["max_dist"] * kw["scale"]
    assert tuple(got.shape) == (B, R, 2 * R, 3) and got.dtype == torch.uint8
    want = DR.draw_bev(c3, rows, counts, DR.PALETTE4, **kw)
    assert np.array_equal(got.cpu().numpy(), want)
    bg = DR.bev_background(kw["max_dist"], kw["scale"])
    assert (want != bg[None]).any() and (want == bg[None]).all(-1).mean() > 0.3
    want_gt = DR.draw_bev(c3, rows, counts, DR.PALETTE4, gt=(g3.cpu().numpy(), gn.cpu().numpy()), **kw)
    for gt in ((g3, gn), gt3):  # device tensors, and the list of host arrays
        assert np.array_equal(plot.draw_bev(*args, gt=gt, palette=DR.PALETTE4, **kw).cpu().numpy(), want_gt)
    green = (want_gt == np.array([0, 255, 0], np.uint8)).all(-1)
    assert green.any() and (want_gt != want).any()
    # the cached background is not painted over
    assert np.array_equal(plot.draw_bev(*args, palette=DR.PALETTE4, **kw).cpu().numpy(), want)


def test_draw_bev_of_one_image_leaves_the_cached_background_alone():
    """B = 1, where expanding the cached map to the batch is no copy by itself: two calls with different boxes (and a ground-truth set
    in between) each start from the empty map, and the cached map is still the empty map afterwards"""
    c3, rows, counts, _ = _fixture_boxes()
    for kw in (dict(max_dist=60, scale=10), dict(max_dist=40, scale=5)):
        bg = DR.bev_background(**kw)
        for b in (1, 2, 1):
            one = (c3[b:b + 1], rows[b:b + 1], counts[b:b + 1])
            gt = None if b == 1 else [plot.corners3d_of(rows[0, :3])]
            out = plot.draw_bev(*(_dev(a) for a in one), gt=gt, palette=DR.PALETTE4, **kw)
            got = out.cpu().numpy()
            want = DR.draw_bev(*one, DR.PALETTE4, gt=None if gt is None else (np.stack(gt), [3]), **kw)
            assert got.shape == (1,) + bg.shape and np.array_equal(got, want) and (want[0] != bg).any(), (kw, b)
            cached = plot._BACKGROUNDS[(str(out.device), float(kw["max_dist"]), float(kw["scale"]))]  # the entry the call used
            assert cached.data_ptr() != out.data_ptr() and np.array_equal(cached.cpu().numpy(), bg), (kw, b)
        first = DR.draw_bev(c3[1:2], rows[1:2], counts[1:2], DR.PALETTE4, **kw)
        second = DR.draw_bev(c3[2:3], rows[2:3], counts[2:3], DR.PALETTE4, **kw)
        assert (first != second).any()  # boxes left behind by the first call would show in the second


# ---------------------------------------------------------------------------------------------------------------- graph replay
def test_draw_boxes3d_replays_under_capture():
    """recorded once, replayed with other boxes on another canvas content: equal to the eager call (default queue settings)"""
    c3a, rowsa, counts, P2, affine, near = DR.box_cases(3, 300)
    rng = np.random.default_rng(11)
    c3b, rowsb = c3a[:, ::-1].copy() + rng.normal(0, 0.3, (3, 300, 1, 3)), rowsa[:, ::-1].copy()
    H, W = 96, 320
    st_c3, st_rows, st_canvas = _dev(c3a).clone(), _dev(rowsa).clone(), torch.zeros(3, H, W, 3, dtype=torch.uint8, device=DEV)
    fixed = (_dev(np.array([300, 300, 300], np.int32)), _dev(P2), _dev(affine * 0.25))
    launch = lambda cv, c, r: plot.draw_boxes3d(cv, c, r, *fixed, palette=DR.PALETTE4, thickness=2, near=near)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture (uploads the palette)
        launch(st_canvas, st_c3, st_rows)
    torch.cuda.current_stream().wait_stream(s)
    first = st_canvas.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(st_canvas, st_c3, st_rows)
    second_start = _dev(_start(3, H, W))
    st_canvas.copy_(second_start)
    st_c3.copy_(_dev(c3b))
    st_rows.copy_(_dev(rowsb))
    graph.replay()
    torch.cuda.synchronize()
    want = launch(second_start.clone(), _dev(c3b), _dev(rowsb))
    assert torch.equal(st_canvas, want)
    assert not torch.equal(want, second_start) and first.any() and not torch.equal(first != 0, (want != second_start))
    graph.reset()


# ---------------------------------------------------------------------------------------------------------------- end to end
RES = (320, 256)


@pytest.fixture(autouse=True)
def _restore_compute_dtype():
    before = P_ops.compute_dtype()
    yield
    y3d.set_compute_dtype(before)


@pytest.fixture(scope="module")
def model():
    """the seeded yolov10n_3D of tests/test_hip_predict3d.py: BatchNorm statistics of a random batch, wider score projections"""
    before = P_ops.compute_dtype()
    y3d.set_compute_dtype(torch.float32)
    cfg = y3d.yaml_model_load("yolov10n_3D.yaml")
    torch.manual_seed(3)
    m = y3d.YOLOv10_3DDetectionModel(cfg).to(DEV)
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


def test_annotate_equals_the_hand_chained_wrappers(model):
    y3d.set_compute_dtype(torch.float32)
    rng = np.random.default_rng(4)
    shapes = [(375, 1242), (370, 1224), (375, 1242)]  # two shapes: two groups, the first of two images that are not neighbours
    rgb = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    P2s = list(PR.synth_camera(3)[1])
    pr = predict.Predictor3d(model, conf=-1.0, resolution=RES)  # every row is kept: 50 boxes per image
    rows, c3, ci, counts = pr(rgb, P2s, static=True)
    assert counts.tolist() == [50, 50, 50]
    keep = [a.copy() for a in rgb]
    got = pr.annotate(rgb, P2s)
    assert all(np.array_equal(a, b) for a, b in zip(rgb, keep))  # the caller's images are left alone
    P = _dev(np.stack(P2s).astype(np.float64))
    drawn = 0
    for b in range(3):
        canvas = _dev(rgb[b][None])
        segs, srgb = plot.box3d_segments(c3[b:b + 1], rows[b:b + 1], counts[b:b + 1], P[b:b + 1])
        plot.draw_segments(canvas, segs, srgb, thickness=2)
        assert got[b].dtype == np.uint8 and got[b].shape == rgb[b].shape and np.array_equal(got[b], canvas[0].cpu().numpy()), b
        # and the restatement, from the same tables
        assert np.array_equal(got[b], DR.paint_segments(rgb[b], segs[0].cpu().numpy(), srgb[0].cpu().numpy(), 2)), b
        drawn += int((got[b] != rgb[b]).any(-1).sum())
    assert drawn > 0
    # the results handed in, in both forms, device images, another thickness, and the BEV maps
    lst = pr(rgb, P2s)
    dev_imgs = [_dev(a) for a in rgb]
    thick, bev = pr.annotate(dev_imgs, P2s, results=lst, bev=True, thickness=5)
    again = pr.annotate(rgb, P2s, results=(rows, c3, ci, counts), thickness=5)
    assert all(np.array_equal(a, b) for a, b in zip(thick, again)) and any(not np.array_equal(a, b) for a, b in zip(thick, got))
    assert all(torch.equal(d, _dev(a)) for d, a in zip(dev_imgs, rgb))
    assert bev.shape == (3, 600, 1200, 3) and np.array_equal(bev, plot.draw_bev(c3, rows, counts).cpu().numpy())
    assert np.array_equal(bev, DR.draw_bev(c3.cpu().numpy(), rows.cpu().numpy(), counts.cpu().numpy(), plot.PALETTE))
