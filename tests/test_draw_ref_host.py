"""CPU: the NumPy restatement of the drawing rules (tests/draw_ref.py) checked on its own, the case lists of tests/test_hip_draw.py shown
to reach the situations they are there for, `plot.corners3d_of` against the reference's corners, and the refusals of the wrappers and
of the entry points (every check of an entry point comes before its launch, so none of this needs a device)."""
import numpy as np
import pytest
import torch

import draw_ref as DR
import predict3d_ref as PR

import yolov10_3d_amd as y3d
from yolov10_3d_amd import plot


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_a_segment_leaves_no_gap():
    """thickness >= 1: every column between the endpoints of a flat segment (every row, of a steep one) holds a covered pixel"""
    rng = np.random.default_rng(5)
    H, W = 40, 56
    for i in range(300):
        t = (1, 1.5, 2, 5)[i % 4]
        ax, bx = rng.uniform(0, W - 1, 2)
        ay, by = rng.uniform(0, H - 1, 2)
        m = DR.segment_mask(H, W, [ax, ay, bx, by], t)
        if abs(bx - ax) >= abs(by - ay):
            lo, hi = int(np.ceil(min(ax, bx))), int(np.floor(max(ax, bx)))
            assert m[:, lo:hi + 1].any(0).all(), (i, ax, ay, bx, by, t)
        else:
            lo, hi = int(np.ceil(min(ay, by))), int(np.floor(max(ay, by)))
            assert m[lo:hi + 1].any(1).all(), (i, ax, ay, bx, by, t)
        assert m.sum() <= (np.hypot(bx - ax, by - ay) + t + 2) * (t + 2)  # and it is a stroke, not a blob


def test_the_bound_is_inclusive_to_the_ulp():
    up = lambda v: np.nextafter(v, np.inf)
    # the body: the pixel centres of row 3 lie at exactly t/2 = 0.5 below the segment
    assert DR.segment_mask(8, 12, [2, 3.5, 8, 3.5], 1)[3, 5] and DR.segment_mask(8, 12, [2, 3.5, 8, 3.5], 1)[4, 5]
    m = DR.segment_mask(8, 12, [2, up(3.5), 8, up(3.5)], 1)
    assert not m[3, 5] and m[4, 5]
    # the caps: pixel (2, 3) at exactly 0.5 before a, pixel (9, 3) at exactly 0.5 behind b
    m = DR.segment_mask(8, 12, [2.5, 3, 8.5, 3], 1)
    assert m[3, 2] and m[3, 9] and not m[3, 1] and not m[3, 10]
    m = DR.segment_mask(8, 12, [up(2.5), 3, np.nextafter(8.5, -np.inf), 3], 1)
    assert not m[3, 2] and not m[3, 9] and m[3, 3] and m[3, 8]
    # thickness 5 on a half-integer line: rows at distance 2.5 are in, and a point is a disc with its rim
    m = DR.segment_mask(12, 12, [2, 5.5, 8, 5.5], 5)
    assert m[3, 5] and m[8, 5] and not m[2, 5] and not m[9, 5]
    d = DR.segment_mask(12, 12, [5, 5, 5, 5], 6)
    assert d[5, 8] and d[2, 5] and not d[5, 9] and d.sum() == 29  # the lattice points within 3 of a lattice point
    # a quad: centres on an edge and on a vertex are covered
    q = DR.quad_mask(8, 8, [[2, 2], [5, 2], [5, 4], [2, 4]])
    assert q[2, 2] and q[4, 5] and q[2, 3] and not q[1, 3] and not q[3, 6] and q.sum() == 12


def test_both_windings_give_the_same_mask():
    quads, _, kinds = DR.quad_cases(2, 37, 53, 300)
    n = 0
    for q in quads.reshape(-1, 4, 2):
        if np.isfinite(q).all():
            a, b = DR.quad_mask(37, 53, q), DR.quad_mask(37, 53, q[::-1])
            assert np.array_equal(a, b)
            n += int(a.any())
    assert n > 100


def test_the_lower_index_wins_and_windows_change_nothing():
    segs, rgb, _ = DR.segment_cases(1, 37, 53, 257, stacked=True)
    base = np.full((37, 53, 3), 9, np.uint8)
    out = DR.paint_segments(base, segs[0], rgb[0], 5)  # 2.5 > the core's 0.5 + the jitter's 0.57
    core = DR.segment_mask(37, 53, [1.4, 1.4, 50.6, 34.6], 1)  # inside every jittered copy
    assert core.sum() > 30 and (out[core] == rgb[0, 0, :3]).all()
    assert len({tuple(c) for c in rgb[0, :, :3]}) == 257
    assert np.array_equal(DR.paint_segments(base, segs[0], rgb[0], 5, n=100)[core], out[core])
    later = DR.paint_segments(base, segs[0, 1:], rgb[0, 1:], 5)
    assert (later[core] == rgb[0, 1, :3]).all()
    q = np.array([[[2, 2], [30, 2], [30, 20], [2, 20]], [[10, 10], [40, 10], [40, 30], [10, 30]]], np.float64)
    c = np.array([[1, 2, 3, 0], [4, 5, 6, 0]], np.uint8)
    out = DR.paint_quads(base, q, c)
    assert tuple(out[15, 20]) == (1, 2, 3) and tuple(out[25, 35]) == (4, 5, 6) and tuple(out[0, 0]) == (9, 9, 9)
    # the windowed painters equal the full-canvas ones
    for (B, H, W, S) in ((2, 37, 53, 257), (1, 1, 1, 257)):
        segs, rgb, _ = DR.segment_cases(B, H, W, S)
        start = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
        for t in (1, 2.5, 5):
            assert np.array_equal(DR.paint_segments(start, segs[0], rgb[0], t), DR.paint_segments(start, segs[0], rgb[0], t, windowed=False))
        quads, qrgb, _ = DR.quad_cases(B, H, W, 300)
        assert np.array_equal(DR.paint_quads(start, quads[0], qrgb[0]), DR.paint_quads(start, quads[0], qrgb[0], windowed=False))


# ---------------------------------------------------------------------------------------------------------------- the case lists
def test_the_segment_cases_reach_their_situations():
    H, W = 37, 53
    segs, rgb, kinds = DR.segment_cases(2, H, W, 257)
    kind = lambda name: segs[0][kinds == DR.SEGMENT_KINDS.index(name)]
    assert all((kinds == i).sum() >= 25 for i in range(len(DR.SEGMENT_KINDS)))
    assert (kind("horizontal")[:, 1] == kind("horizontal")[:, 3]).all() and (kind("vertical")[:, 0] == kind("vertical")[:, 2]).all()
    d = kind("diagonal")
    assert (d[:, 2] - d[:, 0] == d[:, 3] - d[:, 1]).all()
    s = kind("steep")
    assert (np.abs(s[:, 3] - s[:, 1]) > 5 * np.abs(s[:, 2] - s[:, 0])).all()
    assert (kind("point")[:, :2] == kind("point")[:, 2:]).all()
    assert not any(DR.segment_mask(H, W, s, 5).any() for s in kind("outside"))
    c = kind("crossing")
    assert (np.abs(c[:, [0, 2]]) == 1e9).all() and all(DR.segment_mask(H, W, s, 1).sum() >= W for s in c if 2 <= s[1] <= H - 3 and s[1] == s[3])
    assert any(DR.segment_mask(H, W, s, 1).any() for s in c if s[1] != s[3])
    bad = kind("nonfinite")
    assert (~np.isfinite(bad)).sum(1).tolist() == [1] * len(bad) and (~np.isfinite(bad)).any(0).all()
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    # the half-integer lines: with t = 1 some pixel lies on the bound itself (c c == r2 len2), on both sides
    hits = 0
    for s in kind("half"):
        m = DR.segment_mask(H, W, s, 1)
        y, x = int(s[1] - 0.5), int(s[0] + 0.5)
        if 0 <= y < H - 1 and 0 <= x < W and s[2] > s[0] + 1:
            assert m[y, x] and m[y + 1, x]
            hits += 1
    assert hits >= 5
    # a painted canvas changes, but not everywhere; the 1 x 1 canvas is hit by some and missed by some
    start = np.zeros((H, W, 3), np.uint8)
    frac = (DR.paint_segments(start, segs[0], rgb[0], 1) != start).any(2).mean()
    assert 0.05 < frac < 1.0
    one, orgb, _ = DR.segment_cases(1, 1, 1, 257)
    m = [DR.segment_mask(1, 1, s, 1)[0, 0] for s in one[0]]
    assert any(m) and not all(m)


def test_the_quad_cases_reach_their_situations():
    H, W = 37, 53
    quads, rgb, kinds = DR.quad_cases(2, H, W, 300)
    kind = lambda name: quads[0][kinds == DR.QUAD_KINDS.index(name)]
    assert all(DR.quad_area2(q) > 0 for q in kind("ccw")) and all(DR.quad_area2(q) < 0 for q in kind("cw"))
    assert all(DR.quad_area2(q) == 0 and not DR.quad_mask(H, W, q).any() for q in kind("flat"))
    e = kind("edge")[0]
    assert e[0, 0] == int(e[0, 0]) and DR.quad_mask(H + 80, W + 80, e)[int(e[0, 1]), int(e[0, 0])]  # the vertex pixel itself
    assert any(DR.quad_mask(H, W, q).any() for q in kind("vertex"))
    assert all(DR.quad_mask(H, W, q).all() for q in kind("huge"))
    tiny = [int(DR.quad_mask(H, W, q).sum()) for q in kind("tiny")]
    assert set(tiny) == {0, 1}
    bad = kind("nonfinite")
    assert all(not np.isfinite(q).all() for q in bad)


def test_the_box_cases_reach_their_situations():
    for B, K in ((1, 1), (2, 257), (3, 300)):
        c3, rows, counts, P2, affine, near = DR.box_cases(B, K)
        assert c3.shape == (B, K, 8, 3) and counts[0] == K and (B < 2 or counts[1] == 0)
        segs, rgb, clipped = DR.box_segments(c3[0], rows[0], counts[0], P2[0], None, DR.PALETTE4, near)
        W = c3[0, :, :, 2]  # P2's third row is (0, 0, 1, 0)
        assert (W[0] == near).sum() == 4 and np.isfinite(segs[:14]).all() and not clipped[:14].any()  # W == near is kept, unclipped
        if K > 1:
            dropped = np.isnan(segs).all(1)
            assert clipped.any() and dropped.any() and (~dropped & ~clipped.any(1)).any() and not (clipped[:, 0] & clipped[:, 1]).any()
            assert np.isfinite(segs[clipped.any(1)]).all()
            cls = rows[0, :, 0]
            assert np.isnan(cls).any() and (cls > 3).any() and (cls < 0).any()
            col = rgb.reshape(K, 14, 4)[:, 0]
            assert (col[np.isnan(cls)] == DR.colours([0], DR.PALETTE4)[0]).all() and (col[cls > 3] == DR.colours([3], DR.PALETTE4)[0]).all()
            assert (col[cls == 2.9] == DR.colours([2], DR.PALETTE4)[0]).all() and (col[cls < 0] == DR.colours([0], DR.PALETTE4)[0]).all()
        if B > 1:
            s1, r1, _ = DR.box_segments(c3[1], rows[1], counts[1], P2[1], affine[1], DR.PALETTE4, near)
            assert np.isnan(s1).all() and not r1.any()
    # a segment by hand: endpoints (0, 0, 2) and (0, 0, -2) with P2 = [I | 0], near 1: clipped at s = 3/4 of the way from the far end
    c = np.zeros((1, 8, 3))
    c[0, :, 2] = [2, -2, 2, 2, 2, 2, 2, 2]
    c[0, 0, 0], c[0, 1, 0] = 4.0, -4.0
    segs, _, clipped = DR.box_segments(c, None, 1, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], None, DR.PALETTE4, 1.0)
    assert clipped[0].tolist() == [False, True] and segs[0].tolist() == [2.0, 0.0, 2.0, 0.0]  # (4 - 0.25 * 8) / (-2 + 0.25 * 4)
    quads, qrgb = DR.bev_quads(c, None, 1, DR.PALETTE4, 10, 600, 600)
    assert quads[0, 0].tolist() == [640.0, 580.0] and quads[0, 1].tolist() == [560.0, 620.0] and tuple(qrgb[0]) == (250, 10, 20, 0)


def test_the_bev_background():
    bg = DR.bev_background(60, 10)
    assert bg.shape == (600, 1200, 3) and np.array_equal(bg, plot.bev_background(60, 10))
    on = bg[..., 0] == 255
    assert set(np.unique(bg)) == {0, 255} and 0.01 < on.mean() < 0.1
    assert on[599, 100] and on[300, 600] and on[0, 600] and on[599, 1]  # the horizontal ray, the vertical ray, the outer ring
    assert on[599 - 149, 600] and not on[599 - 140, 590]  # the first ring on the axis; nothing between ring and rays
    small = DR.bev_background(6, 2.5)
    assert small.shape == (15, 30, 3) and np.array_equal(small, plot.bev_background(6, 2.5))
    with pytest.raises(y3d.Y3DError, match="whole number"):
        plot.bev_background(6, 0.3)


# ---------------------------------------------------------------------------------------------------------------- corners3d_of
def test_corners3d_of_equals_the_references_corners():
    Z = PR.fixture()
    n = 0
    for tag in ("t001", "t25"):
        for b, cnt in enumerate(Z[f"{tag}/counts"]):
            rows = Z[f"{tag}/rows"][b, :cnt]
            got = plot.corners3d_of(rows)
            assert got.dtype == np.float64 and got.shape == (cnt, 8, 3)
            # the bound of tests/test_predict3d_host.py: the rows are the reference's own, so only the order of a few float64 sums differs
            np.testing.assert_allclose(got, PR.corners(rows, Z["P2"][b])[0], rtol=0, atol=1e-9)
            np.testing.assert_allclose(got, Z[f"{tag}/corners3d"][b, :cnt], rtol=0, atol=1e-9)
            n += int(cnt)
            anno = {"dimensions": rows[:, [8, 6, 7]], "location": rows[:, 9:12], "rotation_y": rows[:, 12]}
            assert np.array_equal(plot.corners3d_of(anno), got)
    assert n > 20 and plot.corners3d_of(np.zeros((0, 14))).shape == (0, 8, 3)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_the_wrappers_refuse_host_tensors():
    c3, rows, counts = torch.zeros(1, 2, 8, 3, dtype=torch.float64), torch.zeros(1, 2, 14, dtype=torch.float64), torch.ones(1, dtype=torch.int32)
    P2 = torch.zeros(1, 3, 4, dtype=torch.float64)
    canvas = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    segs, srgb = torch.zeros(1, 28, 4, dtype=torch.float64), torch.zeros(1, 28, 4, dtype=torch.uint8)
    quads, qrgb = torch.zeros(1, 2, 4, 2, dtype=torch.float64), torch.zeros(1, 2, 4, dtype=torch.uint8)
    for call in (lambda: plot.box3d_segments(c3, rows, counts, P2), lambda: plot.bev_quads(c3, rows, counts, 10, 600, 600),
                 lambda: plot.draw_segments(canvas, segs, srgb), lambda: plot.draw_quads(canvas, quads, qrgb),
                 lambda: plot.draw_boxes3d(canvas, c3, rows, counts, P2), lambda: plot.draw_bev(c3, rows, counts),
                 lambda: plot.draw_segments(canvas.numpy(), segs, srgb), lambda: plot.box3d_segments(c3.numpy(), rows, counts, P2)):
        with pytest.raises(y3d.Y3DError, match="HIP device"):
            call()


def test_the_entry_points_refuse_bad_arguments():
    """the checks of the C entries, reached with made-up addresses: every one of them fails before anything is launched or read.
    NOTE for whoever edits the entries: this test stays safe only while every check, and the early return for K / S / Q = 0, comes
    BEFORE the launch (as in tests/test_predict3d_host.py); with a check dropped or moved behind the launch, a machine with a GPU would
    run a kernel on these addresses.  Keep the order, and keep the sizes here small."""
    L = y3d.lib()
    cv, a, b, c, d, e, f, g = (0x10000000 + 0x1000000 * i for i in range(8))  # 16 MB apart, 16-byte aligned
    seg = lambda **k: L.draw_segments(*[{**dict(canvas=cv, B=2, H=30, W=40, segs=a, rgb=b, n=None, S=5, t=2.0, stream=None), **k}[x]
                                        for x in ("canvas", "B", "H", "W", "segs", "rgb", "n", "S", "t", "stream")])
    quad = lambda **k: L.draw_quads(*[{**dict(canvas=cv, B=2, H=30, W=40, quads=a, rgb=b, n=None, Q=5, stream=None), **k}[x]
                                      for x in ("canvas", "B", "H", "W", "quads", "rgb", "n", "Q", "stream")])
    box = lambda **k: L.box3d_segments(*[{**dict(c3=a, rows=b, counts=c, B=2, K=5, P2=d, aff=None, pal=e, n_pal=3, near=0.1, segs=f, rgb=g,
                                                 stream=None), **k}[x]
                                         for x in ("c3", "rows", "counts", "B", "K", "P2", "aff", "pal", "n_pal", "near", "segs", "rgb", "stream")])
    bev = lambda **k: L.box3d_bev_quads(*[{**dict(c3=a, rows=b, counts=c, B=2, K=5, pal=e, n_pal=3, scale=10.0, cx=600.0, cy=600.0, quads=f,
                                                  rgb=g, stream=None), **k}[x]
                                          for x in ("c3", "rows", "counts", "B", "K", "pal", "n_pal", "scale", "cx", "cy", "quads", "rgb", "stream")])
    for t in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(y3d.Y3DError, match="thickness"):
            seg(t=t)
    for fn in (seg, quad):
        for bad in (dict(B=0), dict(H=0), dict(W=0), dict(B=-1), dict(H=-3), dict(W=-1)):
            with pytest.raises(y3d.Y3DError, match="bad sizes"):
                fn(**bad)
        with pytest.raises(y3d.Y3DError, match="null canvas"):
            fn(canvas=None)
    with pytest.raises(y3d.Y3DError, match="bad sizes"):
        seg(S=-1)
    with pytest.raises(y3d.Y3DError, match="bad sizes"):
        quad(Q=-1)
    for fn in (box, bev):
        for bad in (dict(B=0), dict(K=-1), dict(n_pal=0), dict(n_pal=-2)):
            with pytest.raises(y3d.Y3DError, match="bad sizes"):
                fn(**bad)
        with pytest.raises(y3d.Y3DError, match="null argument"):
            fn(counts=None)
        with pytest.raises(y3d.Y3DError, match="overlaps an input"):
            fn(rgb=c)  # the colours over the counts
        with pytest.raises(y3d.Y3DError, match="overlap each other"):
            fn(rgb=f + 16)
    with pytest.raises(y3d.Y3DError, match="overlaps an input"):
        box(segs=a + 2 * 5 * 192 - 16)  # the last 16 bytes of corners3d: byte ranges, not base addresses
    box(segs=a + 2 * 5 * 192, K=0), seg(S=0), quad(Q=0), bev(K=0)  # nothing to do is no error (and nothing is launched)
    # a canvas over an input, at an offset inside it
    n_canvas = 2 * 30 * 40 * 3
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        seg(segs=cv + n_canvas - 16)
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        seg(rgb=cv - 5 * 2 * 4 + 4)
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        seg(n=cv + 16)
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        quad(quads=cv - 2 * 5 * 64 + 16)
    with pytest.raises(y3d.Y3DError, match="canvas overlaps"):
        quad(n=cv + n_canvas - 4)
    with pytest.raises(y3d.Y3DError, match="aligned"):
        seg(segs=a + 8)
