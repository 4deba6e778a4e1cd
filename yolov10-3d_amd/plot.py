"""Draw 3D predictions on the device: box wireframes over the camera image and a bird's-eye-view (BEV) map — the two pictures of the
reference's `KITTIVisualizer.plot_preds` / `plot_bev` (utils/plotting.py:1280-1411), made from what `predict.Predictor3d` leaves in
device memory (`rows`, `corners3d`, `counts`) by the kernels of csrc/draw3d.hip.

    dets = predictor(images, P2s, static=True)                       # rows, corners3d, corners_img, counts
    plot.draw_boxes3d(canvas, dets[1], dets[0], dets[3], P2)         # (B, H, W, 3) uint8 on the device, painted in place
    bev = plot.draw_bev(dets[1], dets[0], dets[3])                   # (B, 600, 1200, 3) uint8
    pictures = predictor.annotate(images, P2s)                       # one annotated (h, w, 3) uint8 numpy array per image

The coverage rules are exact and restatable (include/y3d.h; tests/draw_ref.py restates them in NumPy): float64, pixel
(x, y) is the point (x, y), a segment of thickness t covers the pixels within t/2 of it (bounds included), a quad the pixels on one side
of all its edges, and the primitive with the lower index wins a pixel, so row 0 (the highest score) ends up on top.  They are not
OpenCV's anti-aliased strokes.  No text labels, no legends, no matplotlib grids and no files: fonts and image encoders are out of scope.

Every wrapper takes device tensors only (there is no host fallback) and launches without allocating more than its outputs or waiting
for the device, so a call whose arguments are device tensors already can be captured into a graph.  One condition: a palette given as
tuples (the default) and `draw_bev`'s background are built on the host and uploaded on their first use per device, which a capture
cannot hold, so pass a uint8 device palette, or make the same call once before capturing."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import Y3DError, lib

# RGB: class 0, 1, 2 (KITTI: Pedestrian, Car, Cyclist), then spares for wider class lists
PALETTE = ((255, 64, 64), (64, 160, 255), (255, 200, 0), (200, 80, 255), (0, 220, 200), (255, 128, 0))
GT_COLOUR = ((0, 255, 0),)

_PALETTES = {}
_BACKGROUNDS = {}


def _dev_tensor(t, dtype, what):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype:
        raise Y3DError(f"plot: {what} must be a {str(dtype).replace('torch.', '')} tensor on a HIP device (no host fallback)")
    return t.contiguous()


def _palette(palette, dev):
    """(n_pal, 3) uint8 on the device; a palette given as nested tuples is uploaded once per device"""
    if torch.is_tensor(palette):
        p = _dev_tensor(palette, torch.uint8, "palette")
        if p.dim() != 2 or p.shape[1] != 3 or not p.shape[0]:
            raise Y3DError(f"plot: palette of shape {tuple(p.shape)}, expected (n, 3) with n >= 1")
        return p
    key = (str(dev), tuple(tuple(int(v) for v in c) for c in palette))
    if not key[1] or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in key[1]):
        raise Y3DError("plot: a palette is a non-empty list of (r, g, b) triples in 0 .. 255")
    if key not in _PALETTES:
        _PALETTES[key] = torch.tensor(key[1], dtype=torch.uint8).reshape(-1, 3).to(dev)
    return _PALETTES[key]


def _boxes(corners3d, rows, counts, what):
    c3 = _dev_tensor(corners3d, torch.float64, f"{what}: corners3d")
    if c3.dim() != 4 or tuple(c3.shape[2:]) != (8, 3) or c3.shape[0] < 1:
        raise Y3DError(f"{what}: corners3d of shape {tuple(c3.shape)}, expected (B, K, 8, 3)")
    B, K = int(c3.shape[0]), int(c3.shape[1])
    if rows is not None:
        rows = _dev_tensor(rows, torch.float64, f"{what}: rows")
        if tuple(rows.shape) != (B, K, 14):
            raise Y3DError(f"{what}: rows of shape {tuple(rows.shape)}, expected {(B, K, 14)}")
    counts = _dev_tensor(counts, torch.int32, f"{what}: counts")
    if tuple(counts.shape) != (B,):
        raise Y3DError(f"{what}: counts of shape {tuple(counts.shape)}, expected {(B,)}")
    return c3, rows, counts, B, K


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def box3d_segments(corners3d, rows, counts, P2, affine=None, palette=PALETTE, near=0.1):
    """`y3d_box3d_segments`: corners3d (B, K, 8, 3), rows (B, K, 14) float64 (or None: every box takes palette entry 0), counts (B,)
    int32, P2 (B, 3, 4) float64, affine (B, 2, 3) float64 or None -> segs (B, K * 14, 4) float64 [ax, ay, bx, by], seg_rgb
    (B, K * 14, 4) uint8 [r, g, b, 0]; dropped segments and the slots behind counts are NaN"""
    c3, rows, counts, B, K = _boxes(corners3d, rows, counts, "box3d_segments")
    P = _dev_tensor(P2, torch.float64, "box3d_segments: P2")
    if P.numel() != B * 12:
        raise Y3DError(f"box3d_segments: {B} images but P2 of shape {tuple(P.shape)} (one 3 x 4 matrix each)")
    if affine is not None:
        affine = _dev_tensor(affine, torch.float64, "box3d_segments: affine")
        if affine.numel() != B * 6:
            raise Y3DError(f"box3d_segments: {B} images but affine of shape {tuple(affine.shape)} (one 2 x 3 matrix each)")
    pal = _palette(palette, c3.device)
    segs = torch.empty(B, K * 14, 4, dtype=torch.float64, device=c3.device)
    rgb = torch.empty(B, K * 14, 4, dtype=torch.uint8, device=c3.device)
    lib().box3d_segments(_ptr(c3), _ptr(rows), counts.data_ptr(), B, K, P.data_ptr(), _ptr(affine), pal.data_ptr(), pal.shape[0],
                         float(near), _ptr(segs), _ptr(rgb), ops.stream())
    return segs, rgb


def bev_quads(corners3d, rows, counts, scale, cx, cy, palette=PALETTE):
    """`y3d_box3d_bev_quads`: the bottom faces as (cx + scale x, cy - scale z) -> quads (B, K, 4, 2) float64, quad_rgb (B, K, 4) uint8"""
    c3, rows, counts, B, K = _boxes(corners3d, rows, counts, "bev_quads")
    pal = _palette(palette, c3.device)
    quads = torch.empty(B, K, 4, 2, dtype=torch.float64, device=c3.device)
    rgb = torch.empty(B, K, 4, dtype=torch.uint8, device=c3.device)
    lib().box3d_bev_quads(_ptr(c3), _ptr(rows), counts.data_ptr(), B, K, pal.data_ptr(), pal.shape[0], float(scale), float(cx), float(cy),
                          _ptr(quads), _ptr(rgb), ops.stream())
    return quads, rgb


def _canvas(canvas, what):
    if not torch.is_tensor(canvas) or not canvas.is_cuda or canvas.dtype != torch.uint8:
        raise Y3DError(f"{what}: the canvas must be a uint8 tensor on a HIP device (no host fallback)")
    if canvas.dim() != 4 or canvas.shape[3] != 3 or not canvas.is_contiguous() or not canvas.numel():
        raise Y3DError(f"{what}: the canvas must be a contiguous, non-empty (B, H, W, 3) tensor, got {tuple(canvas.shape)}")
    return tuple(int(v) for v in canvas.shape[:3])


def _primitives(prims, rgb, n, B, shape, what):
    prims = _dev_tensor(prims, torch.float64, f"{what}: the primitives")
    if prims.dim() != 2 + len(shape) or prims.shape[0] != B or tuple(prims.shape[2:]) != shape:
        raise Y3DError(f"{what}: primitives of shape {tuple(prims.shape)}, expected {(B, 'n') + shape}")
    N = int(prims.shape[1])
    rgb = _dev_tensor(rgb, torch.uint8, f"{what}: the colours")
    if tuple(rgb.shape) != (B, N, 4):
        raise Y3DError(f"{what}: colours of shape {tuple(rgb.shape)}, expected {(B, N, 4)}")
    if n is not None:
        n = _dev_tensor(n, torch.int32, f"{what}: the counts")
        if tuple(n.shape) != (B,):
            raise Y3DError(f"{what}: counts of shape {tuple(n.shape)}, expected {(B,)}")
    return prims, rgb, n, N


def draw_segments(canvas, segs, rgb, nseg=None, thickness=2):
    """`y3d_draw_segments`: paints segs (B, S, 4) float64 with colours rgb (B, S, 4) uint8 into canvas (B, H, W, 3) uint8 in place (image
    b its first nseg[b] segments; all with nseg None) and returns the canvas"""
    B, H, W = _canvas(canvas, "draw_segments")
    segs, rgb, nseg, S = _primitives(segs, rgb, nseg, B, (4,), "draw_segments")
    lib().draw_segments(canvas.data_ptr(), B, H, W, _ptr(segs), _ptr(rgb), _ptr(nseg), S, float(thickness), ops.stream())
    return canvas


def draw_quads(canvas, quads, rgb, nquad=None):
    """`y3d_draw_quads`: fills the convex quads (B, Q, 4, 2) float64 with colours rgb (B, Q, 4) uint8 into the canvas in place"""
    B, H, W = _canvas(canvas, "draw_quads")
    quads, rgb, nquad, Q = _primitives(quads, rgb, nquad, B, (4, 2), "draw_quads")
    lib().draw_quads(canvas.data_ptr(), B, H, W, _ptr(quads), _ptr(rgb), _ptr(nquad), Q, ops.stream())
    return canvas


def draw_boxes3d(canvas, corners3d, rows, counts, P2, affine=None, palette=PALETTE, thickness=2, near=0.1):
    """the wireframes of the boxes over canvas (B, H, W, 3) uint8, in place: `box3d_segments`, then `draw_segments`.  P2 projects into
    the original image; for a canvas in another frame (the network-resolution batch) pass the 2 x 3 `affine` that leads there."""
    segs, rgb = box3d_segments(corners3d, rows, counts, P2, affine, palette, near)
    return draw_segments(canvas, segs, rgb, None, thickness)


# ------------------------------------------------------------------------------------------------------------------------------
# BEV
# ------------------------------------------------------------------------------------------------------------------------------
def _bev_radius(max_dist, scale):
    R = max_dist * scale
    if R != int(R) or R < 1:
        raise Y3DError(f"draw_bev: max_dist * scale = {R} must be a positive whole number of pixels")
    return int(R)


def bev_background(max_dist=60, scale=10):
    """the empty map of plot_bev (utils/plotting.py:1348-1365) as (R, 2R, 3) uint8 numpy, R = max_dist * scale, the ego at (R, R) just
    below the bottom edge: seven white rays at 0, 30 .. 180 degrees from (int(R - R cos), int(R - R sin)) to the ego, by the segment
    rule with thickness 2, and four range rings of radius int(R / 4 .. R), a ring covering p when (rad - 1)^2 <= |p - c|^2 <= (rad + 1)^2.
    Host NumPy float64, built once per (max_dist, scale) by `draw_bev`."""
    R = _bev_radius(max_dist, scale)
    x, y = np.meshgrid(np.arange(2 * R, dtype=np.float64), np.arange(R, dtype=np.float64))
    on = np.zeros((R, 2 * R), bool)
    c = float(R)
    for theta in np.linspace(0, np.pi, 7):
        ax, ay = float(int(R - R * np.cos(theta))), float(int(R - R * np.sin(theta)))
        dx, dy = c - ax, c - ay
        ex, ey = x - ax, y - ay
        len2 = dx * dx + dy * dy
        dot = ex * dx + ey * dy
        gx, gy = x - c, y - c
        cr = dx * ey - dy * ex
        on |= np.where(dot <= 0, ex * ex + ey * ey <= 1.0, np.where(dot >= len2, gx * gx + gy * gy <= 1.0, cr * cr <= 1.0 * len2))
    d2 = (x - c) * (x - c) + (y - c) * (y - c)
    for radius in np.linspace(0, R, 5)[1:]:
        rad = float(int(radius))
        on |= ((rad - 1) * (rad - 1) <= d2) & (d2 <= (rad + 1) * (rad + 1))
    return np.where(on[..., None], np.uint8(255), np.uint8(0)).repeat(3, axis=2)


def _background(max_dist, scale, dev):
    key = (str(dev), float(max_dist), float(scale))
    if key not in _BACKGROUNDS:
        _BACKGROUNDS[key] = torch.from_numpy(np.ascontiguousarray(bev_background(max_dist, scale))).to(dev)
    return _BACKGROUNDS[key]


def pack_boxes(per_image, dev):
    """list of (n_i, 8, 3) host corner arrays -> (corners3d (B, max n_i, 8, 3) float64, counts (B,) int32) on the device"""
    arrs = [np.asarray(a, np.float64).reshape(-1, 8, 3) for a in per_image]
    K = max([len(a) for a in arrs] + [0])
    out = np.zeros((len(arrs), K, 8, 3), np.float64)
    for b, a in enumerate(arrs):
        out[b, :len(a)] = a
    return torch.from_numpy(out).to(dev), torch.tensor([len(a) for a in arrs], dtype=torch.int32).to(dev)


def draw_bev(corners3d, rows, counts, gt=None, max_dist=60, scale=10, palette=PALETTE):
    """the boxes from above -> (B, R, 2R, 3) uint8 on the device, R = max_dist * scale pixels, `scale` pixels per metre, the ego at
    (R, R): a copy of the cached background, the ground truth `gt` = (corners3d (B, Kg, 8, 3), counts (B,)) device tensors, or a list
    of (n_i, 8, 3) host arrays (`corners3d_of`), as green quads, then the predictions over them in their class colours.  The background of a
    (max_dist, scale) is built and uploaded by the first call per device (so call once before capturing); every call paints a copy."""
    c3, rows, counts, B, K = _boxes(corners3d, rows, counts, "draw_bev")
    R = _bev_radius(max_dist, scale)
    canvas = _background(max_dist, scale, c3.device).unsqueeze(0).repeat(B, 1, 1, 1)  # always new memory (also at B = 1): the cached map is never painted
    if gt is not None:
        g3, gn = gt if isinstance(gt, tuple) else pack_boxes(gt, c3.device)
        if g3.shape[0] != B:
            raise Y3DError(f"draw_bev: ground truth for {g3.shape[0]} images, predictions for {B}")
        draw_quads(canvas, *bev_quads(g3, None, gn, scale, R, R, GT_COLOUR))
    return draw_quads(canvas, *bev_quads(c3, rows, counts, scale, R, R, palette))


def corners3d_of(rows):
    """`Object3d.generate_corners3d` (kitti_utils.py:98-114) in host NumPy float64, for ground-truth boxes: rows (n, 14) [cls, alpha, x1,
    y1, x2, y2, h, w, l, x, y, z, ry, score], or an anno dict of `kitti_eval.read_label_file` (dimensions (l, h, w), location,
    rotation_y) -> (n, 8, 3) in the corner order of `y3d_predict3d_rows` (y is the bottom face)"""
    if isinstance(rows, dict):
        dim, loc = np.asarray(rows["dimensions"], np.float64).reshape(-1, 3), np.asarray(rows["location"], np.float64).reshape(-1, 3)
        l, h, w, ry = dim[:, 0], dim[:, 1], dim[:, 2], np.asarray(rows["rotation_y"], np.float64).reshape(-1)
    else:
        r = np.asarray(rows, np.float64).reshape(-1, 14)
        h, w, l, loc, ry = r[:, 6], r[:, 7], r[:, 8], r[:, 9:12], r[:, 12]
    xc = (l / 2)[:, None] * np.array([1.0, 1, -1, -1, 1, 1, -1, -1])
    zc = (w / 2)[:, None] * np.array([1.0, -1, -1, 1, 1, -1, -1, 1])
    yc = -h[:, None] * np.array([0.0, 0, 0, 0, 1, 1, 1, 1])
    c, s = np.cos(ry)[:, None], np.sin(ry)[:, None]
    return np.stack([(c * xc + s * zc) + loc[:, 0:1], yc + loc[:, 1:2], (-s * xc + c * zc) + loc[:, 2:3]], -1)


# ------------------------------------------------------------------------------------------------------------------------------
# label pictures: the decoded labels of a batch (kitti.decode_batch_device) drawn over its images
# ------------------------------------------------------------------------------------------------------------------------------
GT_BOX_COLOUR = ((255, 89, 89),)  # plot_3d_obj's 2D rectangle of a label, (1, 0.35, 0.35) (utils/plotting.py:1408)


def box2d_segments(rows, counts, affine=None, colour=GT_BOX_COLOUR):
    """the 2D rectangles of decoded rows (B, K, 14) (columns 2:6 = x1, y1, x2, y2 in original-image pixels) -> segs (B, K * 4, 4) float64,
    seg_rgb (B, K * 4, 4) uint8: per row the edges top, right, bottom, left, every corner through u' = (A00 u + A01 v) + A02 (v' from
    row 1) when the 2 x 3 `affine` is given, each product and sum rounded on its own as box3d_segments rounds them; the slots behind
    counts are NaN.  Index arithmetic on the device, no read-back."""
    rows = _dev_tensor(rows, torch.float64, "box2d_segments: rows")
    if rows.dim() != 3 or rows.shape[2] != 14 or rows.shape[0] < 1:
        raise Y3DError(f"box2d_segments: rows of shape {tuple(rows.shape)}, expected (B, K, 14)")
    B, K = int(rows.shape[0]), int(rows.shape[1])
    counts = _dev_tensor(counts, torch.int32, "box2d_segments: counts")
    if tuple(counts.shape) != (B,):
        raise Y3DError(f"box2d_segments: counts of shape {tuple(counts.shape)}, expected {(B,)}")
    x1, y1, x2, y2 = (rows[..., c] for c in (2, 3, 4, 5))
    pts = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    if affine is not None:
        A = _dev_tensor(affine, torch.float64, "box2d_segments: affine")
        if A.numel() != B * 6:
            raise Y3DError(f"box2d_segments: {B} images but affine of shape {tuple(A.shape)} (one 2 x 3 matrix each)")
        A = A.reshape(B, 6, 1)
        pts = [(torch.add(torch.add(torch.mul(A[:, 0], u), torch.mul(A[:, 1], v)), A[:, 2]),
                torch.add(torch.add(torch.mul(A[:, 3], u), torch.mul(A[:, 4], v)), A[:, 5])) for u, v in pts]
    segs = torch.stack([torch.stack((pts[e][0], pts[e][1], pts[(e + 1) % 4][0], pts[(e + 1) % 4][1]), -1) for e in range(4)], 2)  # (B, K, 4, 4)
    live = torch.arange(K, device=rows.device).unsqueeze(0) < counts.unsqueeze(1)
    segs = torch.where(live[..., None, None], segs, torch.full_like(segs, float("nan"))).reshape(B, K * 4, 4).contiguous()
    rgb = torch.cat((_palette(colour, rows.device)[0], torch.zeros(1, dtype=torch.uint8, device=rows.device))).repeat(B, K * 4, 1)
    return segs, rgb


def draw_labels3d(canvas, rows, corners3d, counts, P2, affine=None, box2d=True, thickness=2):
    """the decoded labels of `kitti.decode_batch_device` over canvas (B, H, W, 3) uint8, in place: the wireframes in `GT_COLOUR` through
    `box3d_segments` and, with `box2d`, each row's 2D rectangle in `GT_BOX_COLOUR` (four segments, `box2d_segments`), as `plot_3d_obj`
    draws a label (utils/plotting.py:1395-1410).  One `draw_segments` launch: the rectangles hold the lower indices, so they lie over the
    wireframes as there.  P2 (B, 3, 4) float64 projects into the original image; `affine` leads from there to the canvas's frame."""
    segs, rgb = box3d_segments(corners3d, None, counts, P2, affine, GT_COLOUR)
    if box2d:
        s2, c2 = box2d_segments(rows, counts, affine)
        segs, rgb = torch.cat((s2, segs), 1), torch.cat((c2, rgb), 1)
    return draw_segments(canvas, segs, rgb, None, thickness)


def ratio_affine(ratio_pad, n=None):
    """ratio_pad (B, 2, 2) or (B, 2) on the device -> the (n, 2, 3) float64 scaling from the original image to the network frame"""
    rp = _dev_tensor(ratio_pad, torch.float64, "ratio_affine: ratio_pad")
    r = (rp[:, 0] if rp.dim() == 3 else rp)[:n]
    A = torch.zeros(r.shape[0], 2, 3, dtype=torch.float64, device=rp.device)
    A[:, 0, 0], A[:, 1, 1] = r[:, 0], r[:, 1]
    return A


def label_pictures(batch, calibs, P2s, max_imgs=9, cls_mean_size=None, use_camera_dis=False, thickness=2):
    """The array counterpart of `KITTIVisualizer.plot_batch` (utils/plotting.py:1232-1266): the labels of a built batch, decoded with
    undo_augment=False exactly as plot_batch decodes them, drawn over the first `max_imgs` images of `batch["img"]` ((B, H, W, 3) uint8)
    in the network frame (`affine` = the scaling by ratio_pad; the reference resizes the image to the original size instead).
    calibs, P2s: the ORIGINAL images' six constants and projections, as `kitti.decode_batch_device` takes them.
    -> (n, H, W, 3) uint8 on the device, n = min(B, max_imgs); the batch's images are left as they are.
    What the reference's choice implies: a mirrored or cropped training frame is drawn with the original, unmirrored calibration and the
    plain rescale, so its wireframes sit where the reference draws them, not on the augmented objects; validation frames are exact."""
    from . import kitti
    img = batch.get("img") if isinstance(batch, dict) else None
    if not torch.is_tensor(img) or not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise Y3DError("label_pictures: batch['img'] must be a (B, H, W, 3) uint8 tensor on a HIP device (img_mode='uint8')")
    if int(max_imgs) < 1:
        raise Y3DError(f"label_pictures: max_imgs = {max_imgs}")
    rows, c3, _, counts = kitti.decode_batch_device(batch, calibs, P2s, undo_augment=False,
                                                    cls_mean_size=kitti.CLS_MEAN_SIZE if cls_mean_size is None else cls_mean_size,
                                                    use_camera_dis=use_camera_dis)
    n = min(int(img.shape[0]), int(max_imgs))
    P = kitti.p2_device(P2s, int(img.shape[0]), img.device)
    canvas = img[:n].clone()
    return draw_labels3d(canvas, rows[:n].contiguous(), c3[:n].contiguous(), counts[:n].contiguous(), P[:n].contiguous(),
                         ratio_affine(batch["ratio_pad"].to(torch.float64), n), True, thickness)
