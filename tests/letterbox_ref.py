"""The yardstick of `y3d_letterbox_image` (csrc/letterbox.hip) in numpy: pad + tests/yolo2d_ref.py's `resize` (float64 half-pixel-centre
bilinear, taps clamped, rounded to nearest; a plain copy when the size does not change).  Not OpenCV's fixed-point resize."""
import numpy as np

from yolo2d_ref import resize


def letterbox(src, new_h, new_w, top, left, H, W, swap_rb=False):
    """(h0, w0, 3) uint8 -> the (H, W, 3) uint8 canvas: `src` resized to (new_h, new_w) at (top, left), 114 elsewhere"""
    out = np.full((H, W, 3), 114, np.uint8)
    tile = resize(src, new_h, new_w)
    out[top:top + new_h, left:left + new_w] = tile[..., ::-1] if swap_rb else tile
    return out


def canvas(images, rec, H, W):
    """records (B, 8) [src, h0, w0, new_h, new_w, top, left, swap_rb] -> (B, H, W, 3) uint8 (what mode "uint8" holds); a record whose
    source index is outside `images` gives an all-114 image"""
    out = []
    for s, h0, w0, nh, nw, top, left, swap in np.asarray(rec):
        if not 0 <= s < len(images):
            out.append(np.full((H, W, 3), 114, np.uint8))
            continue
        assert images[s].shape[:2] == (h0, w0)
        out.append(letterbox(images[s], nh, nw, top, left, H, W, bool(swap)))
    return np.stack(out)


def to_float(u8):
    """mode "float": (B, 3, H, W) float32 = value / 255 in float32"""
    return np.ascontiguousarray(u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)


def predict_rows(preds, meta, conf, classes=None):
    """`y3d_predict_rows` in numpy float32: preds (B, K, 6), meta (B, 5) [h0, w0, gain, padw, padh] -> (rows (B, K, 6), counts (B,))"""
    preds, meta = np.asarray(preds, np.float32), np.asarray(meta, np.float32)
    out, counts = np.zeros_like(preds), np.zeros(len(preds), np.int32)
    for b, (p, (h0, w0, gain, padw, padh)) in enumerate(zip(preds, meta)):
        keep = p[:, 4] > np.float32(conf)
        if classes is not None:
            keep &= np.isin(p[:, 5], np.asarray(classes, np.float32))
        r = p[keep].copy()
        r[:, [0, 2]] = np.clip((r[:, [0, 2]] - padw) / gain, np.float32(0), w0)
        r[:, [1, 3]] = np.clip((r[:, [1, 3]] - padh) / gain, np.float32(0), h0)
        out[b, :len(r)] = r
        counts[b] = len(r)
    return out, counts
