"""The yardstick of csrc/yolo2d_batch.hip: the image arithmetic of `y3d_yolo2d_image_aug` in numpy float64, in the kernel's order
of operations (its header comment), and the label arithmetic of `y3d_yolo2d_encode_labels` in numpy float32 as the reference's
`Instances` / `RandomPerspective` compute it.

This is NOT OpenCV: `cv2.resize` / `cv2.warpAffine` interpolate in fixed point (coordinates quantised to 1/32 px, integer weights) and
the 8-bit HSV conversions use integer tables; none of that is reproduced.  How far real OpenCV output lies from this arithmetic has
not been measured (tools/make_golden_yolo2d.py --cv2 records it where OpenCV is installed).

Images are (H, W, 3) uint8 in the decoded channel order (RGB from PIL); the reference works on BGR, which only renames channels
until the HSV stage, where the channels are taken by name."""
import numpy as np


def _lerp2(p00, p01, p10, p11, ax, ay):
    return ((p00 * (1.0 - ax) + p01 * ax) * (1.0 - ay)) + ((p10 * (1.0 - ax) + p11 * ax) * ay)


def resize(src, h, w):
    """`load_image`'s resize: bilinear in the half-pixel-centre convention, taps clamped to the image, rounded to nearest"""
    src = np.asarray(src)
    h0, w0 = src.shape[:2]
    if (h, w) == (h0, w0):
        return src.copy()

    def axis(n, n0):
        f = (np.arange(n, dtype=np.float64) + 0.5) * (float(n0) / float(n)) - 0.5
        i0 = np.floor(f)
        b = f - i0
        i0 = i0.astype(np.int64)
        lo, hi = i0 < 0, i0 >= n0 - 1
        b[lo | hi] = 0.0
        i0[lo] = 0
        i0[hi] = n0 - 1
        return i0, np.minimum(i0 + 1, n0 - 1), b

    y0, y1, by = axis(h, h0)
    x0, x1, bx = axis(w, w0)
    s = src.astype(np.float64)
    bx, by = bx[None, :, None], by[:, None, None]
    v = _lerp2(s[y0][:, x0], s[y0][:, x1], s[y1][:, x0], s[y1][:, x1], bx, by)
    return np.floor(v + 0.5).astype(np.uint8)


def canvas(pre, images):
    """the mosaic (2S x 2S) or letter-box (S x S) canvas of one `pre` record of yolo2d.sample_augment; images: frame -> (h0, w0, 3)"""
    C = pre["canvas"]
    out = np.full((C, C, 3), 114, np.uint8)
    for t in pre["tiles"]:
        if t["x2a"] <= t["x1a"] or t["y2a"] <= t["y1a"]:
            continue
        tile = resize(images[t["frame"]], t["h"], t["w"])
        ys = np.arange(t["y1a"], t["y2a"]) - t["padh"]
        xs = np.arange(t["x1a"], t["x2a"]) - t["padw"]
        out[t["y1a"]:t["y2a"], t["x1a"]:t["x2a"]] = tile[ys][:, xs]
    return out


def warp(cv, inv, S, flipud=False, fliplr=False):
    """the (S, S, 3) output of one layer: bilinear taps on the canvas at inv @ (ux, uy, 1), border 114, rounded to nearest"""
    C = cv.shape[0]
    oy, ox = np.mgrid[0:S, 0:S]
    ux = (S - 1 - ox if fliplr else ox).astype(np.float64)
    uy = (S - 1 - oy if flipud else oy).astype(np.float64)
    sx = (inv[0] * ux + inv[1] * uy) + inv[2]
    sy = (inv[3] * ux + inv[4] * uy) + inv[5]
    ok = (sx > -1.0) & (sx < C) & (sy > -1.0) & (sy < C)
    sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
    xf, yf = np.floor(sx), np.floor(sy)
    ax, ay = (sx - xf)[..., None], (sy - yf)[..., None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    pad = np.full((C + 2, C + 2, 3), 114.0)
    pad[1:-1, 1:-1] = cv
    tap = lambda yy, xx: pad[np.clip(yy + 1, 0, C + 1), np.clip(xx + 1, 0, C + 1)]
    v = np.floor(_lerp2(tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1), ax, ay) + 0.5)
    v[~ok] = 114.0
    return v.astype(np.uint8)


def mixup(a, b, r):
    """`(img * r + img2 * (1 - r)).astype(np.uint8)`: truncation"""
    return np.floor(a.astype(np.float64) * r + b.astype(np.float64) * (1.0 - r)).astype(np.uint8)


def rgb_to_hsv(img):
    """(.., 3) r, g, b -> H in 0..179, S, V in 0..255, rounded to nearest (float64 arithmetic, no tables)"""
    v = np.asarray(img, np.float64)
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    V = np.maximum(r, np.maximum(g, b))
    d = V - np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        Sat = np.where(V == 0.0, 0.0, np.floor(255.0 * d / V + 0.5))
        hd = np.where(d == 0.0, 0.0, np.where(V == r, 60.0 * (g - b) / d, np.where(V == g, 120.0 + 60.0 * (b - r) / d, 240.0 + 60.0 * (r - g) / d)))
    hd = np.where(hd < 0.0, hd + 360.0, hd)
    H = np.floor(hd / 2.0 + 0.5)
    H = np.where(H >= 180.0, H - 180.0, H)
    return H, Sat, V


def hsv_to_rgb(H, Sat, V):
    hh = H / 30.0
    fi = np.floor(hh)
    f = hh - fi
    s = Sat / 255.0
    p, q, t = V * (1.0 - s), V * (1.0 - s * f), V * (1.0 - s * (1.0 - f))
    i = fi.astype(np.int64)
    i = np.where(i > 5, i - 6, i)
    R = np.choose(i, [V, q, p, p, t, V])
    G = np.choose(i, [t, V, V, q, p, p])
    B = np.choose(i, [p, p, t, V, V, q])
    return np.floor(np.stack([R, G, B], -1) + 0.5).astype(np.uint8)


def hsv(img, lut):
    """RandomHSV with the three (256,) uint8 tables of yolo2d.hsv_luts"""
    H, Sat, V = rgb_to_hsv(img)
    lut = np.asarray(lut)
    return hsv_to_rgb(lut[0][H.astype(np.int64)].astype(np.float64), lut[1][Sat.astype(np.int64)].astype(np.float64),
                      lut[2][V.astype(np.int64)].astype(np.float64))


def image(sample, images, S, lut=None):
    """one sample of yolo2d.sample_augment -> (S, S, 3) uint8 in the output's channel order (what img_mode "uint8" holds)"""
    out = warp(canvas(sample["pre"], images), sample["pre"]["M_inv"], S, sample["flipud"], sample["fliplr"])
    if sample["pre2"] is not None:
        out = mixup(out, warp(canvas(sample["pre2"], images), sample["pre2"]["M_inv"], S, sample["flipud"], sample["fliplr"]), sample["r"])
    if sample["hsv_gain"] is not None:
        from yolov10_3d_amd import yolo2d
        out = hsv(out, yolo2d.hsv_luts(sample["hsv_gain"]) if lut is None else lut)
    return out if sample["rgb"] else out[..., ::-1].copy()


def image_float(u8):
    """img_mode "float": (3, S, S) float32 = value / 255 in float32"""
    return np.ascontiguousarray(u8.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def labels(sample, label_rows, S):
    """The label arithmetic for one sample in numpy float32, step by step as the reference does it.  label_rows[frame]: (n, 5) float32.
    -> cls (n, 1) float32, boxes (n, 4) float32 xywh normalised, and `diag`: per candidate of the training path the quantities every
    decision is taken on (frame, row, layer, area, w2, h2, ratio, ar and the four verdicts)."""
    f32 = np.float32
    S32, inv = f32(S), f32(1.0 / S)
    cls_out, box_out, diag = [], [], []
    train = sample["mode"] == "train"
    for layer, pre in enumerate((sample["pre"], sample["pre2"])):
        if pre is None:
            continue
        M = np.asarray(pre["M"], f32)
        for t in pre["tiles"]:
            rows = np.asarray(label_rows[t["frame"]], f32).reshape(-1, 5)
            for n, r in enumerate(rows):
                dw, dh = r[3] / f32(2), r[4] / f32(2)
                b = np.array([r[1] - dw, r[2] - dh, r[1] + dw, r[2] + dh], f32)
                b *= np.array([t["w"], t["h"], t["w"], t["h"]], f32)
                b += np.array([t["lab_padw"], t["lab_padh"], t["lab_padw"], t["lab_padh"]], f32)
                keep, area = True, f32(-1)
                if pre["mosaic"]:
                    b = np.clip(b, f32(0), f32(2) * S32)
                    area = (b[2] - b[0]) * (b[3] - b[1])
                    keep = bool(area > 0)
                if train:
                    xs, ys = [], []
                    for px, py in ((b[0], b[1]), (b[2], b[3]), (b[0], b[3]), (b[2], b[1])):
                        xs.append((px * M[0, 0] + py * M[0, 1]) + M[0, 2])
                        ys.append((px * M[1, 0] + py * M[1, 1]) + M[1, 2])
                    nb = np.clip(np.array([min(xs), min(ys), max(xs), max(ys)], f32), f32(0), S32)
                    sc, eps = f32(pre["scale"]), f32(1e-16)
                    w1, h1 = b[2] * sc - b[0] * sc, b[3] * sc - b[1] * sc
                    w2, h2 = nb[2] - nb[0], nb[3] - nb[1]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ar = max(w2 / (h2 + eps), h2 / (w2 + eps))
                        ratio = w2 * h2 / (w1 * h1 + eps)
                    v = (bool(w2 > f32(2)), bool(h2 > f32(2)), bool(ratio > f32(0.1)), bool(ar < f32(100)))
                    if keep:
                        diag.append(dict(frame=t["frame"], row=n, layer=layer, area=float(area), w2=float(w2), h2=float(h2),
                                         ratio=float(ratio), ar=float(ar), verdicts=v))
                    elif pre["mosaic"]:
                        diag.append(dict(frame=t["frame"], row=n, layer=layer, area=float(area), w2=None, h2=None, ratio=None, ar=None, verdicts=None))
                    keep = keep and all(v)
                    b = nb
                if not keep:
                    continue
                o = np.array([(b[0] + b[2]) / f32(2), (b[1] + b[3]) / f32(2), b[2] - b[0], b[3] - b[1]], f32) * inv
                if train:
                    if sample["flipud"]:
                        o[1] = f32(1) - o[1]
                    if sample["fliplr"]:
                        o[0] = f32(1) - o[0]
                    o = o * S32 * inv
                cls_out.append(r[0])
                box_out.append(o)
    return (np.array(cls_out, f32).reshape(-1, 1), np.array(box_out, f32).reshape(-1, 4), diag)
