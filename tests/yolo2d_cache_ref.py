"""Numpy restatement of `y3d_yolo2d_plan_batch` (csrc/yolo2d_cache.hip): the five record arrays of `y3d_yolo2d_image_aug` and
`y3d_yolo2d_encode_labels` from a resident split's frame tables and one table of draws, in the kernel's order of operations (its header
comment).  Nothing here calls `yolo2d.image_records` / `label_records` / `hsv_luts`: tests/test_yolo2d_cache_host.py ties this file to
them, tests/test_hip_yolo2d_cache.py ties the kernel to this file."""
import math

import numpy as np

DRAW_W, LAYER, TAIL = 56, 23, 46
OUTPUTS = (("rec_i", np.int32, (112,)), ("rec_f", np.float64, (16,)), ("lut", np.uint8, (3, 256)), ("lab_i", np.int32, (20,)),
           ("lab_f", np.float32, (48,)))


def resized(h0, w0, S):
    """load_image's size after the resize to long side S, float64"""
    r = np.float64(S) / np.float64(max(h0, w0))
    if r == 1.0:
        return int(h0), int(w0)
    return min(int(math.ceil(np.float64(h0) * r)), S), min(int(math.ceil(np.float64(w0) * r)), S)


def tile(k, mosaic, h, w, yc, xc, S):
    """-> (x1a, y1a, x2a, y2a, padw, padh, label padw, label padh) of tile k"""
    if mosaic:
        C = 2 * S
        if k == 0:
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
        elif k == 1:
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, C), yc
            x1b, y1b = 0, h - (y2a - y1a)
        elif k == 2:
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(C, yc + h)
            x1b, y1b = w - (x2a - x1a), 0
        else:
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, C), min(C, yc + h)
            x1b, y1b = 0, 0
        padw, padh = x1a - x1b, y1a - y1b
        return x1a, y1a, x2a, y2a, padw, padh, np.float32(padw), np.float32(padh)
    dw, dh = np.float64(S - w) / 2.0, np.float64(S - h) / 2.0
    top, left = int(np.rint(dh - 0.1)), int(np.rint(dw - 0.1))
    return left, top, left + w, top + h, left, top, np.float32(dw), np.float32(dh)


def luts(gain):
    """the three HSV tables from the float64 gains -> (3, 256) uint8"""
    x = np.arange(256, dtype=np.float64)
    t = x * np.float64(gain[0])
    m = np.fmod(t, 180.0)
    m = np.where((m != 0.0) & (m < 0.0), m + 180.0, m)
    out = [m.astype(np.int32).astype(np.uint8)]
    for c in (1, 2):
        t = x * np.float64(gain[c])
        out.append(np.minimum(np.maximum(t, 0.0), 255.0).astype(np.int32).astype(np.uint8))
    return np.stack(out)


def plan(frame_hw, rec_span, S, draws):
    """frame_hw (N, 2) int32, rec_span (N, 2) int32, imgsz, draws (B, 56) float64 -> dict of the five arrays"""
    draws = np.asarray(draws, np.float64)
    B, N = len(draws), len(frame_hw)
    o = {k: np.zeros((B,) + s, dt) for k, dt, s in OUTPUTS}
    for b, d in enumerate(draws):
        for l in range(2):
            L = d[l * LAYER:(l + 1) * LAYER]
            if L[0] == 0.0:
                continue
            mosaic = L[1] != 0.0
            nt = 4 if mosaic else 1
            o["rec_i"][b, l * 50], o["rec_i"][b, l * 50 + 1] = nt, int(L[9])
            o["lab_i"][b, 16 + l] = 1 | (2 if mosaic else 0) | (4 if L[2] != 0.0 else 0)
            o["lab_f"][b, 32 + l * 8:32 + l * 8 + 6] = L[10:16].astype(np.float32)
            o["lab_f"][b, 32 + l * 8 + 6] = np.float32(L[22])
            o["rec_f"][b, l * 6:l * 6 + 6] = L[16:22]
            for k in range(nt):
                f = int(L[3 + k])
                if not 0 <= f < N:
                    continue
                h0, w0 = int(frame_hw[f, 0]), int(frame_hw[f, 1])
                h, w = resized(h0, w0, S)
                x1a, y1a, x2a, y2a, padw, padh, lpw, lph = tile(k, mosaic, h, w, int(L[7]), int(L[8]), S)
                q = l * 4 + k
                o["rec_i"][b, l * 50 + 2 + k * 12:l * 50 + 2 + k * 12 + 11] = (f, h0, w0, h, w, x1a, y1a, x2a, y2a, padw, padh)
                o["lab_i"][b, 2 * q:2 * q + 2] = rec_span[f]
                o["lab_f"][b, 4 * q:4 * q + 4] = (np.float32(w), np.float32(h), lpw, lph)
        T = d[TAIL:]
        flipud, fliplr = int(T[6] != 0.0), int(T[7] != 0.0)
        o["rec_i"][b, 100:105] = (flipud, fliplr, int(T[8] != 0.0), int(T[2] != 0.0), int(T[0] != 0.0))
        o["lab_i"][b, 18] = flipud | (fliplr << 1)
        o["rec_f"][b, 12] = T[1]
        if T[2] != 0.0:
            o["lut"][b] = luts(T[3:6])
    return o
