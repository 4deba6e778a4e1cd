"""The synthetic validation sets behind tests/golden/det_metrics.npz, rebuilt from a seed wherever they are needed.

tools/make_golden_det_metrics.py scores these sets with the reference and stores only its outputs; the tests rebuild the same inputs
here.  The generator is splitmix64 in Python integers, and every value is made with IEEE additions, multiplications and divisions
only (normal deviates are Irwin-Hall sums of four uniforms), so the sets are bit-identical on every machine and numpy version.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1
SQRT3 = 1.7320508075688772


class SplitMix64:
    def __init__(self, seed):
        self.s = seed & _M64

    def next64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def random(self):
        return (self.next64() >> 11) * (1.0 / (1 << 53))

    def uniform(self, lo, hi, n=None):
        if n is None:
            return lo + (hi - lo) * self.random()
        return np.array([lo + (hi - lo) * self.random() for _ in range(n)])

    def integers(self, lo, hi):
        return lo + int(self.random() * (hi - lo))

    def normal(self, n):
        return np.array([(self.random() + self.random() + self.random() + self.random() - 2.0) * SQRT3 for _ in range(n)])

    def choice(self, p):
        u, acc = self.random(), 0.0
        for i, q in enumerate(p):
            acc += q
            if u < acc:
                return i
        return len(p) - 1

    def permutation(self, n):
        a = list(range(n))
        for i in range(n - 1, 0, -1):
            j = self.integers(0, i + 1)
            a[i], a[j] = a[j], a[i]
        return np.array(a, np.int64)


def jitter(rng, box, s):
    w, h = box[2] - box[0], box[3] - box[1]
    return box + rng.normal(4) * s * np.array([w, h, w, h])


def make_k3(rng, n_img=200, B=8, K=50, nc=3):
    """KITTI-like: decode rows (B, K, 14) fp64 with a keep mask, targets in the original frame"""
    batches = []
    for b0 in range(0, n_img, B):
        nb = min(B, n_img - b0)
        rows = np.zeros((nb, K, 14))
        keep = np.zeros((nb, K), bool)
        bidx, cls, boxes, ori = [], [], [], []
        for i in range(nb):
            h0, w0 = rng.integers(370, 376), rng.integers(1224, 1243)
            ori.append((h0, w0))
            g = []
            for _ in range(rng.integers(0, 12)):
                x1, y1 = rng.uniform(0, w0 - 150), rng.uniform(100, h0 - 60)
                bw, bh = rng.uniform(20, 150), rng.uniform(20, 60)
                c = rng.choice([0.7, 0.2, 0.1])
                g.append((c, np.array([x1, y1, x1 + bw, y1 + bh])))
                bidx.append(i)
                cls.append(c)
                boxes.append([(x1 + bw / 2) / w0, (y1 + bh / 2) / h0, bw / w0, bh / h0])
            k = 0
            for c, box in g:
                for _ in range(rng.integers(0, 4)):
                    if k < K:
                        rows[i, k, 0] = c if rng.random() < 0.85 else rng.integers(0, nc)
                        rows[i, k, 2:6] = jitter(rng, box, rng.uniform(0.01, 0.2))
                        k += 1
            while k < K:
                x1, y1 = rng.uniform(0, w0 - 100), rng.uniform(100, h0 - 50)
                rows[i, k, 0] = rng.integers(0, nc)
                rows[i, k, 2:6] = [x1, y1, x1 + rng.uniform(15, 100), y1 + rng.uniform(15, 50)]
                k += 1
            rows[i] = rows[i, rng.permutation(K)]
            rows[i, :, 13] = rng.uniform(0.0, 1.0, K) ** 2
            keep[i] = rows[i, :, 13] >= 0.05
        batches.append(dict(rows=rows, keep=keep, batch_idx=np.array(bidx, np.float32), cls=np.array(cls, np.float32),
                            bboxes=np.array(boxes, np.float32).reshape(-1, 4), ori_shape=np.array(ori, np.int64)))
    return batches


def letterbox_meta(h0, w0, S=640):
    gain = min(S / h0, S / w0)
    nw, nh = int(round(w0 * gain)), int(round(h0 * gain))
    return gain, (S - nw) / 2, (S - nh) / 2


def make_c2(rng, n_img=150, B=16, K=300, nc=80, S=640):
    """COCO-like: letterboxed (S, S) frames of varied ori_shape / ratio_pad, rows (B, K, 6) [xyxy, conf, cls]"""
    # confidences k / 2^16, distinct over the whole set (single_cls pools the classes), descending within an image (v10postprocess)
    codes = rng.permutation(65535)[:n_img * K].reshape(n_img, K) + 1
    batches = []
    for b0 in range(0, n_img, B):
        nb = min(B, n_img - b0)
        preds = np.zeros((nb, K, 6), np.float32)
        bidx, cls, boxes, ori, rp = [], [], [], [], []
        for i in range(nb):
            h0, w0 = rng.integers(240, 1000), rng.integers(240, 1000)
            gain, pw, ph = letterbox_meta(h0, w0, S)
            ori.append((h0, w0))
            rp.append(((gain, gain), (pw, ph)))
            g = []
            for _ in range(rng.integers(2, 13)):
                bw, bh = rng.uniform(10, w0 / 2), rng.uniform(10, h0 / 2)
                x1, y1 = rng.uniform(-5, w0 - bw + 5), rng.uniform(-5, h0 - bh + 5)  # a few cross the border (clip_boxes)
                c = rng.integers(0, nc) if rng.random() < 0.5 else rng.integers(0, 8)
                lb = np.array([x1, y1, x1 + bw, y1 + bh]) * gain + [pw, ph, pw, ph]  # letterboxed frame
                g.append((c, lb))
                bidx.append(i)
                cls.append(c)
                boxes.append([(lb[0] + lb[2]) / 2 / S, (lb[1] + lb[3]) / 2 / S, (lb[2] - lb[0]) / S, (lb[3] - lb[1]) / S])
            k = 0
            for c, box in g:
                for _ in range(rng.integers(0, 5)):
                    if k < K:
                        preds[i, k, 5] = c if rng.random() < 0.8 else rng.integers(0, nc)
                        preds[i, k, :4] = jitter(rng, box, rng.uniform(0.005, 0.25))
                        k += 1
            while k < K:
                x1, y1 = rng.uniform(0, S - 120), rng.uniform(0, S - 120)
                preds[i, k, 5] = rng.integers(0, nc)
                preds[i, k, :4] = [x1, y1, x1 + rng.uniform(4, 120), y1 + rng.uniform(4, 120)]
                k += 1
            preds[i] = preds[i, rng.permutation(K)]
            preds[i, :, 4] = np.sort(codes[b0 + i])[::-1].astype(np.float32) / np.float32(65536)
        batches.append(dict(preds=preds, batch_idx=np.array(bidx, np.float32), cls=np.array(cls, np.float32).reshape(-1, 1),
                            bboxes=np.array(boxes, np.float32).reshape(-1, 4), ori_shape=np.array(ori, np.int64),
                            ratio_pad=np.array([[list(a), list(b)] for a, b in rp], np.float64), imgsz=np.array([S, S], np.int64)))
    return batches


def make_e3():
    """6 images, K = 8; classes 0..3 (class 3 only in gts, class 2 only in dets)"""
    K = 8
    rows = np.zeros((6, K, 14))
    keep = np.zeros((6, K), bool)
    bidx, cls, boxes = [], [], []
    ori = np.array([[400, 1000]] * 6, np.int64)

    def gt(i, c, x1, y1, x2, y2):
        bidx.append(i)
        cls.append(c)
        boxes.append([(x1 + x2) / 2 / 1000, (y1 + y2) / 2 / 400, (x2 - x1) / 1000, (y2 - y1) / 400])

    def det(i, k, c, box, score):
        rows[i, k, 0], rows[i, k, 2:6], rows[i, k, 13], keep[i, k] = c, box, score, True

    # image 0: no gts, two dets
    det(0, 0, 0, [10, 10, 60, 60], 0.91)
    det(0, 3, 1, [100, 10, 160, 60], 0.42)
    # image 1: gts, no kept det (rows present but not kept)
    gt(1, 0, 100, 100, 200, 200)
    gt(1, 3, 300, 100, 400, 200)
    rows[1, :2, 2:6] = [[100, 100, 200, 200], [300, 100, 400, 200]]
    rows[1, :2, 13] = [0.99, 0.98]
    # image 2: duplicate dets on one gt, and a det of class 2 (no targets of class 2 anywhere)
    gt(2, 0, 100, 100, 200, 200)
    det(2, 0, 0, [101, 100, 200, 201], 0.55)
    det(2, 1, 0, [100, 101, 201, 200], 0.87)
    det(2, 2, 0, [102, 99, 199, 202], 0.33)
    det(2, 4, 2, [100, 100, 200, 200], 0.77)
    # image 3: det 1 (higher IoU with A) loses A to det 0 and does not fall back to B
    gt(3, 1, 100, 100, 200, 200)
    gt(3, 1, 110, 100, 210, 200)
    det(3, 0, 1, [90, 100, 190, 200], 0.61)
    det(3, 1, 1, [103, 100, 203, 200], 0.74)
    det(3, 5, 1, [600, 100, 700, 180], 0.12)
    # image 4: a class-3 gt missed, a class-0 hit
    gt(4, 3, 500, 200, 560, 260)
    gt(4, 0, 10, 10, 110, 90)
    det(4, 2, 0, [12, 11, 108, 92], 0.66)
    det(4, 3, 0, [500, 200, 560, 260], 0.21)
    # image 5: wrong-class overlap and a box at the image border
    gt(5, 1, 0, 0, 80, 50)
    det(5, 0, 0, [0, 0, 80, 50], 0.58)
    det(5, 1, 1, [0, 0, 79, 52], 0.47)
    return [dict(rows=rows, keep=keep, batch_idx=np.array(bidx, np.float32), cls=np.array(cls, np.float32),
                 bboxes=np.array(boxes, np.float32).reshape(-1, 4), ori_shape=ori)]


def make_n3():
    """no true positive anywhere"""
    rows = np.zeros((2, 4, 14))
    keep = np.zeros((2, 4), bool)
    rows[:, :3, 0] = [[0, 1, 0], [2, 0, 1]]
    rows[:, :3, 2:6] = [[500, 100, 560, 150], [10, 300, 40, 330], [700, 50, 720, 90]]
    rows[:, :3, 13] = [[0.9, 0.5, 0.3], [0.8, 0.6, 0.2]]
    keep[:, :3] = True
    return [dict(rows=rows, keep=keep, batch_idx=np.array([0, 1, 1], np.float32), cls=np.array([0, 1, 2], np.float32),
                 bboxes=np.array([[0.1, 0.1, 0.05, 0.1], [0.2, 0.8, 0.1, 0.1], [0.9, 0.9, 0.05, 0.05]], np.float32),
                 ori_shape=np.array([[400, 1000]] * 2))]


def make_tiny(rng):
    """small boxes (normalised coordinates), where the place of box_iou's 1e-7 shows in the rounding: (64, 4), (96, 4) fp32"""
    a = np.stack([rng.uniform(0, 0.01, 2) for _ in range(64)])
    a = np.concatenate((a, a + np.stack([rng.uniform(1e-4, 3e-3, 2) for _ in range(64)])), 1).astype(np.float32)
    b = a[[rng.integers(0, 64) for _ in range(96)]] + (np.stack([rng.normal(4) for _ in range(96)]) * 3e-4).astype(np.float32)
    return a, b


_SETS = None


def input_sets():
    """{"k3", "c2", "c2s", "e3", "n3": [batch dicts], "tiny": (a, b)} — the same on every call and every machine"""
    global _SETS
    if _SETS is None:
        rng = SplitMix64(20261016)
        k3 = make_k3(rng)
        c2 = make_c2(rng)
        c2s = [dict(b, cls=np.zeros_like(b["cls"])) for b in c2]  # a single-class dataset's labels
        _SETS = {"k3": k3, "c2": c2, "c2s": c2s, "e3": make_e3(), "n3": make_n3(), "tiny": make_tiny(SplitMix64(7))}
    return _SETS
