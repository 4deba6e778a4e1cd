"""float64 numpy restatement of the reference's feature-distillation item: `SupervisionLoss.forward_head` (utils/loss.py:1156-1188)
and its gradient with respect to the embeddings.  Comparator of the host and HIP distillation tests; pinned to the reference itself
by tests/golden/distill.npz (tools/make_golden_distill.py).

Differences from the reference, both stated in the package (csrc/distill.hip):
  * an image with valid objects but no foreground anchor contributes 0 (the reference: 0 / 0 = NaN);
  * `target_gt_idx` indexes the padded object rows; the reference indexes the valid rows, the same thing while the valid rows are a
    prefix (asserted here).
"""
from __future__ import annotations

import numpy as np

CRITERIA = ("soft", "mse", "cos")
COS_EPS = 1e-12  # torch's cosine_embedding_loss adds it to the SQUARED norms


def teacher_pixels(centers, img_wh, map_wh):
    """loss.py:1165-1171 in the reference's own arithmetic: float32 centre / image size * map size, round half to even, clamp.
    centers (..., 2) px; -> (..., 2) int64 (x, y)"""
    c = np.asarray(centers, np.float32)
    out = np.empty(c.shape, np.int64)
    for k in range(2):
        v = c[..., k] / np.float32(img_wh[k]) * np.float32(map_wh[k])
        out[..., k] = np.clip(np.rint(v).astype(np.int64), 0, map_wh[k] - 1)
    return out


def _log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def rows_loss_grad(e, t, T, crit):
    """criterion over the row sets e, t (n_fg, C) of one image -> (loss, d loss / d e)"""
    nf, C = e.shape
    if crit == "soft":
        lp, lq = _log_softmax(t / T), _log_softmax(e / T)
        p = np.exp(lp)
        return (p * (lp - lq)).sum() / nf * T ** 2, (np.exp(lq) * p.sum(-1, keepdims=True) - p) * T / nf
    if crit == "mse":
        d = e - t
        return (d * d).mean(), 2.0 * d / (nf * C)
    if crit == "cos":
        m1, m2 = (e * e).sum(-1, keepdims=True) + COS_EPS, (t * t).sum(-1, keepdims=True) + COS_EPS
        den = np.sqrt(m1 * m2)
        cs = (e * t).sum(-1, keepdims=True) / den
        return (1.0 - cs).mean(), -(t / den - cs * e / m1) / nf
    raise RuntimeError(f"Unknown criterion function: {crit}")


def forward_head(emb, teacher, gt_center, mask_gt, fg, gt_idx, mixed, img_wh, T, weight, crit, no_mixup):
    """emb (B, C, A), teacher (B, C, h, w), gt_center (B, n, 2) px, mask_gt (B, n), fg (B, A), gt_idx (B, A), mixed (B,), img_wh (W, H)
    -> (loss, grad (B, C, A) float64, rows: list of (image, anchor))"""
    emb, teacher = np.asarray(emb, np.float64), np.asarray(teacher, np.float64)
    B, C, A = emb.shape
    h, w = teacher.shape[2:]
    fg, mask_gt = np.asarray(fg).astype(bool), np.asarray(mask_gt).astype(bool)
    grad = np.zeros_like(emb)
    total, rows = 0.0, []
    for b in range(B):
        if not mask_gt[b].any() or (no_mixup and bool(mixed[b])):
            continue
        nv = int(mask_gt[b].sum())
        assert mask_gt[b, :nv].all(), "valid objects must be a prefix of the padded rows"
        a = np.nonzero(fg[b])[0]
        if a.size == 0:
            continue  # the reference: NaN
        px = teacher_pixels(gt_center[b], img_wh, (w, h))[np.asarray(gt_idx)[b, a]]
        t = teacher[b][:, px[:, 1], px[:, 0]].T
        l, g = rows_loss_grad(emb[b][:, a].T, t, float(T), crit)
        total += l
        grad[b][:, a] = g.T * weight
        rows += [(b, int(i)) for i in a]
    return total * weight, grad, rows
