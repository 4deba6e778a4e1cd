"""CPU: the box metrics' host side (yolov10-3d_amd/metrics.py) — ABI declarations, refusals, and numpy restatements of what the
kernels of csrc/det_metrics.hip compute (the claim-table matching rule, np.interp by grid ownership, compute_ap's trapezoid), held to
the reference's own outputs in tests/golden/det_metrics.npz (minted by tools/make_golden_det_metrics.py) and to numpy."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from det_metrics_sets import input_sets

import yolov10_3d_amd as y3d
from yolov10_3d_amd import _lib
from yolov10_3d_amd import metrics as DM

IOUV32 = torch.linspace(0.5, 0.95, 10).numpy()


def golden():
    return np.load(os.path.join(GOLDEN, "det_metrics.npz"))


def batches(name):
    """the input set `name` as per-batch dicts (the layout BoxStats.update_* and the reference validators took), rebuilt from its seed"""
    return input_sets()[name]


CURVE_ROWS = {"k3": slice(None), "e3": slice(None), "c2": slice(None, None, 16)}  # the classes whose curves the fixture stores


# ------------------------------------------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------------------------------------------
def iou_f32(gt, det, eps=np.float32(1e-7)):
    """box_iou in fp32, the reference's operation order"""
    a, b = gt.astype(np.float32)[:, None, :], det.astype(np.float32)[None, :, :]
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), np.float32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), np.float32(0))
    inter = iw * ih
    return inter / (((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter) + eps)


def claim_rule(iou, gt_cls, det_cls, thr=IOUV32):
    """the kernel's rule: L(d) = best class-matched label (ties -> higher gt index), m(d) its IoU; d is a TP at t iff m(d) >= t and
    no lower-index d' with L(d') = L(d) has m(d') >= t.  -> (n_det,) int masks"""
    n_gt, n_det = iou.shape
    out = np.zeros(n_det, np.int64)
    if n_gt == 0:
        return out
    v = np.where(np.asarray(gt_cls)[:, None] == np.asarray(det_cls)[None, :], iou, np.float32(0))
    L = n_gt - 1 - np.argmax(v[::-1], axis=0)  # the last maximum
    m = v[L, np.arange(n_det)]
    for t, th in enumerate(thr):
        seen = set()
        for d in range(n_det):
            if m[d] >= th and L[d] not in seen:
                out[d] |= 1 << t
            if m[d] >= th:
                seen.add(L[d])
    return out


def two_unique(iou, gt_cls, det_cls, thr=IOUV32):
    """match_predictions' two np.unique steps (use_scipy = False), restated; stable orders where the reference's are unstable"""
    v = iou * (np.asarray(gt_cls)[:, None] == np.asarray(det_cls)[None, :])
    out = np.zeros(iou.shape[1], np.int64)
    for t, th in enumerate(thr):
        mt = np.array(np.nonzero(v >= th)).T
        if mt.shape[0] > 1:
            mt = mt[v[mt[:, 0], mt[:, 1]].argsort(kind="stable")[::-1]]
            mt = mt[np.unique(mt[:, 1], return_index=True)[1]]
            mt = mt[np.unique(mt[:, 0], return_index=True)[1]]
        for d in mt[:, 1] if mt.shape[0] else []:
            out[d] |= 1 << t
    return out


def prep_3d(b, i):
    m = b["batch_idx"] == i
    q = b["bboxes"][m].astype(np.float32)
    dw, dh = q[:, 2] / np.float32(2), q[:, 3] / np.float32(2)
    g = np.stack((q[:, 0] - dw, q[:, 1] - dh, q[:, 0] + dw, q[:, 1] + dh), 1) * np.float32(b["ori_shape"][i][[1, 0, 1, 0]]).astype(np.float32)
    d = b["rows"][i][b["keep"][i]]
    return g, b["cls"][m], d[:, 2:6].astype(np.float32), d[:, 0]


def scale_f32(x, gain, pw, ph, h0, w0):
    x = x.copy()
    x[:, [0, 2]] -= np.float32(pw)
    x[:, [1, 3]] -= np.float32(ph)
    x /= np.float32(gain)
    x[:, [0, 2]] = np.clip(x[:, [0, 2]], 0, np.float32(w0))
    x[:, [1, 3]] = np.clip(x[:, [1, 3]], 0, np.float32(h0))
    return x


def prep_2d(b, i, single_cls=False):
    m = b["batch_idx"] == i
    q = b["bboxes"][m].astype(np.float32)
    S = np.float32(b["imgsz"][0])
    dw, dh = q[:, 2] / np.float32(2), q[:, 3] / np.float32(2)
    g = np.stack((q[:, 0] - dw, q[:, 1] - dh, q[:, 0] + dw, q[:, 1] + dh), 1) * S
    rp, (h0, w0) = b["ratio_pad"][i], b["ori_shape"][i]
    g = scale_f32(g, rp[0, 0], rp[1, 0], rp[1, 1], h0, w0)
    d = b["preds"][i]
    return g, b["cls"][m].reshape(-1), scale_f32(d[:, :4], rp[0, 0], rp[1, 0], rp[1, 1], h0, w0), (0 * d[:, 5] if single_cls else d[:, 5])


def interp_owned(x, xp, fp, left, right):
    """np.interp by ownership, as the kernels write it: sample j owns the queries in [xp[j], xp[j+1]) (j = the LAST index with
    xp[j] <= x); below xp[0] -> left; at or beyond the last sample -> fp[-1] (or right past it)"""
    out = np.empty(len(x))
    n = len(xp)
    for k, v in enumerate(x):
        j = np.searchsorted(xp, v, side="right") - 1
        if j < 0:
            out[k] = left
        elif j == n - 1:
            out[k] = fp[j] if v == xp[j] else right
        elif v == xp[j]:
            out[k] = fp[j]
        else:
            out[k] = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (v - xp[j]) + fp[j]
    return out


def trapz_pairwise(y, x):
    """np.trapz's add.reduce over <= 128 terms: 8 running sums, combined pairwise, then the remainder, from 0.0"""
    a = (x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0
    m = len(a)
    if m < 8:
        s = 0.0
        for v in a:
            s += v
        return 0.0 + s
    r = list(a[:8])
    k = 8
    while k < m - m % 8:
        for j in range(8):
            r[j] += a[k + j]
        k += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[k:]:
        s += v
    return 0.0 + s


def compute_ap_restated(recall, precision):
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    env = np.maximum.accumulate(mpre[::-1])[::-1]
    x = np.linspace(0, 1, 101)
    return trapz_pairwise(interp_owned(x, mrec, env, env[0], env[-1]), x)


# ------------------------------------------------------------------------------------------------------------------------------
def test_prototypes_declared():
    protos = _lib.parse_header()
    for name in ("y3d_det_metrics_max_gts", "y3d_det_metrics_max_dets", "y3d_box_iou", "y3d_match_predictions", "y3d_box_match_batch",
                 "y3d_ap_per_class"):
        assert name in protos, name
    assert {"det_metrics_max_gts", "det_metrics_max_dets"} <= _lib._PLAIN_INT
    assert y3d.lib().det_metrics_max_gts() >= 512 and y3d.lib().det_metrics_max_dets() >= 1000
    assert y3d.metrics.Det3dMetrics().fitness == 0


def test_refusals():
    box = torch.tensor([[0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(y3d.Y3DError):
        DM.box_iou(box, box)
    with pytest.raises(y3d.Y3DError):
        DM.match_predictions(torch.zeros(1), torch.zeros(1), torch.zeros(1, 1))
    with pytest.raises(y3d.Y3DError):
        DM.process_batch(torch.zeros(1, 6), box, torch.zeros(1))
    with pytest.raises(y3d.Y3DError, match="at most"):
        DM.match_predictions(torch.zeros(4), torch.zeros(DM.max_gts() + 1), torch.zeros(DM.max_gts() + 1, 4))
    with pytest.raises(y3d.Y3DError, match="at most"):
        DM.match_predictions(torch.zeros(DM.max_dets() + 1), torch.zeros(3), torch.zeros(3, DM.max_dets() + 1))
    with pytest.raises(y3d.Y3DError, match="plot"):
        DM.ap_per_class(torch.zeros(1, 10, dtype=torch.bool), torch.zeros(1), torch.zeros(1), torch.zeros(1), plot=True)
    with pytest.raises(y3d.Y3DError):
        DM.ap_per_class(torch.zeros(1, 10, dtype=torch.bool), torch.zeros(1), torch.zeros(1), torch.zeros(1))
    with pytest.raises(y3d.Y3DError):
        DM.BoxStats(80, device="cpu")
    st = object.__new__(DM.BoxStats)  # the per-image row limit is checked before anything touches a device
    with pytest.raises(y3d.Y3DError, match="at most"):
        st.update_2d(torch.zeros(1, DM.max_dets() + 1, 6), {})
    with pytest.raises(y3d.Y3DError, match="at most"):
        st.update_3d(torch.zeros(1, DM.max_dets() + 1, 14), torch.ones(1, DM.max_dets() + 1, dtype=torch.bool), {})


def test_iou_restatement_is_bit_exact():
    z = golden()
    np.testing.assert_array_equal(iou_f32(z["one/gt"], z["one/det"][:, :4]), z["one/iou"])
    np.testing.assert_array_equal(iou_f32(*input_sets()["tiny"]), z["tiny/iou"])


@pytest.mark.parametrize("name", ["k3", "e3", "n3", "c2", "c2s"])
def test_claim_rule_reproduces_the_reference_tp(name):
    z = golden()
    got = []
    for b in batches(name):
        n_img = len(b["rows"] if "rows" in b else b["preds"])
        for i in range(n_img):
            g, gc, d, dc = prep_3d(b, i) if "rows" in b else prep_2d(b, i, name == "c2s")
            got.append(claim_rule(iou_f32(g, d), gc, dc))
    got = np.concatenate(got)
    np.testing.assert_array_equal(got, z[f"{name}/tp"].astype(np.int64) & 0x3FF)


def test_claim_rule_equals_two_unique_on_random_cases():
    rng = np.random.default_rng(3)
    for _ in range(300):
        ng, nd = int(rng.integers(0, 9)), int(rng.integers(1, 14))
        g = rng.uniform(0, 50, (ng, 2))
        g = np.concatenate((g, g + rng.uniform(5, 30, (ng, 2))), 1)
        src = g[rng.integers(0, max(ng, 1), nd)] if ng else rng.uniform(0, 50, (nd, 4))
        d = src + rng.normal(0, 3, (nd, 4))
        gc, dc = rng.integers(0, 3, ng), rng.integers(0, 3, nd)
        iou = iou_f32(g, d)
        np.testing.assert_array_equal(claim_rule(iou, gc, dc), two_unique(iou, gc, dc))


def test_interp_restatement_equals_np_interp_with_duplicate_xp():
    rng = np.random.default_rng(5)
    x = np.linspace(0, 1, 101)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        xp = np.sort(np.round(rng.uniform(0, 1, n), 1))  # many duplicates, some on grid points
        xp = np.concatenate(([0.0], xp, [1.0]))
        fp = rng.uniform(0, 1, xp.size)
        for left, right in ((0.0, 0.0), (1.0, fp[-1])):
            np.testing.assert_array_equal(interp_owned(x, xp, fp, left, right), np.interp(x, xp, fp, left=left, right=right))
            np.testing.assert_array_equal(interp_owned(-x, -xp[::-1], fp, left, right), np.interp(-x, -xp[::-1], fp, left=left, right=right))


def test_compute_ap_restatement_is_bit_exact():
    rng = np.random.default_rng(9)
    for _ in range(200):
        n, nl = int(rng.integers(1, 60)), int(rng.integers(1, 30))
        tp = rng.random(n) < 0.4
        tpc = np.minimum(np.cumsum(tp), nl)
        recall, precision = tpc / (nl + 1e-16), tpc / np.arange(1, n + 1)
        mrec, mpre = np.concatenate(([0.0], recall, [1.0])), np.concatenate(([1.0], precision, [0.0]))
        mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
        x = np.linspace(0, 1, 101)
        want = getattr(np, "trapezoid", getattr(np, "trapz", None))(np.interp(x, mrec, mpre), x)  # np.trapz, renamed in numpy 2
        assert compute_ap_restated(recall, precision) == want


@pytest.mark.parametrize("name", ["k3", "e3"])  # (the fixture keeps a sample of c2's curves only)
def test_host_operating_point_reproduces_p_r_f1(name):
    z = golden()
    ci = z[f"{name}/ap_class_index"]
    nt = z[f"{name}/nt_per_class"][ci]
    r = DM._operating_point(z[f"{name}/all_ap"], z[f"{name}/p_curve"], z[f"{name}/r_curve"], ci, nt, 1e-16)
    np.testing.assert_array_equal(r[2], z[f"{name}/p"])
    np.testing.assert_array_equal(r[3], z[f"{name}/r"])
    np.testing.assert_array_equal(r[4], z[f"{name}/f1"])
    np.testing.assert_array_equal(r[6], ci)


def test_metric_classes_follow_the_reference_formulas():
    z = golden()
    for name, cls in (("c2", DM.Det3dMetrics), ("c2d", DM.DetMetrics)):
        m = cls(names={i: str(i) for i in range(80)})
        ci = z[f"{name}/ap_class_index"]
        m._update((None, None, z[f"{name}/p"], z[f"{name}/r"], z[f"{name}/f1"], z[f"{name}/all_ap"], ci, None, None, None, None, None))
        got = np.array([float(v) for v in m.results_dict.values()])
        np.testing.assert_allclose(got, z[f"{name}/results"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(m.maps, z[f"{name}/maps"], rtol=0, atol=1e-12)
        assert list(m.results_dict) == m.keys + ["fitness"]
