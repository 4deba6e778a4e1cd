"""Loader and host checks of the one-to-many eval fixtures tests/golden/head3d_o2m_eval_{k33,k31}.npz (+ _state.npz), minted by
tools/make_golden_o2m_eval.py from the reference.  Nothing here touches the
device or the library."""
import numpy as np
import torch

from conftest import load_golden

import val_tail_ref as V

TAGS = ("k33", "k31")
NC, MAX_DET, KM, NPROP = 3, 50, 250, 500
SIZES = (32, 16, 8)


def load(tag):
    """-> the fixture as a dict of host tensors: x (list), state, y, y_m, maps_m (list of (B, 38, H, W), rebuilt: `y_m`'s anchors of
    the level with the six raw channels nc .. nc + 6 of `maps_m_raw` put back), rowsO, rowsM, fused, meta = (k1, k2, nl)"""
    g = load_golden(f"head3d_o2m_eval_{tag}")
    g["state"] = load_golden(f"head3d_o2m_eval_{tag}_state")["state"]
    k1, k2, nl = [int(v) for v in g["meta"]]
    flat = g["y_m"].clone()
    flat[:, NC:NC + 6] = g["maps_m_raw"]
    B, maps, a0 = flat.shape[0], [], 0
    for s in SIZES[:nl]:
        maps.append(flat[:, :, a0:a0 + s * s].reshape(B, NC + 35, s, s).contiguous())
        a0 += s * s
    assert a0 == flat.shape[2]
    g["maps_m"] = maps
    return g


_ROWS = {}


def fusion_rows(tag):
    """`val_tail_ref.fusion_rows` of the fixture's reference rows at the validator's defaults (computed once per tag, left unchanged)"""
    if tag not in _ROWS:
        g = load(tag)
        _ROWS[tag] = V.fusion_rows(g["rowsO"], g["rowsM"], V.THRES, V.IOU_THRES, NPROP)
    return _ROWS[tag]


def conditions(tag):
    """the conditions tools/make_golden_o2m_eval.py asserts, recomputed from the file alone -> dict of the measured figures"""
    g = load(tag)
    O, M = g["rowsO"], g["rowsM"]
    rows = fusion_rows(tag)
    n = np.array([r["n"] for r in rows])
    nf, under, smallest = V.fusion_stats(rows, V.TAU_MIXED)
    iou = torch.stack([V.box_iou_xyxy(O[b, :, :4], M[b, :, :4]) for b in range(O.shape[0])])
    w = torch.exp(-torch.cat((O[..., -3].flatten(), M[..., -3].flatten())).double())
    restated = V.kde_fuse_depth(O, M, V.THRES, V.IOU_THRES, NPROP)
    ties = sum(int(t[b, :, 35].unique().numel() != t.shape[1]) for t in (O, M) for b in range(t.shape[0]))
    for t, y in ((O, g["y"]), (M, g["y_m"])):
        best = y[:, :NC].amax(1).sort(1, descending=True)[0]
        ties += int((best[:, t.shape[1] - 1] == best[:, t.shape[1]]).sum())
    return {"score_ties": ties, "rows": int(n.size), "fused": nf, "under_tau": under, "smallest_margin": smallest, "three_voters": int((n >= 3).sum()),
            "lonely": int((n <= 1).sum()), "iou_gap": float((iou.double() - 0.9).abs().min()), "weight_gap": float((w - 0.1).abs().min()),
            "restated_equal": torch.equal(restated.contiguous().view(torch.int32), g["fused"].contiguous().view(torch.int32))}
