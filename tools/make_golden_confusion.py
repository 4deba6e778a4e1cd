"""Mints tests/golden/confusion.npz from the REFERENCE's own `ConfusionMatrix`, run on the CPU through the reference validators'
`update_metrics` with `args.plots = True` on stub instances.

    python tools/make_golden_confusion.py        # needs the reference checkout (oracle.ref_shim.import_reference)

Built on tools/make_golden_det_metrics.py: importing it makes every socket connect raise OSError before the reference is imported, and
its `run_3d` / `run_2d` drive the validators; here the stubs get `plots = True` and `ConfusionMatrix(nc, conf=args.conf)` as
`init_metrics` builds it (models/yolo/detect/val.py:76).  The inputs are the seeded sets "k3", "c2", "c2s" (single_cls) and "n3" of
tests/det_metrics_sets.py and the edge images "x3" of tests/confusion_ref.py, so the fixture holds only the reference's matrices.

The reference's `argsort()[::-1]` is an unstable sort, so the script asserts what makes its output independent of the sort: among the
pairs above the IoU threshold (detections above the confidence threshold, any classes), no two that share a detection and no two that
share a gt have equal IoU.  ("e3" of det_metrics_sets.py breaks that, which is why the edge images are a set of their own.)
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_det_metrics as G  # noqa: E402  (disables the sockets, puts the repository and tests/ on sys.path)
import confusion_ref as CR  # noqa: E402

OUT = os.path.join(G.ROOT, "tests", "golden", "confusion.npz")


def assert_sort_independent(M, name, single_cls):
    worst = 0
    for n, (g, gc, box, cf, dc) in enumerate(CR.images(CR.batches_of(name), single_cls)):
        part = cf > (np.float32(CR.CONF) if cf.dtype == np.float32 else CR.CONF)
        if not len(gc) or not part.any():
            continue
        iou = M.box_iou(torch.from_numpy(g), torch.from_numpy(box[part])).numpy()
        above = iou > np.float32(CR.IOU_THRES)
        for d in range(iou.shape[1]):
            col = iou[above[:, d], d]
            assert np.unique(col).size == col.size, f"{name}: image {n}, detection {d}: two gts above the threshold with equal IoU"
        for i in range(iou.shape[0]):
            row = iou[i, above[i]]
            assert np.unique(row).size == row.size, f"{name}: image {n}, gt {i}: two detections above the threshold with equal IoU"
        worst = max(worst, int(above.sum()))
    return worst


def main():
    VD, V3, M, ops = G.load_reference()
    stub = G.stub_common

    def stub_with_plots(v, M_, nc, single_cls, metrics_cls):
        stub(v, M_, nc, single_cls, metrics_cls)
        v.args.plots = True
        v.confusion_matrix = M_.ConfusionMatrix(nc=nc, conf=v.args.conf)

    G.stub_common = stub_with_plots
    out = {}
    for name, (src, nc, single_cls) in CR.SETS.items():
        pairs = assert_sort_independent(M, name, single_cls)
        sets = CR.batches_of(src)
        v = (G.run_3d(V3, M, ops, sets, nc, single_cls) if "rows" in sets[0] else G.run_2d(VD, M, sets, nc, single_cls))[0]
        cm = v.confusion_matrix
        assert cm.conf == 0.25 and cm.iou_thres == 0.45
        m = np.asarray(cm.matrix)
        assert m.shape == (nc + 1, nc + 1) and np.array_equal(m, np.round(m))
        out[name] = m.astype(np.int32)
        print(name, "sum", int(m.sum()), "matched", int(m[:nc, :nc].sum()), "missed", int(m[nc].sum()), "background", int(m[:, nc].sum()),
              "| most pairs above the threshold in one image:", pairs)
    assert out["n3"][:3].sum() == 0 and out["n3"][3].sum() > 0  # no match anywhere: only missed gts
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
