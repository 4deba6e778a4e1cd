"""Mints tests/golden/htl.npz from the REFERENCE's `Hierarchical_Task_Learning` (utils/htl.py), run on the CPU:

    python tools/make_golden_htl.py      # needs the reference checkout (oracle.ref_shim.REF_ROOT)

The loss sequences are those of tests/htl_ref.py (`SEQUENCES`); each goes through one fresh `Hierarchical_Task_Learning()` call by call, as
engine/trainer.py:357-358 calls it, and the file records inputs and outputs only: per sequence `epochs`, `losses` (float32) and the `weights`
`compute_weight` returned (float32).  The `constant` sequence is recorded up to the call before the reference raises (`RECORDED`); the
tool checks that the next call does raise."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import htl_ref as H  # noqa: E402
from oracle import ref_shim  # noqa: E402


def reference_class():
    path = os.path.join(ref_shim.REF_ROOT, "ultralytics", "utils", "htl.py")
    spec = importlib.util.spec_from_file_location("reference_htl", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Hierarchical_Task_Learning


def main():
    cls = reference_class()
    out = {}
    for name, (epochs, losses) in H.SEQUENCES.items():
        wt, rows, n = cls(), [], H.RECORDED[name]
        with contextlib.redirect_stdout(io.StringIO()):
            for e, l in zip(epochs[:n], losses[:n]):
                rows.append(wt.compute_weight(torch.from_numpy(l.copy()), int(e)).numpy().copy())
            if n < len(epochs):
                try:
                    wt.compute_weight(torch.from_numpy(losses[n].copy()), int(epochs[n]))
                except KeyError:
                    pass
                else:
                    raise SystemExit(f"{name}: the reference was expected to raise at call {n}")
        w = np.stack(rows)
        assert w.dtype == np.float32
        out[f"{name}/epochs"] = np.asarray(epochs[:n], np.int64)
        out[f"{name}/losses"] = np.asarray(losses[:n], np.float32)
        out[f"{name}/weights"] = w
        print(f"{name}: {n} calls, non-finite weights in rows {sorted(set(np.nonzero(~np.isfinite(w))[0].tolist()))}")
    np.savez_compressed(H.GOLDEN, **out)
    print(f"wrote {H.GOLDEN} ({os.path.getsize(H.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
