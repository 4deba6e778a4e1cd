"""Records tests/golden/label3d_pin.npz: what THIS build's 3D label encoders and plan kernels compute, byte for byte, on the inputs of
tests/label3d_pin_cases.py.  Needs a GPU.

    python tools/make_golden_label3d_pin.py [--out PATH]

The file is a pin, not a parity fixture: tests/test_hip_label3d_pin.py holds a later build to the same bytes, so record it from the
build whose behaviour is to be kept (a checkout of the commit before a refactor of csrc/label3d.h and its four sources), never from
the tree under test.  It also stores the SHA-256 of the generated inputs, and a host-side float64 estimate of how many candidate
lines lie on each side of every geometric filter is printed and asserted, so a pin that misses a filter arm is not written.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label3d_pin_cases as C  # noqa: E402


def coverage(kind):
    """lines of the unmirrored and the mirrored run on each side of the depth and centre filters, estimated in float64 on the host"""
    rec, images = C.encoder_tables(kind)
    out_w, out_h = C.GEOMETRY["kitti" if kind == "kitti" else "json3d"][0]
    h, pos = (rec[:, 7], rec[:, 10:13]) if kind == "kitti" else (rec[:, 5], rec[:, 8:11])
    seen = {}
    for (row, n0, n1), _, P, Pm, t, s in images:
        for flip, Q in ((0, P), (1, Pm)):
            p = pos[row:row + n0 + n1].copy()
            p[:, 0] *= -1 if flip else 1
            p[:, 1] -= h[row:row + n0 + n1] / 2
            u = (p @ Q[0:3] + Q[3]) / p[:, 2]
            v = (p @ Q[4:7] + Q[7]) / p[:, 2]
            x, y, zs = t[0] * u + t[1] * v + t[2], t[3] * u + t[4] * v + t[5], p[:, 2] * s
            for name, hit in (("x <= -1", x <= -1), ("-1 < x < 0", (x > -1) & (x < 0)), ("x inside", (x >= 0) & (x < out_w)), ("x >= out_w", x >= out_w),
                              ("y <= -1", y <= -1), ("-1 < y < 0", (y > -1) & (y < 0)), ("y inside", (y >= 0) & (y < out_h)), ("y >= out_h", y >= out_h),
                              ("z < min", zs < C.MIN_DEPTH), ("z > max", zs > C.MAX_DEPTH), ("z between", (zs >= C.MIN_DEPTH) & (zs <= C.MAX_DEPTH))):
                seen[flip, name] = seen.get((flip, name), 0) + int(hit.sum())
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "label3d_pin.npz"))
    a = ap.parse_args()
    for kind in C.KINDS:
        seen = coverage(kind)
        print(kind, {f"{'mirrored ' if f else ''}{n}": c for (f, n), c in seen.items()})
        assert all(seen.values()), f"{kind}: a filter arm without a line"
    lanes = C.wave_lanes(64, 1)
    assert any(n0 == 64 for n0, _ in lanes) and any(n1 == 64 for _, n1 in lanes), "max_objs = 64 must fill both waves in some image"
    out = C.run("cuda")
    for kind in C.KINDS:
        counts = out[f"{kind}/counts"].reshape(len(C.ENCODER_RUNS), len(C.COUNTS))
        print(kind, "survivors per image:", {str(r): c.tolist() for r, c in zip(C.ENCODER_RUNS, counts)})
        assert all(c.sum() >= (20 if r[0] > 1 else 2) for r, c in zip(C.ENCODER_RUNS, counts)), f"{kind}: a run with too few survivors"
    out["inputs_sha256"] = np.array(C.inputs_digest())
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {len(out)} arrays, {os.path.getsize(a.out)} bytes, inputs {out['inputs_sha256']}")
    assert os.path.getsize(a.out) < 100_000, "thin the cases: the pin is meant to stay under 100 KB"


if __name__ == "__main__":
    main()
