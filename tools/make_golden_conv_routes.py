"""Mints tests/golden/conv_routes.npz: what the library's host-side conv dispatch answers for a table of geometries.

    python tools/make_golden_conv_routes.py        # needs the built library; no GPU (pure host code)

The table pins `y3d_conv2d_route`, `y3d_conv2d_stat_rows` (forward cases the route accepts) and `y3d_conv2d_wgrad_plan` (weight-gradient
cases the route accepts), so that a change to the dispatch code that is meant to keep every kernel choice and every buffer size can be
checked against the answers from before it.  Regenerate it ONLY with a change that is meant to move a route, and say so there.

Cases: both dtypes x (forward with each of the five epilogues, data gradient, weight gradient) x the maps the models use and ragged
ones x channel pairs around every threshold of the `*_ok` functions and `tile_height` x groups 1 / 16 x five filter geometries, each
under the default knobs, `set_tile_kernels(0)` and `set_stream1x1(0)`.  The full product has 200 k cases: every pair with Cin == Cout
is kept, the other pairs are thinned by a CRC of the case (deterministic), which keeps the file well below the size limit.
"""
from __future__ import annotations

import itertools
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_routes.npz")

FWD, DGRAD, WGRAD = 0, 1, 2
NONE = -(1 << 30)  # "not recorded" (the route refused the case, or the query does not apply to the op)
KEEP_1_IN = 14     # thinning of the Cin != Cout pairs

# (B, H, W)
MAPS = [(b, s, s) for s in (160, 80, 40, 20) for b in (32, 4)] + [(32, 48, 160), (32, 12, 40), (1600, 5, 5), (32, 640, 640), (4, 24, 6)]
CHANNELS = (8, 16, 32, 40, 64, 80, 96, 128, 192, 256, 512, 640)
PAIRS = list(itertools.product(CHANNELS, CHANNELS)) + [(12, 12), (12, 16), (16, 12), (1152, 1152), (192, 1152), (1152, 192), (64, 1152)]
KSP = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0), (7, 1, 3)]
OPS = [(FWD, e) for e in range(5)] + [(DGRAD, 0), (WGRAD, 0)]
KNOBS = (0, 1, 2)  # default, set_tile_kernels(0), set_stream1x1(0)


def cases():
    out = []
    for dt, (op, epi), (B, H, W), (ci, co), g, (k, s, p) in itertools.product((0, 1), OPS, MAPS, PAIRS, (1, 16), KSP):
        if g > 1 and (ci % g or co % g):
            continue
        c = (dt, op, epi, B, H, W, ci, co, g, k, k, s, p)
        if ci != co and zlib.crc32(repr(c).encode()) % KEEP_1_IN:
            continue
        out.append(c)
    return out


def answers(L, cs):
    """-> int32 arrays (route, stat_rows, wgrad_plan) for the cases, under the knobs as they are set"""
    route = np.full(len(cs), NONE, np.int32)
    rows = np.full(len(cs), NONE, np.int32)
    plan = np.full(len(cs), NONE, np.int32)
    for i, c in enumerate(cs):
        dt, op, epi = (int(v) for v in c[:3])
        geo = [int(v) for v in c[3:]]
        route[i] = L.conv2d_route(dt, op, epi, *geo)
        if route[i] >= 0 and op == FWD:
            rows[i] = L.conv2d_stat_rows(dt, *geo)
        if route[i] >= 0 and op == WGRAD:
            plan[i] = L.conv2d_wgrad_plan(dt, *geo)
    return route, rows, plan


def with_knob(L, knob, fn):
    setter = {0: None, 1: L.set_tile_kernels, 2: L.set_stream1x1}[knob]
    old = setter(0) if setter else None
    try:
        return fn()
    finally:
        if setter:
            setter(old)


def main():
    import yolov10_3d_amd as y3d
    L = y3d.lib()
    cs = cases()
    arr = np.asarray(cs, np.int32)
    out = {"cases": arr}
    for knob in KNOBS:
        route, rows, plan = with_knob(L, knob, lambda: answers(L, cs))
        out[f"route/{knob}"], out[f"stat_rows/{knob}"], out[f"wgrad_plan/{knob}"] = route, rows, plan
    np.savez_compressed(OUT, **out)
    r0 = np.concatenate([out[f"route/{k}"] for k in KNOBS])
    print(f"{OUT}: {len(cs)} cases x {len(KNOBS)} knob settings, {os.path.getsize(OUT)} bytes; routes reached "
          f"{sorted(set(int(v) for v in r0 if v >= 0))}, {int((r0 < 0).sum())} refusals")


if __name__ == "__main__":
    main()
