"""CPU: the conv dispatch answers what tests/golden/conv_routes.npz recorded (tools/make_golden_conv_routes.py): the kernel choice of
`y3d_conv2d_route`, the BatchNorm partial rows of `y3d_conv2d_stat_rows` and the split count of `y3d_conv2d_wgrad_plan`, for 37 674
geometries under the default knobs, `set_tile_kernels(0)` and `set_stream1x1(0)`.  All three are pure host code (conv_route in
csrc/conv_gemm.hip and the `*_ok` / `*_rows` / `*_splits` functions next to each kernel), so a change there that is meant to move no
route - splitting the dispatch out of conv_gemm.hip, for one - leaves every row equal."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import yolov10_3d_amd as y3d
from test_abi import route_codes

FWD, WGRAD = 0, 2
NONE = -(1 << 30)


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(GOLDEN, "conv_routes.npz"))
    return {k: z[k] for k in z.files}


def test_table_reaches_every_route_and_holds_refusals(table):
    routes = np.concatenate([table[f"route/{k}"] for k in range(3)])
    codes = route_codes()
    assert len(codes) == 13
    assert set(codes.values()) <= set(int(v) for v in routes), f"routes not reached: {set(codes.values()) - set(int(v) for v in routes)}"
    assert int((routes < 0).sum()) > 0 and int((routes >= 0).sum()) > 0
    # every accepted forward / weight-gradient case carries its derived size
    ops = np.tile(table["cases"][:, 1], 3)
    rows = np.concatenate([table[f"stat_rows/{k}"] for k in range(3)])
    plan = np.concatenate([table[f"wgrad_plan/{k}"] for k in range(3)])
    assert ((rows != NONE) == ((routes >= 0) & (ops == FWD))).all()
    assert ((plan != NONE) == ((routes >= 0) & (ops == WGRAD))).all()


@pytest.mark.parametrize("knob", [0, 1, 2], ids=["default", "tile_kernels_off", "stream1x1_off"])
def test_dispatch_answers_the_recorded_table(table, knob):
    L = y3d.lib()
    cases = table["cases"].tolist()
    want_route, want_rows, want_plan = (table[f"{n}/{knob}"].tolist() for n in ("route", "stat_rows", "wgrad_plan"))
    setter = {0: None, 1: L.set_tile_kernels, 2: L.set_stream1x1}[knob]
    old = setter(0) if setter else None
    bad = []
    try:
        for c, wr, ws, wp in zip(cases, want_route, want_rows, want_plan):
            got = L.conv2d_route(*c)
            geo = [c[0]] + c[3:]
            rows = L.conv2d_stat_rows(*geo) if ws != NONE else NONE
            plan = L.conv2d_wgrad_plan(*geo) if wp != NONE else NONE
            if (got, rows, plan) != (wr, ws, wp):
                bad.append((c, (got, rows, plan), (wr, ws, wp)))
    finally:
        if setter:
            setter(old)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ (case, got, recorded): {bad[:8]}"
