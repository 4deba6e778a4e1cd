"""GPU: the 3D label encoders (csrc/kitti_labels.hip, csrc/json3d_labels.hip) and plan kernels (csrc/kitti_cache.hip,
csrc/json3d_cache.hip) held to recorded bytes.  tests/golden/label3d_pin.npz holds what the build before the kernels were given
their shared frame (csrc/label3d.h) wrote for the inputs of tests/label3d_pin_cases.py; every output array of every call must be equal
to it in dtype, shape and bit pattern (-0.0 is not 0.0 here).  The parity tests of these kernels compare against the reference within
1e-6; this one is the check that a change which only moves arithmetic has moved nothing."""
import os

import numpy as np
import pytest

import label3d_pin_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label3d_pin.npz")
KEYS = [f"{kind}/{k}" for kind in C.KINDS for k in C.LABEL_KEYS] + [f"plan/{k}" for k in C.PLAN_KEYS]


@pytest.fixture(scope="module")
def pinned():
    z = np.load(GOLDEN)
    assert C.inputs_digest() == str(z["inputs_sha256"]), "the generator of label3d_pin_cases.py drifted: the inputs are not the recorded ones"
    return z, C.run("cuda")


def test_the_pin_lists_these_calls(pinned):
    z, got = pinned
    assert sorted(got) == sorted(k for k in z.files if k != "inputs_sha256") == sorted(KEYS)
    assert os.path.getsize(GOLDEN) < 100_000
    rows = sum(len(C.COUNTS) * r[0] for r in C.ENCODER_RUNS)
    assert all(got[f"{kind}/cls"].shape == (rows, 1) and got[f"{kind}/counts"].shape == (len(C.COUNTS) * len(C.ENCODER_RUNS),) for kind in C.KINDS)
    assert got["plan/img_f"].shape == (C.PLAN_B * len(C.PLAN_RUNS), 19)
    # the cases the pin is there for: lane 63 of either wave live at max_objs = 64, the clipped partner (n1 = 10) at 50, one lane at 1
    full = [lanes for m, _, _, p in C.ENCODER_RUNS if m == 64 and p for lanes in C.wave_lanes(m, p)]
    assert any(n0 == 64 for n0, _ in full) and any(n1 == 64 for _, n1 in full)
    assert C.wave_lanes(50, 1)[5] == (40, 10) and C.wave_lanes(1, 1)[0] == (0, 1) and C.wave_lanes(1, 1)[1] == (1, 0)


@pytest.mark.parametrize("key", KEYS)
def test_every_output_byte_is_the_recorded_one(pinned, key):
    z, got = pinned
    g, w = got[key], z[key]
    assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1)).any(1))
        raise AssertionError(f"{key}: {len(bad)} rows differ, the first in the run with {C.run_of(key, int(bad[0]))}: got {g[bad[0]]}, recorded {w[bad[0]]}")
    assert np.array_equal(g, w)
