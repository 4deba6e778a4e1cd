"""CPU: the NumPy restatement of the reference's hierarchical task learning weights (tests/htl_ref.py) against the reference's own outputs
(tests/golden/htl.npz, minted by tools/make_golden_htl.py from utils/htl.py), and the edges the sequences were built to reach.

`htl_ref.d_ref`, computed here - the largest distance between the fixture (the reference in float32) and the float64 restatement over the entries finite in both -
is what the reference's own rounding amounts to; tests/test_hip_htl.py derives the device bound from it, 4 x max(d_ref, 6 x 2^-23)."""
import numpy as np
import pytest

import htl_ref as H


@pytest.fixture(scope="module")
def golden():
    return H.load_golden()


@pytest.mark.parametrize("name", list(H.SEQUENCES))
def test_fixture_holds_the_sequences_of_this_file(golden, name):
    epochs, losses = H.SEQUENCES[name]
    n = H.RECORDED[name]
    assert np.array_equal(golden[name]["epochs"], np.asarray(epochs[:n])) and np.array_equal(golden[name]["losses"], losses[:n])
    assert golden[name]["weights"].shape == (n, 12) and golden[name]["weights"].dtype == np.float32


@pytest.mark.parametrize("name", list(H.SEQUENCES))
def test_float32_restatement_against_the_reference(golden, name):
    epochs, losses = H.SEQUENCES[name]
    n = H.RECORDED[name]
    w32, _ = H.run(epochs[:n], losses[:n], np.float32)
    gw = golden[name]["weights"]
    assert w32.dtype == np.float32
    ex = H.exact_rows(name)
    for r in range(n):
        assert np.array_equal(np.isnan(w32[r]), np.isnan(gw[r])), f"{name} call {r}: NaN pattern {w32[r]} vs {gw[r]}"
        fin = ~np.isnan(gw[r])
        d = float(np.abs(w32[r][fin].astype(np.float64) - gw[r][fin]).max())
        print(f"{name} call {r} (epoch {epochs[r]}): distance {d:.3e}")
        if r in ex:
            assert np.array_equal(w32[r], gw[r], equal_nan=True), f"{name} call {r}: {w32[r]} vs {gw[r]}"
        assert d <= H.F32_BOUND, f"{name} call {r}: {d:.3e} > {H.F32_BOUND:.3e}"
    first = [1.5, 1.5, 0, 0, 0, 0] * 2
    for r in range(min(n, 6)):
        assert gw[r].tolist() == first, f"{name}: the reference gives exactly [1.5, 1.5, 0, 0, 0, 0] x 2 up to epoch 5"


def test_d_ref_is_a_rounding_distance(golden):
    d = H.d_ref(golden)
    print(f"d_ref = {d:.3e}; device bound 4 * max(d_ref, 6 * 2^-23) = {4 * max(d, 6 * 2.0 ** -23):.3e}")
    assert 0 < d < 16 * 6 * 2.0 ** -24, "fixture and float64 restatement further apart than float32 rounding of weights up to 6 explains"


def test_sequences_reach_their_edges(golden):
    mids = {n: H.run(e, l, np.float32) for n, (e, l) in H.SEQUENCES.items()}
    # 3D weights first leave 0 at epoch 6
    w, _ = mids["decay"]
    assert (w[:6, 2:6] == 0).all() and (w[6:, 2:6] > 0).all() and (w[6:, 8:12] > 0).all()
    assert H.SEQUENCES["decay"][0][-1] >= 200 and np.array_equal(w[-1], np.full(12, 0.5, np.float32))  # time_value clamped at 1
    # a rising predecessor: the ratio is negative and clipped, c = 1, the exponent exactly 0
    w, m = mids["rising"]
    assert m[6]["ratio"][0] < 0 and m[6]["c"][0] == 1 and m[6]["expo"][3] == 0 and m[6]["tv"] > 0
    # both predecessors of depth above 2: two c below -1, a negative exponent, inf at time_value 0
    w, m = mids["restart_inf"]
    assert m[6]["tv"] == 0 and m[6]["c"][0] < -1 and m[6]["c"][4] < -1 and m[6]["expo"][2] < 0 and m[6]["expo"][3] > 1
    assert np.isnan(w[6][2]) and (np.delete(w[6], 2) == 0).all(), "inf / inf for depth, finite / inf for the others"
    assert np.isnan(golden["restart_inf"]["weights"][6][2])
    assert m[7]["expo"][2] < 0 and np.isfinite(w[7:]).all() and w[7][2] > 5.99
    # 0 ** 0 = 1
    w, m = mids["restart_one"]
    assert m[6]["tv"] == 0 and (m[6]["expo"][9:12] == 0).all() and m[6]["ratio"][6] < 0
    want = np.float32(1) / np.float32(7) * np.float32(6)
    assert (w[6][[0, 1, 6, 7, 9, 10, 11]] == want).all() and (w[6][[2, 3, 4, 5, 8]] == 0).all()
    assert np.array_equal(golden["restart_one"]["weights"][6], w[6])
    # a constant predecessor: 0 / 0 at epoch 5, one call past what the fixture holds
    w, m = mids["constant"]
    assert H.RECORDED["constant"] == 5 and len(w) == 6 and np.isfinite(w[:5]).all()
    assert np.isnan(m[5]["ratio"][0]) and np.isnan(w[5]).all(), "the NaN weight of dep/o3d/s3d/hd_om makes the sum, and with it every weight, NaN"
    for dt in (np.float32, np.float64):
        assert np.isnan(H.run(*H.SEQUENCES["constant"], dt)[0][5]).all()
