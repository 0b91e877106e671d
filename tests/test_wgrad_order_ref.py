"""The NumPy emulation of the weight-gradient summation order (tests/wgrad_order_ref.py), checked without a GPU: its inputs
make every product exact (asserted from the inputs alone), its result depends on the row order (so a kernel that sums in
another order cannot match it by accident), and in fp64 it is the plain contraction."""
import numpy as np
import pytest

import aux_ref as R
import wgrad_order_ref as WO

CASES = [("v", 17, 1, 1, 257), ("actor", 17, 6, 1, 283), ("twin_q", 23, 1, 2, 513), ("mopo", 23, 17, 7, 1025)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-rows{c[4]}")
def case(request):
    kind, in_dim, out_dim, members, rows = request.param
    c = WO.order_case(11 + rows, in_dim, out_dim, members, rows)
    return c, WO.emulate(c), (in_dim, out_dim, members, rows)


def test_products_are_exact(case):
    c, _, _ = case
    for k in ("x", "dz3", "h1", "h2", "dz2", "dz1"):
        assert WO.significand_bits(c[k]) <= 11, k
    assert WO.products_exact(c)
    # a 12-bit operand breaks the precondition, and the check sees it
    bad = dict(c, x=c["x"] * np.float32(1 + 2.0 ** -11))
    assert not WO.products_exact(bad)


def test_backward_operands_are_exact_copies(case):
    """dz2 / dz1 as order_case states them are what the fp64 backward gives: the kernel's GEMMs have one non-zero term."""
    c, _, _ = case
    ref = R.mlp3_backward_ref(c["W1"], c["W2"], c["W3"], c["x"], c["h1"], c["h2"], c["dz3"])
    assert np.array_equal(ref["dz2"], c["dz2"].astype(np.float64)) and np.array_equal(ref["dz1"], c["dz1"].astype(np.float64))
    assert np.count_nonzero(c["dz1"]) > 0.7 * c["dz1"].size


def test_emulation_is_the_contraction_and_rounds(case):
    c, emu, _ = case
    ref = R.mlp3_backward_ref(c["W1"], c["W2"], c["W3"], c["x"], c["h1"], c["h2"], c["dz3"])
    for k in ("dW1", "dW3"):
        err = np.abs(emu[k] - ref[k])
        bound = (c["x"].shape[0] + 8) * 2.0 ** -24 * ref["abs_" + k]
        assert (err <= bound).all(), k
        assert (emu[k].astype(np.float64) != ref[k]).mean() > 0.5, f"{k}: the partial sums do not round"


def test_result_depends_on_the_row_order(case):
    c, emu, _ = case
    rev = WO.emulate(c, reverse=True)
    for k in ("dW1", "dW3"):
        changed = (emu[k].view(np.int32) != rev[k].view(np.int32)).mean()
        print(k, "fraction of elements whose bits change with the row order reversed: %.3f" % changed)
        assert changed >= 0.5, (k, changed)


def test_geometry_is_the_launch_geometry():
    """ordered_sum walks the wave slices aux_ref.wgrad_geometry lists (rows_per_wave whole 16-row blocks, 4 waves a slice)."""
    for rows, members in ((1, 1), (65, 1), (257, 1), (513, 2), (1025, 7)):
        geo = R.wgrad_geometry(rows, members)
        got = [max(0, min(rows, (g + 1) * geo["rows_per_wave"]) - min(rows, g * geo["rows_per_wave"])) for g in range(4 * geo["nsplit"])]
        assert got == [w[0] for w in geo["waves"]] and sum(got) == rows
