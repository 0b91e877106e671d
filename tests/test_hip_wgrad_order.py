"""The summation order of the weight-gradient launches, bit for bit (csrc/mlp_bwd.hip k_wgrad*, k_grad_reduce).

1. test_wgrad_order: mobody_mlp3_backward (exact fp32: k_wgrad) on the inputs of tests/wgrad_order_ref.py -- every product
   exact, every partial sum rounding -- must `torch.equal` the NumPy emulation of the documented order for dW1 and dW3; the
   padding entries must be exactly 0 and every entry written (NaN sentinels in the gradient blob and the workspace:
   test_hip_aux_grad.run_backward).  Which wave or workgroup computes which columns, and which instruction forms the chain,
   is free; the order is not: a form that splits a wave's rows differently, pairs the waves differently or adds the slabs
   in another order fails here (tests/test_wgrad_order_ref.py: reversing the rows alone changes four elements in five).
   Row counts: the split-K geometries 1 .. 283, 513 (twin) and 1025 (7 members), plus those that leave a last wave of
   depth - 1, depth, depth + 1 rows around one, two, three and four blocks of 8 and of 16 rows (7, 8, 9; 15, 16, 17; 23, 24,
   25; 31, 32, 33) and odd and even block counts behind them (47, 48, 49; 63) -- the row loop of wgrad_tile takes 8-row
   blocks; the 16- and 12-row cases are there for a form that changes the block.
2. test_critic_f16_dispatch: the integer-exact critic cases of tests/test_hip_twinq_rank1.py through the gradient form of
   mobody_critic in both MFMA modes (f16x2: k_wgrad_f16) at row counts up to 1025 -- bit for bit the integer closed form.
"""
import numpy as np
import pytest
import torch

import aux_ref as R
import wgrad_order_ref as WO
from test_hip_aux_grad import run_backward
from test_hip_twinq_rank1 import int_critic_case, run_critic, same_bits

pytestmark = pytest.mark.gpu

KINDS = {  # (in_dim, out_dim, members)
    "twin_q": (23, 1, 2), "v": (17, 1, 1), "cls_sa": (23, 2, 1), "actor_A6": (17, 6, 1), "actor_A24": (45, 24, 1),
    "actor_A3": (11, 3, 1), "mopo": (23, 17, 7)}
ROWS = [1, 7, 8, 9, 16, 17, 33, 65, 257, 283]
# one member, nsplit 1: rows = 3 rows_per_wave + n puts n rows in the last wave (rows_per_wave 32: 97 .. 128, 48: 145 .. 192,
# 64: 193 .. 255)
BRANCH_ROWS = [96 + n for n in (7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32)] + [144 + n for n in (33, 47, 48)] + [192 + n for n in (49, 63)]
EXTRA = {"twin_q": [513], "mopo": [1025]}
CASES = [(k, r) for k in KINDS for r in ROWS + BRANCH_ROWS + EXTRA.get(k, [])]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_branch_rows_hit_the_blocks_they_name():
    for n in (7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32):
        assert R.wgrad_geometry(96 + n, 1)["waves"][:4] == [(32, 4, 0)] * 3 + [(n, n // 8, n % 8)]
    for n in (33, 47, 48):
        assert R.wgrad_geometry(144 + n, 1)["waves"][3][0] == n and R.wgrad_geometry(144 + n, 1)["rows_per_wave"] == 48
    for n in (49, 63):
        assert R.wgrad_geometry(192 + n, 1)["waves"][3][0] == n and R.wgrad_geometry(192 + n, 1)["rows_per_wave"] == 64


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-rows{c[1]}")
def test_wgrad_order(case, dev):
    kind, rows = case
    in_dim, out_dim, members = KINDS[kind]
    c = WO.order_case(1000 + 7 * rows + in_dim, in_dim, out_dim, members, rows)
    assert WO.products_exact(c)
    want = WO.emulate(c)
    g, dz2, dz1 = run_backward(c, in_dim, out_dim, members, dev)       # asserts: every entry written, padding exactly 0
    assert np.array_equal(dz2, c["dz2"]) and np.array_equal(dz1, c["dz1"]), "the backward's dz2 / dz1 are not the exact copies"
    for m in range(members):
        for k, pk in (("dW1", "network.0.weight"), ("dW3", "network.4.weight")):
            got, ref = torch.from_numpy(np.ascontiguousarray(g[m][pk])), torch.from_numpy(np.ascontiguousarray(want[k][m]))
            assert got.shape == ref.shape
            if not torch.equal(got, ref):
                bad = (got != ref)
                i = tuple(int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{kind} rows {rows} member {m} {k}: {int(bad.sum())} of {bad.numel()} elements differ from the "
                                     f"documented order; first {i}: got {float(got[i])!r} want {float(ref[i])!r}")


@pytest.mark.parametrize("N", (1, 7, 9, 17, 33, 65, 257, 513, 769, 1025))
def test_critic_f16_dispatch(N, mfma, dev):
    S, A = 17, 6
    c = int_critic_case((S, A), N)
    _, g, loss, _ = run_critic(c["pa"], c["pq"], c["batch"], S, A, N, c["Ng"], mfma, dev)
    for m in range(2):
        for k, v in c["out"][m]["grads"].items():
            same_bits(g[m][k], v, f"N{N} {mfma} member {m} {k}")
    same_bits([loss], [c["loss"]], "q_loss")
