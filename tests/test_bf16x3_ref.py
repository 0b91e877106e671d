"""The CPU twin of the "bf16x3" product (tests/bf16x3_ref.py) against the bound tests/test_hip_bf16x3.py holds the kernels to.

(a) the twin meets c = C_BF16X3 (split=False: bf16 keeps fp32's exponent range) on every input pattern of the GPU tests;
(b) three wrong products -- pair (1, 1) dropped, pairs (0, 2) and (2, 0) dropped, two planes only -- each miss it on at least
    one of those patterns: the bound would notice a kernel that lost a term pair;
(c) in the integer cases of the row-geometry test every dropped pair is exactly zero and every kept product and partial sum
    exact in fp32: the kernel has no freedom left, so bit equality is the right comparison."""
import numpy as np
import pytest

import bf16x3_ref as B
import f64_bounds as fb

Q_PRE = ("network1.", "network2.")


def layer2_cases():
    """(name, h1 fp32 [rows, 256], W2 fp32 [256, 256] (in, out), b2) of every layer-2 GEMM the GPU forward tests run."""
    from test_hip_f16_scaling import FWD_PATTERNS, DYN_PATTERNS, dyn_params_nobias, rows_pattern
    out = []
    for pattern in FWD_PATTERNS + ["coherent"]:
        pa, pq, s, a = B.forward_case(pattern)
        x = np.concatenate([s, a], 1)
        for p, pre, inp in ((pq, Q_PRE[0], x), (pq, Q_PRE[1], x), (pa, "network.", s)):
            out.append((f"{pattern} {pre}", B.h1_fp32(p, pre, inp), p[pre + "network.2.weight"].T, p[pre + "network.2.bias"]))
    pa, pq = B.wide_q_params()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal((96, B.S)), rng.uniform(-1, 1, (96, B.A))], 1).astype(np.float32)
    for pre in Q_PRE:
        out.append((f"wide W2 {pre}", B.h1_fp32(pq, pre, x), pq[pre + "network.2.weight"].T, pq[pre + "network.2.bias"]))
    for S_, A_ in ((17, 6), (45, 24)):
        p = dyn_params_nobias(31, S_, A_)
        for pattern in DYN_PATTERNS:
            rng = np.random.default_rng(7 + len(pattern))
            rows, f, _ = rows_pattern(pattern, rng)
            if pattern == "tile_scales":
                f = np.repeat(2.0 ** np.arange(-40, 21, 20), 32); rows = f.size
            obs = (rng.standard_normal((rows, S_)) * f[:, None]).astype(np.float32)
            z = (obs.astype(np.float64) @ p["zs1.weight"][0].astype(np.float64) + p["zs1.bias"][0]).astype(np.float32)
            with np.errstate(over="ignore"):
                h = (z / (1 + np.exp(-z.astype(np.float64)))).astype(np.float32)
            out.append((f"dyn S{S_} {pattern} zs2", h, p["zs2.weight"][0], p["zs2.bias"][0, 0]))
    return out


@pytest.fixture(scope="module")
def cases():
    return layer2_cases()


def worst(got, ref, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == ref, 0.0, np.inf))
    return float(np.max(r))


def test_split_is_round_to_nearest_even_and_lossless():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.0e38, 1e-30,
                  np.inf, -np.inf], np.float32)
    t0 = B.bf16_rne(x)
    assert t0[0] == 1.0 and t0[1] == 1.0 and t0[2] == 1.0 + 2.0 ** -6 and t0[3] == -1.0 and t0[4] == 1.0 + 2.0 ** -7   # ties to even
    assert np.isfinite(t0[5]) and t0[6] > 0
    assert t0[7] == np.inf and t0[8] == -np.inf and np.isnan(B.bf16_rne(np.float32(np.nan)))
    assert not (B.bf16_rne(x).view(np.uint32) & 0xFFFF).any()
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(4096) * 2.0 ** rng.integers(-60, 60, 4096)).astype(np.float32)
    t = B.split3(v).astype(np.float64)
    assert np.array_equal(t.sum(0), v.astype(np.float64))                     # 8 + 8 + 8 bits hold an fp32 significand
    assert (np.abs(t[1]) <= 2.0 ** -8 * np.abs(t[0])).all() and (np.abs(t[2]) <= 2.0 ** -16 * np.abs(t[0])).all()


def test_twin_meets_the_bound_on_every_pattern(cases):
    for name, h1, W2, b2 in cases:
        fin = np.isfinite(h1).all(1)
        ref, bnd = fb.layer_bound(h1[fin], W2, b2, fb.C_BF16X3, split=False)
        got = B.gemm(h1[fin], W2) + b2.astype(np.float64)
        r = worst(got, ref, bnd)
        print(f"{name}: twin err / bound = {r:.3g}")
        assert r <= 1.0, name


@pytest.mark.parametrize("mutant", sorted(B.MUTANTS))
def test_bound_rejects_a_product_that_lost_term_pairs(mutant, cases):
    ratios = {}
    for name, h1, W2, b2 in cases:
        fin = np.isfinite(h1).all(1)
        ref, bnd = fb.layer_bound(h1[fin], W2, b2, fb.C_BF16X3, split=False)
        ratios[name] = worst(B.gemm(h1[fin], W2, B.MUTANTS[mutant]) + b2.astype(np.float64), ref, bnd)
    rejected = [n for n, r in ratios.items() if r > 1.0]
    print(mutant, "rejected on", rejected, "worst", max(ratios.values()))
    assert any(n.startswith("coherent") for n in rejected), ratios


@pytest.mark.parametrize("N", B.WGRAD_ROWS)
def test_integer_critic_cases_leave_the_kernel_no_freedom(N):
    """Every bf16x3 GEMM of the critic step on int_critic_case((17, 6), N): layer 2 of Q(s, a), of the target Q(s2, pi = 0) and
    of the actor at s2, the backward dz2 W2^T and the weight gradient h1^T dz2."""
    from test_hip_twinq_rank1 import int_critic_case
    B.assert_critic_case_exact(int_critic_case((B.S, B.A), N), f"N{N}")
