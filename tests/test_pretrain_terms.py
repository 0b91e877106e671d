"""The per-term fp64 references of tests/pretrain_terms.py, and proof that their acceptance rule has teeth -- on the CPU,
before tests/test_hip_pretrain_terms.py holds csrc/pretrain.hip to it.

Each mutant swaps ONE expression of the loss (a wrong divisor, a dropped chain-rule term, a wrong sample).  The rule has to
reject it by more than 4x in the term the table names.  The dropped chain-rule term through std_e(mean6) passes the
summed-loss tolerance the suite had so far (1e-5 of the sub-network's largest gradient, source step); the KL and
biased-std mutants turned out not to (pretrain_terms.OLD_TOLERANCE_SEES), so no such claim is asserted for them.
"""
import numpy as np
import pytest
import torch

import pretrain_terms as PT

CASES = [(g, t) for g in PT.GEOMETRIES for t in PT.TERMS]


@pytest.mark.parametrize("geom,term", CASES, ids=[f"S{g[0]}A{g[1]}b{g[2]}-{t}" for g, t in CASES])
def test_reference_is_usable(geom, term):
    """fp64 gradients finite; every tensor the term reaches is non-zero, every other one None or zero; the fp32 restatement
    passes the rule; the ensemble std of mean6 stays above 1e-3 |mean6| (no case rests on 0 / 0)."""
    S, A, b = geom
    for use_trg in (False, True):
        l64, g64, g32 = PT.reference(S, A, b, term, use_trg)
        assert np.isfinite(l64).all()
        live = {n + sfx for n in PT.expected_nonzero(term, use_trg) for sfx in (".weight", ".bias")}
        other = ("za_src" if use_trg else "za_trg")
        for k, g in g64.items():
            if k in live:
                assert g is not None and np.isfinite(g).all() and np.any(PT.blob_view(k, g)), (k, use_trg)
            elif PT.judged(term, k):
                assert PT.is_zero(g), (k, use_trg)
            if k.startswith(other):
                assert g is None, (k, use_trg)
            if g is not None and PT.judged(term, k):
                v32 = PT.blob_view(k, g32[k])
                assert PT.rule_ratio(v32, PT.blob_view(k, g), v32) <= 1.0 / 3, (k, use_trg)
        mean6, std = PT.fake_std(S, A, b, term, use_trg)
        assert (std > 1e-3 * mean6.abs()).all()


@pytest.mark.parametrize("use_trg", [False, True])
def test_unmutated_restatement_equals_the_oracle(use_trg):
    """mutated_losses with nothing swapped IS oracle.dyn_learn_losses: same losses and gradients bit for bit."""
    p, rows, noise = PT.case_inputs(5, 8, 23, "all")
    for dtype in (torch.float32, torch.float64):
        la, ga = PT.term_grads(p, rows, noise, use_trg, (1.0, 1.0, 1.0), dtype)
        lb, gb = PT.term_grads(p, rows, noise, use_trg, (1.0, 1.0, 1.0), dtype, mutate="none")
        assert np.array_equal(la, lb)
        for k in ga:
            assert (ga[k] is None and gb[k] is None) or np.array_equal(ga[k], gb[k]), k


def test_local_share_scales_by_b_over_b_global():
    l, g, _ = PT.reference(17, 6, 12, "all", True)
    lh, gh, _ = PT.reference(17, 6, 12, "all", True, 24)
    assert np.array_equal(lh, 0.5 * l) and all(np.array_equal(gh[k], 0.5 * g[k]) for k in g if g[k] is not None)


def _mutant_ratios(name):
    term, (S, A, b), use_trg = PT.MUTANTS[name]
    p, rows, noise = PT.case_inputs(S, A, b, term)
    _, g64, g32 = PT.reference(S, A, b, term, use_trg)
    _, gm = PT.term_grads(p, rows, noise, use_trg, PT.TERMS[term], torch.float32, mutate=name)
    out = {}
    for k, ref in g64.items():
        if PT.judged(term, k) and not PT.is_zero(ref):
            out[k] = PT.rule_ratio(PT.blob_view(k, gm[k]), PT.blob_view(k, ref), PT.blob_view(k, g32[k]))
    return out


@pytest.mark.parametrize("name", list(PT.MUTANTS))
def test_rule_rejects_mutant(name):
    ratios = _mutant_ratios(name)
    worst = max(ratios, key=ratios.get)
    print(f"{name}: worst {worst} err / bound = {ratios[worst]:.3g}")
    assert ratios[worst] > 4.0, ratios


@pytest.mark.parametrize("name", PT.OLD_TOLERANCE_BLIND + PT.OLD_TOLERANCE_SEES)
def test_summed_loss_tolerance_on_mutant(name):
    """What test_pretrain_grads_vs_oracle_shapes asserts (full loss, source step, fp32 oracle, sub-network scale) does not see
    the OLD_TOLERANCE_BLIND mutants (reward_src_factor_in_trg does not act on a source step at all; on a target step it is 100x
    and is seen).  It does see the others: recorded, so that the table stays true."""
    S, A, b = PT.MUTANTS[name][1]
    p, rows, noise = PT.case_inputs(S, A, b, "all")
    _, want = PT.term_grads(p, rows, noise, False, PT.TERMS["all"], torch.float32)
    _, got = PT.term_grads(p, rows, noise, False, PT.TERMS["all"], torch.float32, mutate=name)
    assert PT.old_tolerance_passes(got, want) == (name in PT.OLD_TOLERANCE_BLIND)
