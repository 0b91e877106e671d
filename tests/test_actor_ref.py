"""The closed forms of tests/actor_ref.py against float64 autograd on the reference's formulation of the actor update
(O.train_step), the sensitivity of the GPU test to one named bug per edge, the fp32 reference arithmetic inside the derived
bounds, and the preconditions and case table of tests/test_hip_actor_fp64.py.  No GPU needed."""
import numpy as np
import pytest
import torch

import actor_ref as AR
import f64_bounds as FB
import golden_util as gu
import test_hip_actor_fp64 as G
from oracle import mobody_oracle as O

RTOL = 1e-12


def actor_step_torch(pa, pq, s, a, h, Nt, Ng, Ntg, dtype, stats=None, v_true=None):
    """update_policy + bc_loss as O.train_step states them (mobody.py:246-276, 314-345), with what the oracle's signature
    cannot express: global row counts and all-reduced stats of a data-parallel rank, a given V(s_true), and Nt = 0
    (L_BC = 0).  Pinned to O.train_step below wherever both can run."""
    s, a = O.T(s, dtype), O.T(a, dtype)
    ap = {k: O.T(v, dtype).clone().requires_grad_(True) for k, v in pa.items()}
    qd = {k: O.T(v, dtype) for k, v in pq.items()}
    A = a.shape[1]
    pi = O.actor(ap, s, h["max_action"])
    b1, b2 = O.twin_q(qd, s, pi)
    qv = torch.min(b1, b2)
    local = [qv.abs().sum().detach()]
    p_w = h["weight"] / ((local[0] if stats is None else stats[0]) / Ng) if h["scale_Q"] else 1.0
    loss = p_w * (-qv).sum() / Ng
    bc = torch.zeros((), dtype=dtype)
    w = torch.ones(0, 1, dtype=dtype)
    local.append(torch.zeros((), dtype=dtype))
    if Nt:
        with torch.no_grad():
            c1, c2 = O.twin_q(qd, s[:Nt], a[:Nt])
            qb = torch.min(c1, c2)
            local[1] = qb.abs().sum()
            adv = qb - O.T(v_true, dtype).reshape(-1, 1) if v_true is not None else qb / ((local[1] if stats is None else stats[1]) / Ntg)
            w = torch.exp(3 * adv).clamp(max=100.0) if h["q_weighted"] else torch.ones_like(qb)
        bc = (w * (pi[:Nt] - a[:Nt]) ** 2).sum() / (Ntg * A)
    loss = loss + h["bc_coef"] * bc
    names = list(ap)
    gs = torch.autograd.grad(loss, [ap[k] for k in names])
    return dict(grads={k: g.numpy() for k, g in zip(names, gs)}, L_pi=float(loss.detach()), L_BC=float(bc.detach()),
                bcw=w.detach().numpy()[:, 0], pi=pi.detach().numpy(), stats=np.array([float(x) for x in local]))


def abs_floor(tape):
    """Two fp64 evaluations of one contraction in different orders differ by ~K 2^-53 of its sum |a||b| (three nested ones)."""
    out = {}
    for i in (0, 2, 4):
        r = tape[f"network.network.{i}"][0]
        out[f"network.network.{i}.weight"] = 3 * 256 * 2.0 ** -53 * (np.abs(r["dz"]).T @ np.abs(r["x"])).max()
        out[f"network.network.{i}.bias"] = 3 * 256 * 2.0 ** -53 * np.abs(r["dz"]).sum(0).max()
    return out


VARIANTS = {"default": {}, "noqw": dict(q_weighted=0), "noscale": dict(scale_Q=0), "adv": dict(advantage=1), "bc0": dict(bc_coef=0.0),
            "bc05": dict(bc_coef=0.5), "ma04": dict(max_action=0.4), "ma2": dict(max_action=2.0)}


@pytest.mark.parametrize("tag", list(VARIANTS))
@pytest.mark.parametrize("S,A,N,Nt", [(17, 6, 37, 19), (11, 3, 64, 64)])
def test_closed_forms_vs_autograd(S, A, N, Nt, tag):
    cfg = gu.policy_cfg(S, A, **VARIANTS[tag])
    pa, pq, pv = gu.policy_params(90 + S, S, A)
    batch = gu.gi.batch(91, N, S, A)
    want = O.train_step(O.TrainState(pa, pq, pv), batch, Nt, cfg, apply=False, dtype=torch.float64)
    s, a = batch[0], batch[1]
    fw = AR.forward_ref(pa, pq, s, a, Nt, cfg["max_action"])
    v_true = None
    if cfg["advantage"]:
        v_true = FB.input_gradient(FB.net_weights(pv, "network."), s[:Nt].astype(np.float64))[0][:, 0]
    cf = AR.closed_forms(fw["pi"], fw["qp"], fw["qb"], fw["dqda"], a, cfg, N, Nt, N, Nt, v_true=v_true)
    grads, tape = AR.actor_grads_ref(pa, s, fw, cf["dz3"])
    close = lambda got, ref, what, atol=0.0: np.testing.assert_allclose(np.asarray(got, np.float64), FB.f64(ref), rtol=RTOL, atol=atol, err_msg=what)
    close(fw["pi"], want["pi"], "pi")
    close(cf["minq"], want["q_pi"][:, 0], "min q")
    close(cf["bcw"], want["bc_w"][:, 0], "bc_w")
    close(cf["L_pi"], want["pi_loss"], "pi_loss")
    close(cf["L_BC"], want["bc_loss"], "bc_loss")
    floor = abs_floor(tape)
    for k, v in want["actor_grads"].items():
        close(grads[k], v, k, atol=floor[k])
    # the restatement with global counts agrees with the oracle too (both precisions of its arithmetic)
    t64 = actor_step_torch(pa, pq, s, a, cfg, Nt, N, Nt, torch.float64, v_true=v_true)
    for k, v in want["actor_grads"].items():
        close(t64["grads"][k], v, "restatement " + k, atol=floor[k])
    close(t64["L_pi"], want["pi_loss"], "restatement pi_loss")
    close(t64["stats"], cf["stats"], "stats")


def test_tie_rule_is_torch_min_backward():
    """Integer nets with tied rows: the 1/2 split is what autograd does with torch.min(q0, q1) at q0 == q1."""
    c = G.EXACT[9]
    p = G.exact_probe(c)
    assert (p["fw"]["qp"][0] == p["fw"]["qp"][1]).sum() >= 5
    exp, ok, _ = AR.int_probe_expected(p)
    t = actor_step_torch(p["pa"], p["pq"], p["s"], p["act"], p["h"], p["Nt"], p["Ng"], p["Ntg"], torch.float64, stats=p["stats_in"],
                         v_true=p["v_true"])
    for k, v in exp["grads"].items():
        assert np.array_equal(t["grads"][k].astype(np.float32), v.astype(np.float32)), k   # (fp64 exp(-192) is 1e-84, fp32's is 0)
    assert np.float32(t["L_pi"]) == np.float32(exp["cf"]["L_pi"]) and np.float32(t["L_BC"]) == np.float32(exp["cf"]["L_BC"])


def test_case_table_of_the_actor_tests():
    G.check_case_table()


@pytest.mark.parametrize("case", G.EXACT, ids=G.exact_id)
def test_exact_probe_preconditions(case):
    (N, Nt), (S, A), gmul, variant = case
    p = G.exact_probe(case)
    exp, ok, detail = AR.int_probe_expected(p)
    assert ok, detail
    assert AR.f16_bits_ok(p, exp), "an operand of an fp16-core GEMM carries more than 11 bits below its tile maximum"
    cf, fw = exp["cf"], p["fw"]
    assert np.log2(abs(cf["p_w"])) % 1 == 0 and p["Ng"] & (p["Ng"] - 1) == 0 and p["Ntg"] & (p["Ntg"] - 1) == 0
    if N >= 31:                                              # tied and untied rows of both orders; dz2 of the actor is not zero
        tie = fw["qp"][0] == fw["qp"][1]
        assert tie.sum() >= 5 and (fw["qp"][0] < fw["qp"][1]).any() and (fw["qp"][0] > fw["qp"][1]).any()
        assert np.abs(fw["dqda"][:, tie]).max() == 1 and np.abs(exp["tape"]["network.network.2"][0]["dz"]).max() > 0
        assert np.abs(exp["grads"]["network.network.0.weight"]).max() > 0
    if Nt >= 31:                                             # all three regions of the clamp
        assert set(np.unique(cf["bcw"])) == {0.0, 1.0, 100.0}
        assert (3 * cf["adv"][cf["bcw"] == 0] <= -104).all() and (3 * cf["adv"][cf["bcw"] == 100] >= AR.LN100).all()


def real_pick(kind, sa, N, gmul=None):
    return next(c for c in AR.REAL_CASES if c[:3] == (kind, sa, N) and gmul in (None, c[3]))


# mutant -> the case whose inputs tell it apart.  An exact probe's bound is 0 (bit equality): any difference is a failure.
# (n_local: N_global cancels between p_w and 1 / N_global unless scale_Q = 0, so it takes a bc_only case.)
_BC2 = next(c for c in AR.REAL_CASES if c[0] == "bc_only" and c[2] == 33 and c[3] == 2)
SENSITIVITY = {"tie_le": ("exact", G.EXACT[9]), "no_clamp": ("real", real_pick("clamp", (11, 3), 257)),
               "clamp_10": ("real", real_pick("clamp", (111, 8), 33)), "bc_all_rows": ("real", real_pick("plain", (11, 3), 33)),
               "nt_local": ("real", _BC2), "n_local": ("real", _BC2),
               "th_no_div": ("real", real_pick("max_action_0.4", (11, 3), 257)),
               "no_max_action": ("real", real_pick("max_action_2", (17, 6), 33)), "bcw_row": ("real", _BC2)}


@pytest.mark.parametrize("mutant", AR.MUTANTS)
def test_each_mutant_is_rejected_at_4x_its_bound(mutant):
    kind, case = SENSITIVITY[mutant]
    if kind == "exact":
        p = G.exact_probe(case)
        stats, bound = p["stats_in"], None
    else:
        assert case in AR.REAL_CASES
        p = AR.real_case(*case)
        stats, bound = p["gmul"] * p["cf"]["stats"], AR.real_bounds(*case, True)          # the wider (f16x2) bound
    fw = p["fw"]
    args = (fw["pi"], fw["qp"], fw["qb"], fw["dqda"], p["act"], p["h"], p["N"], p["Nt"], p["Ng"], p["Ntg"])
    true = AR.closed_forms(*args, stats=stats, v_true=p["v_true"])
    mut = AR.closed_forms(*args, stats=stats, v_true=p["v_true"], mutant=mutant)
    g0, _ = AR.actor_grads_ref(p["pa"], p["s"], fw, true["dz3"])
    g1, _ = AR.actor_grads_ref(p["pa"], p["s"], fw, mut["dz3"])
    if bound is None:
        worst = max(np.abs(g1[k].astype(np.float32) - g0[k].astype(np.float32)).max() for k in g0)
        assert worst > 0
        assert np.abs(mut["dz3"][fw["qp"][0] == fw["qp"][1]][:, np.abs(fw["dqda"][0]).max(0) > 0]).max() > 0     # +-c, not 0
        return
    worst = max(AR.ratios(g1[k], g0[k], bound["grads"][k]) for k in g0)
    print(mutant, "worst |mutant - true| / bound", worst)
    assert worst > 4.0, worst


@pytest.mark.parametrize("case", AR.REAL_CASES, ids=AR.real_id)
def test_fp32_reference_stays_inside_the_bounds(case):
    """The reference's own arithmetic (torch float32) against fp64: err / bound <= 1 for every checked output, with the
    bound of the exact-fp32 mode.  Also the condition on the filter: at most 1/8 of the pool dropped, N robust rows exist."""
    c = AR.real_case(*case)
    assert c["all_robust"] and 8 * c["kept"] >= 7 * c["pool"], (c["kept"], c["pool"])
    bd = AR.real_bounds(*case, False)
    cf = c["cf"]
    s32 = actor_step_torch(c["pa"], c["pq"], c["s"], c["act"], c["h"], c["Nt"], c["Ng"], c["Ntg"], torch.float32, v_true=c["v_true"])
    got = actor_step_torch(c["pa"], c["pq"], c["s"], c["act"], c["h"], c["Nt"], c["Ng"], c["Ntg"], torch.float32,
                           stats=np.float32(c["gmul"]) * s32["stats"].astype(np.float32), v_true=c["v_true"])
    t64 = actor_step_torch(c["pa"], c["pq"], c["s"], c["act"], c["h"], c["Nt"], c["Ng"], c["Ntg"], torch.float64,
                           stats=c["gmul"] * cf["stats"], v_true=c["v_true"])
    out = {}
    for k, v in c["grads"].items():
        np.testing.assert_allclose(t64["grads"][k], v, rtol=1e-9, atol=1e-9 * np.abs(v).max(), err_msg=k)   # same reference
        out[k] = AR.ratios(got["grads"][k], v, bd["grads"][k])
    out["stats"] = AR.ratios(got["stats"], cf["stats"], bd["stats"])
    out["L_pi"] = AR.ratios(got["L_pi"], cf["L_pi"], bd["L_pi"])
    out["L_BC"] = AR.ratios(got["L_BC"], cf["L_BC"], bd["L_BC"])
    print(AR.real_id(case), {k.replace("network.network.", "l"): f"{v:.3g}" for k, v in out.items()})
    assert max(out.values()) <= 1.0, out
    if case[0] == "clamp":                                    # at, just below, far below
        t = 3 * cf["adv"]
        assert (cf["bcw"] == 100).any() and ((cf["bcw"] < 100) & (t > AR.LN100 - 2e-3)).any() and (t < -89).any()
    if case[0] == "saturated":
        z = np.abs(c["fw"]["z3"])
        assert ((z > 5) & (z < 9)).mean() > 0.2
