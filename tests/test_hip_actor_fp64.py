"""The actor half of the training step -- pi(s) with the tanh head, twin Q at (s, pi), k_actor_stats, the frozen-Q backward
with input gradient (BwdSeed mode 2, the DX instances of k_mlp3_bwd), the actor seed (mode 3), the actor backward, the
weight gradients and LossFinal kind 2 -- against the fp64 closed forms of tests/actor_ref.py, per element.

(a) Exact probes.  Integer nets (actor_ref.int_nets): pi = 0 and tanh' = 1 exactly, q0 == q1 on the rows where both members'
    own state units are dead, BC weights 0, 1 and 100 only, every scalar factor a power of two.  Every intermediate is an
    integer or an integer multiple of one power of two with all sums of |terms| below 2^24 of it, so each fp32 summation
    order -- and each fp16 split of the "f16x2" mode, whose precondition (11 bits below the tile maximum) is asserted in
    tests/test_actor_ref.py -- gives the same bits, and the kernels must equal the fp64 closed form rounded once.
    1 / N_global is a power of two only if N_global is: the probes hand N_global = pow2ceil(N) and twice that (Nt_global
    likewise); N_global = N and 2 N at the odd row counts are part (b)'s.  The stats handed to the backward are crafted
    (a data-parallel caller hands its all-reduced sums the same way); the stats actor_forward wrote are compared first.

(b) Real-valued inputs against fp64 with the derived bound of actor_ref.actor_bounds, nothing normalised by a tensor's
    maximum.  Its terms (u = 2^-24; C_E2E, SUBNORMAL of tests/f64_bounds.py):
      E_pi   = max_action tanh'(|z3| - E_z3) E_z3 + 4 u |pi|                  forward error of the stored policy output
      E_q    = forward bound of q + |dq/da| E_pi                              (masks fixed on robust rows)
      stats  : (N + 3) u sum |min q| + sum E_q;  e_s = its relative size
      E_dxa  = C_E2E |dz| |W^T| propagated seed -> dz2 -> dz1 -> dx (+ the split floor on the 256 x 256 layer)
               + (e_s0 + 4 u) |dxa|                                           the seed's own roundings (p_w, 1 / N_global)
      E_w    = w (3 E_adv + (|3 adv| + 4) u) + 2^-126                         expf, its argument, the 1-Lipschitz clamp
      E_t    = 6 u |t| + wscale (E_w |pi - a| + w E_pi)                       the BC term t = wscale w (pi - a)
      E_f    = 2 |th| E_pi / max_action + 5 u th^2 + u (1 - th^2)             1 - th^2 from the stored output
      E      = max_action (1 - th^2) (E_dxa0 + E_dxa1 + E_t + 3 u sum |terms|) + |d| max_action E_f + 2 u |v|
    and the gradients take grad_bounds(tape, C_E2E, split, "network.", edz3=E, ex=...).  Cases: plain, saturated (every
    third column of b3 shifted by +-7 -- b3 cannot pick rows), clamp, bc_only, pi_only, max_action 0.4 and 2, row_scale and
    Nt = 0, each at every (S, A) and N in {33, 257, 1025}.  These are worst-case bounds, 1 .. 25 % of a typical element (DESIGN.md
    says what that does and does not catch); the exact probes are the sharp part.  The fp32 reference arithmetic
    meets the same bounds on the CPU (tests/test_actor_ref.py); the measured worst err / bound per case, mode and tensor
    is kept in profiles/actor_grad_bounds.json (set MOBODY_ACTOR_BOUNDS_JSON=<path> to rewrite it).
"""
import json
import os

import numpy as np
import pytest
import torch

import actor_ref as AR
import aux_ref as R
import f64_bounds as FB

pytestmark = pytest.mark.gpu

SA = [(11, 3), (17, 6), (45, 24), (111, 8)]
# (N, Nt) -> what the pair is there for
ROWS = [((1, 0), "one row, no BC rows"), ((1, 1), "one row, Nt = N"), ((31, 31), "ragged tile, Nt = N"),
        ((33, 1), "second tile of one row; Nt inside the first"), ((33, 32), "Nt at a tile edge"),
        ((65, 33), "Nt one row into the second tile"), ((257, 129), "wgrad nsplit 2; Nt inside a tile"),
        ((1025, 1024), "2 strides of k_actor_stats; Nt at a tile edge, one non-BC row"),
        ((4097, 31), "5 strides; wgrad nsplit cap with empty slices")]
EXACT = [(n_nt, sa, 1 + (i + k) % 2, ("stats", "adv")[(i + k // 2) % 2])
         for i, (n_nt, _) in enumerate(ROWS) for k, sa in enumerate(SA)]
EXPECT_NT = {(11, 3): 1, (17, 6): 2, (45, 24): 0, (111, 8): 0}


def exact_id(c):
    return f"N{c[0][0]}-Nt{c[0][1]}-S{c[1][0]}A{c[1][1]}-g{c[2]}-{c[3]}"


def exact_probe(c):
    (N, Nt), (S, A), gmul, variant = c
    return AR.int_probe(S, A, N, Nt, gmul, 100 + N + 7 * S + gmul, variant)


def check_case_table():
    """(Also run without a GPU by tests/test_actor_ref.py.)  Every branch the module names is in the tables, from the launch
    formulas: NT 1, 2 and 0 of the input-gradient instance, the weight-gradient split, the strides of k_actor_stats, the
    place of the row < Nt boundary, N_global != N, max_action != 1, and the three regions of the clamp."""
    for sa, nt in EXPECT_NT.items():
        assert AR.bwd_dx_nt(*sa) == nt
    assert {AR.bwd_dx_nt(*c[1]) for c in EXACT} == {0, 1, 2} == {AR.bwd_dx_nt(*c[1]) for c in AR.REAL_CASES}
    assert {AR.stats_strides(c[0][0]) for c in EXACT} >= {1, 2, 5} and {AR.stats_strides(c[2]) for c in AR.REAL_CASES} >= {1, 2}
    assert {AR.nt_place(*c[0]) for c in EXACT} == {"none", "all", "tile_edge", "inside_tile"}
    assert {R.wgrad_nsplit(c[0][0], 1) for c in EXACT} >= {1, 2, 8, 32}
    assert R.wgrad_nsplit(4097, 1) == 32 and "empty_slice" in R.wgrad_geometry(4097, 1)["branches"]
    for sa in SA:                                           # every dim at every row pair, both global factors, both variants
        mine = [c for c in EXACT if c[1] == sa]
        assert {c[0] for c in mine} == {r[0] for r in ROWS} and {c[2] for c in mine} == {1, 2} and {c[3] for c in mine} == {"stats", "adv"}
    assert len(AR.REAL_CASES) == 9 * 4 * 3 == len(set(AR.REAL_CASES))     # every case at every (S, A) and N
    assert {c[1] for c in AR.REAL_CASES} == set(SA) and {c[2] for c in AR.REAL_CASES} == {33, 257, 1025}
    for kind in AR.REAL_KINDS:
        assert {c[3] for c in AR.REAL_CASES if c[0] == kind} == {1, 2}
    assert len(AR.CLAMP_TARGETS) == 5 and min(AR.CLAMP_TARGETS) == -90.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_ACTOR_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst |got - fp64| / bound per tensor, tests/test_hip_actor_fp64.py part (b)", "cases": RATIOS},
                      f, indent=1, sort_keys=True)


def run_actor(p, mode, dev, stats_in=None, stats_mul=1.0, ride=False):
    """pack -> transposes -> NaN sentinels -> actor_forward -> (crafted or scaled stats) -> actor_backward on one workspace.
    ride: pi(s) comes from critic_step(policy_forward=True) instead.  Returns (stats actor_forward wrote, per-tensor
    gradients, loss_out[0:2]) as numpy and asserts that the whole gradient blob was written with exact zeros in its padding."""
    from mobody_amd import _lib, ops, packing
    S, A, N, Nt = p["s"].shape[1], p["act"].shape[1], p["N"], p["Nt"]
    cfg = dict(gamma=0.99, tau=0.005, mfma=mode, **{k: p["h"][k] for k in ("max_action", "weight", "bc_coef", "q_weighted", "scale_Q")})
    actor = packing.pack_mlp([{k[len("network."):]: v for k, v in p["pa"].items()}], S, A, dev)
    q = packing.pack_mlp(p["pq"], S + A, 1, dev, prefixes=["network1.", "network2."])
    actor_T = ops.mlp_transpose(actor, S, A, 1, precision=mode)
    q_T = ops.mlp_transpose(q, S + A, 1, 2, precision=mode)
    dims, hyp = ops.train_dims(S, A, N, Nt, p["Ng"], p["Ntg"]), ops.hyper(cfg)
    ws = ops.train_workspace(dims, dev)
    s, a = torch.from_numpy(p["s"]).to(dev).contiguous(), torch.from_numpy(p["act"]).to(dev).contiguous()
    nan = lambda n: torch.full((n,), float("nan"), device=dev)
    L = _lib.mlp_layout(S, A, 1)
    grad, loss, stats = nan(L.total_floats), nan(2), nan(2)
    if ride:
        z = torch.zeros(N, 1, device=dev)
        ops.critic_step(dims, hyp, actor, q, q_T, q.clone(), (s, a, s, z, z), torch.empty_like(q), nan(1), ws,
                        policy_forward=True, actor_blob_T=actor_T, qtarg_blob_T=q_T.clone())
    ops.actor_forward(dims, hyp, actor, q, s, a, stats, ws, policy_ready=ride, actor_blob_T=actor_T, q_blob_T=q_T)
    torch.cuda.synchronize()
    wrote = stats.cpu().numpy().copy()
    handed = torch.tensor(stats_in, dtype=torch.float32, device=dev) if stats_in is not None else stats * stats_mul
    v_true = torch.from_numpy(p["v_true"]).to(dev) if p["v_true"] is not None else None
    ops.actor_backward(dims, hyp, actor, actor_T, q, q_T, s, a, handed, grad, loss, ws, v_true=v_true)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()), f"{int((~torch.isfinite(grad)).sum())} entries of the gradient blob unwritten / non-finite"
    w1 = packing.wide_unpack(grad[L.w1:L.w1 + L.Kp1 * 256], L.Kp1)
    w3 = grad[L.w3:L.w3 + 256 * L.Np3].view(256, L.Np3)
    b3 = grad[L.b3:L.b3 + L.Np3]
    assert bool((w1[S:] == 0).all()), "dW1 padding rows k >= S are not exactly 0"
    assert bool((w3[:, A:] == 0).all()) and bool((b3[A:] == 0).all()), "dW3 / db3 padding columns are not exactly 0"
    g = {"network." + k: v.cpu().numpy() for k, v in packing.unpack_mlp(grad, S, A, 1)[0].items()}
    return wrote, g, loss.cpu().numpy()


def same_bits(got, want, what):
    """Bit equality of fp32 `got` with the fp64 `want` rounded once (a zero's sign is not a bit of the sum: +0 + -0)."""
    got = np.asarray(got, np.float32) + np.float32(0)
    want = np.asarray(want, np.float64).astype(np.float32) + np.float32(0)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first {i}: got {got[i]!r} want {want[i]!r}")


def test_case_table_covers_what_it_claims():
    check_case_table()


@pytest.mark.parametrize("case", EXACT, ids=exact_id)
def test_exact_probes(case, mfma, dev):
    (N, Nt), (S, A), gmul, variant = case
    assert AR.bwd_dx_nt(S, A) == EXPECT_NT[(S, A)]
    p = exact_probe(case)
    exp, ok, detail = AR.int_probe_expected(p)
    assert ok, f"precondition of bit equality fails: {detail}"
    cf = exp["cf"]
    wrote, g, loss = run_actor(p, mfma, dev, stats_in=p["stats_in"], ride=(N + S) % 2 == 0 and N > 1)
    same_bits(wrote, cf["stats"], "stats of actor_forward")
    for k, v in exp["grads"].items():
        same_bits(g[k], v, f"{exact_id(case)} {mfma} {k}")
    same_bits(loss, [cf["L_pi"], cf["L_BC"]], "loss_out[0:2]")


@pytest.mark.parametrize("case", AR.REAL_CASES, ids=AR.real_id)
def test_actor_vs_fp64_bounds(case, mfma, dev):
    c = AR.real_case(*case)
    assert c["all_robust"] and 8 * c["kept"] >= 7 * c["pool"], (c["kept"], c["pool"])
    bd = AR.real_bounds(*case, mfma == "f16x2")
    cf = c["cf"]
    wrote, g, loss = run_actor(c, mfma, dev, stats_mul=float(c["gmul"]))
    got = dict(g, stats=wrote, L_pi=loss[0], L_BC=loss[1])
    ref = dict(c["grads"], stats=cf["stats"], L_pi=cf["L_pi"], L_BC=cf["L_BC"])
    bound = dict(bd["grads"], stats=bd["stats"], L_pi=bd["L_pi"], L_BC=bd["L_BC"])
    name = f"{AR.real_id(case)}-{mfma}"
    RATIOS[name] = {k: AR.ratios(got[k], ref[k], bound[k]) for k in ref}
    print(name, {k: f"{v:.3g}" for k, v in RATIOS[name].items()})
    for k in ref:
        FB.check(got[k], ref[k], bound[k], f"{name} {k}")
