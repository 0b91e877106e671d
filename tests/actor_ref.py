"""fp64 closed forms, in plain numpy, of the row-wise part of the actor update (csrc/train.h ActorRowArgs / BwdSeed modes 2
and 3, k_actor_stats, LossFinal kind 2; the reference's update_policy and bc_loss, mobody.py:246-276, 314-345), the launch
formulas that pick its kernels, the integer nets of the exact probes and the derived error bound of d(pre-tanh)
(tests/test_hip_actor_fp64.py; every closed form is itself checked against torch.autograd in tests/test_actor_ref.py).

Shapes: pi [N][A] = max_action tanh(z3), qp [2][N] twin Q at (s, pi), qb [2][Nt] twin Q at the true rows (the first Nt),
dqda [2][N][A] = dQ_m/da at (s, pi), act [N][A], stats [2] = the GLOBAL sums (sum |min qp|, sum_{rows < Nt} |min qb|),
v_true [Nt] (the `advantage` variant) or None.  h: dict(max_action, weight, bc_coef, q_weighted, scale_Q).
"""
import functools

import numpy as np

import aux_ref as R
import f64_bounds as FB
import golden_util as gu

U = 2.0 ** -24
TINY = 2.0 ** -126                      # smallest normal fp32: expf may flush what lies below it
LN100 = float(np.log(100.0))
MUTANTS = ("tie_le", "no_clamp", "clamp_10", "bc_all_rows", "nt_local", "n_local", "th_no_div", "no_max_action", "bcw_row")


def closed_forms(pi, qp, qb, dqda, act, h, N, Nt, Ng, Ntg, stats=None, v_true=None, mutant=None):
    """Every row-wise quantity of the actor update.  stats=None: the local sums (one rank).  `mutant`: one of MUTANTS, a
    named wrong reading of the same formulas (the sensitivity table of tests/test_actor_ref.py), else None."""
    assert mutant is None or mutant in MUTANTS
    pi, qp, qb, dqda, act = (np.asarray(x, np.float64) for x in (pi, qp, qb, dqda, act))
    A = pi.shape[1]
    ma, bc_coef = float(h["max_action"]), float(h["bc_coef"])
    minq = np.minimum(qp[0], qp[1])
    local = np.array([np.abs(minq).sum(), np.abs(np.minimum(qb[0], qb[1])).sum() if Nt else 0.0])      # k_actor_stats
    stats = local if stats is None else np.asarray(stats, np.float64)
    ng = float(N if mutant == "n_local" else Ng)
    ntg = float(max(Nt if mutant == "nt_local" else Ntg, 1))
    p_w = h["weight"] / (stats[0] / ng) if h["scale_Q"] else 1.0                       # policy_weight, train.h:23
    # mode 2 (mlp_bwd.hip bwd_seed): dz3[m][row] = -p_w / Ng * d min(q0, q1) / dq_m, a tie split 1/2 as torch.min's backward
    g0 = np.where(qp[0] < qp[1], 1.0, np.where(qp[0] == qp[1], 0.5, 0.0))
    if mutant == "tie_le":
        g0 = np.where(qp[0] <= qp[1], 1.0, 0.0)
    seed = -p_w / ng * np.stack([g0, 1.0 - g0])
    dxa = seed[:, :, None] * dqda
    # BC weights, bc_weight train.h:25-31
    adv = np.zeros(Nt)
    w_unc = np.ones(Nt)
    if h["q_weighted"] and Nt:
        qbm = np.minimum(qb[0], qb[1])
        adv = qbm - np.asarray(v_true, np.float64) if v_true is not None else qbm / (stats[1] / ntg)
        with np.errstate(over="ignore"):                     # the weights are fp32: expf gives 0 below half its smallest subnormal
            w_unc = np.where(3.0 * adv < -150.0 * np.log(2.0), 0.0, np.exp(3.0 * adv))
    cap = {"no_clamp": np.inf, "clamp_10": 10.0}.get(mutant, 100.0)
    bcw = np.minimum(w_unc, cap)
    # mode 3: d(pre-tanh) = (dxa[0] + dxa[1] + [row < Nt] bc_coef 2 w (pi - a) / (Ntg A)) max_action (1 - tanh^2)
    w_row = np.zeros(N)
    w_row[:Nt] = bcw
    is_bc = np.arange(N) < Nt
    if mutant == "bc_all_rows":
        is_bc = np.ones(N, bool)
        w_row[Nt:] = 1.0
    if mutant == "bcw_row":      # a non-BC row takes bcw[row] as a weight AND adds the BC term.  (The read alone -- mode 3 loads
        # bcw[bc ? row : 0] -- is gated by `if (bc)`: reading bcw[row] there would be out of bounds with no numerical effect,
        # which no numerical test can see.  This mutant is the nearest bug that has one.)
        is_bc = np.ones(N, bool)
        w_row[Nt:] = np.resize(bcw, N - Nt) if Nt else 1.0
    df = (pi - act) * is_bc[:, None]
    t = bc_coef * 2.0 / (ntg * A) * w_row[:, None] * df
    d = dxa[0] + dxa[1] + t
    th = pi if mutant == "th_no_div" else pi / ma
    f = 1.0 - th * th
    dz3 = d * (1.0 if mutant == "no_max_action" else ma) * f
    # LossFinal kind 2 (mlp_bwd.hip k_grad_reduce): the local shares of the global means; Nt = 0 gives L_BC = 0
    sq = (w_row[:, None] * df * df)[:Nt].sum()
    L_BC = sq / (ntg * A)
    L_pi = p_w * (-minq).sum() / ng + bc_coef * L_BC
    return dict(p_w=p_w, seed=seed, dxa=dxa, bcw=bcw, adv=adv, w_unc=w_unc, dz3=dz3, stats=local, L_pi=L_pi, L_BC=L_BC,
                d=d, t=t, f=f, df=df, w_row=w_row, minq=minq)


def forward_ref(pa, pq, s, a, Nt, max_action):
    """fp64 forwards of the actor phase from nn.Linear parameter dicts: what closed_forms takes, and the actor's activations."""
    s, a = np.asarray(s, np.float64), np.asarray(a, np.float64)
    (W1, b1), (W2, b2), (W3, b3) = FB.net_weights(pa, "network.")
    z1 = s @ W1 + b1
    z2 = np.maximum(z1, 0) @ W2 + b2
    z3 = np.maximum(z2, 0) @ W3 + b3
    pi = max_action * np.tanh(z3)
    S = s.shape[1]
    qp, dqda, qb = [], [], []
    for pre in ("network1.", "network2."):
        lq = FB.net_weights(pq, pre)
        q, g = FB.input_gradient(lq, np.concatenate([s, pi], 1))
        qp.append(q[:, 0]); dqda.append(g[:, S:])
        qb.append(FB.input_gradient(lq, np.concatenate([s[:Nt], a[:Nt]], 1))[0][:, 0])
    return dict(z1=z1, z2=z2, z3=z3, pi=pi, qp=np.stack(qp), dqda=np.stack(dqda), qb=np.stack(qb))


def actor_grads_ref(pa, s, fw, dz3):
    """The actor's six gradient tensors (nn.Linear names) from d(pre-tanh), and the tape of its three layers in the form
    tests/f64_bounds.py grad_bounds reads."""
    W = {i: np.asarray(pa[f"network.network.{i}.weight"], np.float64) for i in (0, 2, 4)}
    s = np.asarray(s, np.float64)
    h1, h2 = np.maximum(fw["z1"], 0), np.maximum(fw["z2"], 0)
    ref = R.mlp3_backward_ref(W[0][None], W[2][None], W[4][None], s, h1[None], h2[None], dz3[None])
    grads = {"network." + pk: ref[rk][0] for rk, pk in R.GRAD_KEYS}
    tape = {"network.network.0": [dict(x=s, z=fw["z1"], dz=ref["dz1"][0])],
            "network.network.2": [dict(x=h1, z=fw["z2"], dz=ref["dz2"][0])],
            "network.network.4": [dict(x=h2, z=fw["z3"], dz=dz3)],
            "_W": {f"network.network.{i}.weight": W[i] for i in (0, 2, 4)}}
    return grads, tape


# ---- launch formulas (csrc/core.hip mobody_mlp_layout, csrc/mlp_bwd.hip dispatch_dx_nt, train.hip) ----
def bwd_dx_nt(S, A):
    """NT of the frozen-Q backward's input-gradient instance k_mlp3_bwd<true, NT, ...>: Np1t = round_up(S + A, 16)."""
    np1t = (S + A + 15) // 16 * 16
    return 1 if np1t == 16 else 2 if np1t == 32 else 0


def stats_strides(N):
    """Rows base + u * 1024 < N a thread of k_actor_stats visits, summed over its base loop: thread 0 sees ceil(N / 1024)."""
    return -(-N // 1024)


def nt_place(N, Nt):
    """Where the row < Nt boundary falls relative to the 32-row tiles."""
    return "none" if Nt == 0 else "all" if Nt == N else "tile_edge" if Nt % 32 == 0 else "inside_tile"


# ---- integer nets of the exact probes ------------------------------------------------------------------------------
def pow2ceil(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def int_nets(S, A, seed):
    """Actor and twin-Q parameter dicts (nn.Linear names) with small-integer weights, one input per hidden unit on the
    paths a gradient takes, so that every intermediate of the actor phase is an integer (forwards) or an integer multiple
    of one power of two (backwards):
      actor   h1[2j] = h1[2j+1] = relu(+-s_i + b), h2[u] = relu(h1[u] + g) for u < 2A, z3_j = h2[2j] - h2[2j+1] = 0 exactly:
              pi = 0 and tanh' = 1 while dz2 = +-dz3 != 0; further hidden units (sparse {-1, 0, 1}) feed dW3, dW2 only.
      twin Q  member m has relu(+-a_j + c_j) on action column j (+ for m = 0, - for m = 1), shared state units, and one
              state unit of its own (relu(s_1 - 1) in member 0, relu(s_0) in member 1): q0 == q1 at pi = 0 wherever both are
              dead, with dq0/da_j = -dq1/da_j = +-1, and q0 < q1 / q0 > q1 on the other rows."""
    rng = np.random.default_rng(seed)
    H = R.HID
    z = lambda *sh: np.zeros(sh, np.float32)
    W1, b1, W2, b2, W3, b3 = z(H, S), z(H), z(H, H), z(H), z(A, H), z(A)
    for j in range(A):
        i, sg, b = int(rng.integers(S)), float(rng.choice([-1, 1])), float(rng.integers(1, 3))
        g = float(rng.integers(-1, 2))
        for u in (2 * j, 2 * j + 1):
            W1[u, i], b1[u], W2[u, u], b2[u] = sg, b, 1.0, g
        W3[j, 2 * j], W3[j, 2 * j + 1] = 1.0, -1.0
    ext = np.arange(2 * A, 2 * A + 32)
    W1[ext] = rng.integers(-1, 2, (32, S)) * (rng.random((32, S)) < 2.0 / S)
    b1[ext] = rng.integers(-1, 2, 32)
    W2[np.ix_(ext, ext)] = rng.integers(-1, 2, (32, 32)) * (rng.random((32, 32)) < 0.1)
    b2[ext] = rng.integers(0, 2, 32)
    pa = {"network.network.0.weight": W1, "network.network.0.bias": b1, "network.network.2.weight": W2,
          "network.network.2.bias": b2, "network.network.4.weight": W3, "network.network.4.bias": b3}
    pq = {}
    ns = min(S, 16)
    cj, gj, wj = rng.integers(1, 4, A), rng.integers(-1, 1, A), rng.choice([-1.0, 1.0], A)
    gj[0] = -cj[0]                                              # one action unit dead at pi = 0: its dq/da is 0
    si, ssg, sb, sw = rng.integers(0, S, ns), rng.choice([-1.0, 1.0], ns), rng.integers(-1, 2, ns), rng.choice([-1.0, 1.0], ns)
    q_b3 = float(rng.integers(-2, 3))
    for m, pre in enumerate(("network1.", "network2.")):
        W1, b1, W2, b2, W3, b3 = z(H, S + A), z(H), z(H, H), z(H), z(1, H), z(1)
        for j in range(A):
            W1[j, S + j], b1[j], W2[j, j], b2[j], W3[0, j] = (1.0, -1.0)[m], cj[j], 1.0, gj[j], wj[j]
        for k in range(ns):
            u = A + k
            W1[u, si[k]], b1[u], W2[u, u], W3[0, u] = ssg[k], sb[k], 1.0, sw[k]
        u = A + ns + m
        if m == 0:
            W1[u, 1 % S], b1[u] = 1.0, -1.0
        else:
            W1[u, 0] = 1.0
        W2[u, u], W3[0, u], b3[0] = 1.0, 1.0, q_b3
        for k, v in (("network.0.weight", W1), ("network.0.bias", b1), ("network.2.weight", W2), ("network.2.bias", b2),
                     ("network.4.weight", W3), ("network.4.bias", b3)):
            pq[pre + k] = v
    return pa, pq


def int_probe(S, A, N, Nt, gmul, seed, variant):
    """One exact probe: nets, batch, hyper-parameters, the stats handed to the backward and the global counts, all chosen
    so that every scalar factor is a power of two:  N_global = gmul * pow2ceil(N) (1 / N_global is not representable for
    any other count), Nt_global likewise, stats[0] = N_global * 2^k (so p_w = 2^(1-k)), weight = 2, bc_coef = (odd part of A) / 2 -- then
    bc_coef * 2 / (Nt_global * A) is a power of two -- and max_action in {1/2, 1, 2}.
    variant "stats": adv = qb / (stats[1] / Nt_global) with stats[1] = Nt_global / 64, so 3 adv = 192 qb is 0, >= ln 100 or
    <= -104 for every integer qb.  variant "adv": v_true = qb - (0, 2, -35 in turn), the same three values of adv."""
    rng = np.random.default_rng(seed + 1)
    pa, pq = int_nets(S, A, seed)
    s = rng.integers(-3, 4, (N, S)).astype(np.float32)
    rep = 3 if A % 3 == 0 else 1            # every |pi - a|^2 three times: sum w (pi - a)^2 / (Ntg A) stays a dyadic number
    act = np.repeat(rng.integers(-2, 3, (N, A // rep)), rep, axis=1).astype(np.float32)
    Ng, Ntg = gmul * pow2ceil(N), gmul * pow2ceil(max(Nt, 1))
    odd = A
    while odd % 2 == 0:
        odd //= 2
    ma = (1.0, 2.0, 0.5)[seed % 3]
    h = dict(max_action=ma, weight=2.0, bc_coef=odd / 2.0, q_weighted=1, scale_Q=1, advantage=int(variant == "adv"))
    fw = forward_ref(pa, pq, s, act, Nt, ma)
    if Nt:                                  # centre min(qb) on 0 (both members' b3 move together: ties stay ties)
        shift = np.float32(np.median(np.minimum(fw["qb"][0], fw["qb"][1])).round())
        for pre in ("network1.", "network2."):
            pq[pre + "network.4.bias"] = pq[pre + "network.4.bias"] - shift
        fw = forward_ref(pa, pq, s, act, Nt, ma)
    # p_w = weight / (stats[0] / N_global) within a factor 2 of N_global * wscale: the frozen-Q term and the BC term of
    # d(pre-tanh) then share one tile of the fp16 split without either losing bits (f16_bits_ok)
    p_w = 2.0 ** np.rint(np.log2(Ng * h["bc_coef"] * 2.0 / (Ntg * A))) * (1.0, 2.0, 0.5)[seed % 3]
    stats_in = np.array([h["weight"] * Ng / p_w, Ntg / 64.0])
    v_true = None
    if variant == "adv":
        v_true = (np.minimum(fw["qb"][0], fw["qb"][1]) - np.resize([0.0, 2.0, -35.0], Nt)).astype(np.float32)
    return dict(pa=pa, pq=pq, s=s, act=act, h=h, fw=fw, N=N, Nt=Nt, Ng=Ng, Ntg=Ntg, stats_in=stats_in, v_true=v_true)


def dyadic_ok(x, sum_abs, quantum):
    """Exactness precondition of one output: every value an integer multiple of `quantum` (a power of two), and the sum of
    absolute values of its terms below 2^24 quanta -- then every partial sum in every order is exact in fp32."""
    x = np.asarray(x, np.float64) / quantum
    return bool(np.array_equal(x, np.rint(x))) and float(np.max(sum_abs, initial=0.0)) / quantum < R.TWO24


def int_probe_expected(p):
    """Expected outputs of an exact probe and the check of its precondition.  Returns (dict, ok, detail)."""
    fw, h, N, Nt = p["fw"], p["h"], p["N"], p["Nt"]
    cf = closed_forms(fw["pi"], fw["qp"], fw["qb"], fw["dqda"], p["act"], h, N, Nt, p["Ng"], p["Ntg"], stats=p["stats_in"],
                      v_true=p["v_true"])
    grads, tape = actor_grads_ref(p["pa"], p["s"], fw, cf["dz3"])
    A = p["act"].shape[1]
    quantum = min(abs(cf["p_w"]) / p["Ng"] / 2.0, h["bc_coef"] * 2.0 / (p["Ntg"] * A)) * h["max_action"]
    W = tape["_W"]
    ok = np.all(fw["pi"] == 0) and np.all(fw["z3"] == 0) and set(np.unique(cf["bcw"])) <= {0.0, 1.0, 100.0}
    ok = ok and all(np.array_equal(fw[k], np.rint(fw[k])) for k in ("qp", "qb", "z1", "z2"))
    detail = {}
    ax = {0: np.abs(p["s"].astype(np.float64)), 2: np.maximum(fw["z1"], 0), 4: np.maximum(fw["z2"], 0)}
    for i in (0, 2, 4):
        adz = np.abs(tape[f"network.network.{i}"][0]["dz"])
        good = dyadic_ok(grads[f"network.network.{i}.weight"], adz.T @ ax[i], quantum) and \
            dyadic_ok(grads[f"network.network.{i}.bias"], adz.sum(0), quantum)
        detail[i] = good
        ok = ok and good
    # the scalars: every intermediate of `pw * s0 / ng + bc_coef * bc` representable, so neither the order nor an fma matters
    s0, sq = (-cf["minq"]).sum(), (cf["w_row"][:, None] * cf["df"] ** 2).sum()
    for v in (cf["p_w"] * s0, cf["p_w"] * s0 / p["Ng"], cf["L_BC"], h["bc_coef"] * cf["L_BC"], cf["L_pi"], cf["stats"][0], cf["stats"][1]):
        ok = ok and float(np.float32(v)) == float(v)
    ok = ok and np.abs(cf["minq"]).sum() < R.TWO24 and sq < R.TWO24
    return dict(cf=cf, grads=grads, tape=tape, quantum=quantum), bool(ok), detail


def f16_bits_ok(p, exp):
    """The "f16x2" precondition: every operand of the GEMMs that run on the fp16 core (h1 of both nets in the forward, dz2 in
    the backwards, both again in the layer-2 weight gradient) keeps at most 11 significant bits below the largest
    magnitude of its 32-row tile, i.e. tile maximum / lowest set bit of the value < 2^11."""
    fw = p["fw"]
    ops_ = [np.maximum(fw["z1"], 0), exp["tape"]["network.network.2"][0]["dz"]]
    for x in ops_:
        x = np.abs(np.asarray(x, np.float64))
        tm = FB.tile_max(x)
        with np.errstate(divide="ignore", invalid="ignore"):
            m, e = np.frexp(x)
            low = np.ldexp(1.0, e - 53) * ((m * 2.0 ** 53).astype(np.int64) & -(m * 2.0 ** 53).astype(np.int64))
        if np.any((x > 0) & (tm / np.where(x > 0, low, 1.0) >= 2.0 ** 11)):
            return False
    return True


# ---- the derived bound of the real-valued cases ------------------------------------------------------------------------
def dx_rounding(lq, z1, z2, seed, S, split):
    """Rounding of the frozen-Q backward (k_mlp3_bwd<DX>) onto the action columns: c |dz| |W^T| propagated from the seed
    down to dx, with the split floor on the 256 x 256 layer.  Returns the bound [N, A]."""
    (W1, _), (W2, _), (W3, _) = lq
    c = FB.C_E2E
    dz2 = np.abs(seed[:, None] * W3[:, 0][None, :]) * (z2 > 0)
    E2 = c * dz2
    dz1 = (dz2 @ np.abs(W2).T) * (z1 > 0)
    E1 = c * dz1 + E2 @ np.abs(W2).T
    if split:
        E1 = E1 + FB.SUBNORMAL * FB.tile_max(dz2) * np.abs(W2).sum(1)[None, :]
    E1 = E1 * (z1 > 0)
    return (c * dz1 + E1) @ np.abs(W1).T[:, S:]


def actor_bounds(pa, pq, s, a, h, N, Nt, Ng, Ntg, fw, cf, tape, split, v_true=None):
    """Per-element bounds of the actor phase against fp64 (conventions of tests/f64_bounds.py; u = 2^-24).  Returns
    dict(stats [2], L_pi, L_BC, dz3 [N, A], grads {name: bound})."""
    s, a = np.asarray(s, np.float64), np.asarray(a, np.float64)
    S, A = s.shape[1], a.shape[1]
    ma = float(h["max_action"])
    la = FB.net_weights(pa, "network.")
    pad = lambda L: np.maximum(L[0][1], 0).max()
    # forward errors.  pi = max_action * tanhf(z3) (layers.h:194): tanh' <= 1 - tanh^2(|z3| - E_z3) on the interval the
    # computed z3 lies in, tanhf itself and the product a few units in the last place of pi
    _, Ez3 = FB.e2e_bound(s, la, FB.C_E2E, split, pad(la))
    fmax = 1.0 - np.tanh(np.maximum(np.abs(fw["z3"]) - Ez3, 0.0)) ** 2
    Epi = ma * fmax * Ez3 + 4 * U * np.abs(fw["pi"])
    Eqp, Eqb, Edx = 0.0, 0.0, []
    x = np.concatenate([s, fw["pi"]], 1)
    for m, pre in enumerate(("network1.", "network2.")):
        lq = FB.net_weights(pq, pre)
        # q at (s, pi): its own forward bound + |dq/da| E_pi (masks fixed on robust rows: q is linear in a there)
        Eqp = np.maximum(Eqp, FB.e2e_bound(x, lq, FB.C_E2E, split, pad(lq))[1][:, 0] + (np.abs(fw["dqda"][m]) * Epi).sum(1))
        if Nt:
            Eqb = np.maximum(Eqb, FB.e2e_bound(np.concatenate([s[:Nt], a[:Nt]], 1), lq, FB.C_E2E, split, pad(lq))[1][:, 0])
        z1 = x @ lq[0][0] + lq[0][1]
        z2 = np.maximum(z1, 0) @ lq[1][0] + lq[1][1]
        Edx.append(dx_rounding(lq, z1, z2, cf["seed"][m], S, split))
    # k_actor_stats (train.hip:97-119): at most N sequential adds, the forward error of every term
    qbm = np.minimum(fw["qb"][0], fw["qb"][1])
    Bs = np.array([(N + 3) * U * np.abs(cf["minq"]).sum() + np.sum(Eqp), (Nt + 3) * U * np.abs(qbm).sum() + np.sum(Eqb)])
    es = Bs / np.maximum(np.abs(cf["stats"]), 1e-300)        # relative error of the sums handed to the backward
    # the mode-2 seed -p_w / Ng * g (train.h:23 two divisions, mlp_bwd.hip:171 one, :173 one product)
    e_seed = (es[0] if h["scale_Q"] else 0.0) + 4 * U
    Edxa = [Edx[m] + e_seed * np.abs(cf["dxa"][m]) for m in range(2)]
    # the BC weight fminf(expf(3 adv), 100) (train.h:27-30): the clamp is 1-Lipschitz; expf below the normal range may flush
    Ew = np.zeros(N)
    if h["q_weighted"] and Nt:
        adv = cf["adv"]
        Eadv = Eqb + U * np.abs(adv) if v_true is not None else Eqb / (np.abs(cf["stats"][1]) / Ntg) + np.abs(adv) * (es[1] + 3 * U)
        Ew[:Nt] = np.minimum(cf["w_unc"], 100.0) * (3 * Eadv + (np.abs(3 * adv) + 4) * U) + TINY
    # the BC term wscale * w * (pi - a) (mlp_bwd.hip:187 three roundings, :201 two products and the difference)
    wscale = h["bc_coef"] * 2.0 / (max(Ntg, 1) * A)
    isbc = (np.arange(N) < Nt)[:, None]
    Et = np.abs(cf["t"]) * 6 * U + wscale * (Ew[:, None] * np.abs(cf["df"]) + cf["w_row"][:, None] * Epi * isbc)
    # d = d0 + d1 + t (:200-201)
    Ed = Edxa[0] + Edxa[1] + Et + 3 * U * (np.abs(cf["dxa"][0]) + np.abs(cf["dxa"][1]) + np.abs(cf["t"]))
    # th = p / max_action; 1 - th * th (:202-203): the error of p itself, the division, the square, the difference
    th = fw["pi"] / ma
    Ef = 2 * np.abs(th) * Epi / ma + 5 * U * th * th + U * cf["f"]
    # v = d * max_action * (1 - th^2) (:203): two products
    E = ma * cf["f"] * Ed + np.abs(cf["d"]) * ma * Ef + 2 * U * np.abs(cf["dz3"])
    # LossFinal kind 2 (mlp_bwd.hip:884-887)
    sq_terms = cf["w_row"][:, None] * cf["df"] ** 2
    E_LBC = ((Nt * A + 3) * U * sq_terms.sum() + (Ew[:, None] * cf["df"] ** 2 + 2 * cf["w_row"][:, None] * np.abs(cf["df"]) * Epi * isbc).sum()) \
        / (max(Ntg, 1) * A) + 2 * U * cf["L_BC"]
    pw = abs(cf["p_w"])
    first = cf["p_w"] * (-cf["minq"]).sum() / Ng
    E_Lpi = pw / Ng * ((N + 3) * U * np.abs(cf["minq"]).sum() + np.sum(Eqp)) + (e_seed + 2 * U) * abs(first) \
        + h["bc_coef"] * E_LBC + 2 * U * (abs(first) + h["bc_coef"] * cf["L_BC"])
    # the gradients: grad_bounds with E as the error of the output gradient; ex = forward error of each layer's input
    (W1, b1), (W2, b2), _ = la
    z1, e1 = FB.layer_bound(s, W1, b1, FB.C_E2E)
    _, e2 = FB.layer_bound(np.maximum(z1, 0), W2, b2, FB.C_E2E, split=split, pad=pad(la))
    gb = FB.grad_bounds(tape, FB.C_E2E, split, "network.", edz3=E, ex={2: e1, 4: e1 @ np.abs(W2) + e2})
    return dict(stats=Bs, L_pi=E_Lpi, L_BC=E_LBC, dz3=E, grads=gb)


# ---- real-valued cases -----------------------------------------------------------------------------------------------
# (case, (S, A), N, N_global / N): every case at every shipped (S, A) and every N, the global factor 1 and 2 in turn
REAL_KINDS = ("plain", "saturated", "clamp", "bc_only", "pi_only", "max_action_0.4", "max_action_2", "row_scale", "nt0")
REAL_SA = ((11, 3), (17, 6), (45, 24), (111, 8))
REAL_N = (33, 257, 1025)
REAL_CASES = [(kind, sa, N, 1 + (i + j + k) % 2) for i, kind in enumerate(REAL_KINDS) for j, sa in enumerate(REAL_SA)
              for k, N in enumerate(REAL_N)]
SEED_TRIES = 8       # a case takes the first of its 8 seeds whose pool keeps 7/8 of its rows and yields N robust ones
CLAMP_TARGETS = (LN100 + 1e-3, LN100 - 1e-3, LN100 + 1.0, LN100 - 1.0, -90.0)


def real_id(c):
    return f"{c[0]}-S{c[1][0]}A{c[1][1]}-N{c[2]}-g{c[3]}"


@functools.lru_cache(maxsize=8)
def real_case(case, SA, N, gmul):
    """Parameters as gu.policy_params, a batch of N robust rows out of a pool of 4 N (FB.robust_rows), the fp64 reference of
    every checked output and what the bounds need.  Cached: the f32 and f16x2 runs share one reference."""
    base = 700 + 13 * REAL_CASES.index((case, SA, N, gmul))
    for shift in range(SEED_TRIES):
        c = _real_case(case, SA, N, gmul, base + shift)
        if c["all_robust"] and 8 * c["kept"] >= 7 * c["pool"]:
            break
    return c


def _real_case(case, SA, N, gmul, seed):
    S, A = SA
    pa, pq, _ = gu.policy_params(seed, S, A)
    pa = {k: v.copy() for k, v in pa.items()}
    ma = {"max_action_0.4": 0.4, "max_action_2": 2.0}.get(case, 1.0)
    h = dict(max_action=ma, weight=2.5, bc_coef=1.0, q_weighted=1, scale_Q=1, advantage=int(case == "clamp"))
    if case == "bc_only":
        h.update(scale_Q=0, weight=0.0)     # p_w = 1; the frozen-Q term stays, of order 1 / N next to the BC term's 1 / (Nt A)
    if case == "pi_only":
        h.update(bc_coef=0.0)
    if case.startswith("max_action"):       # |z3| of order 1 on every third column: th = pi / max_action is not small there
        b3 = pa["network.network.4.bias"]
        b3[::3] += np.where(np.arange(len(b3[::3])) % 2, -1.0, 1.0).astype(np.float32)
    if case == "saturated":                 # b3 is per column, so the shift cannot pick rows: every third COLUMN sits at |z3| in
        # about 5 .. 9 on every row (not a third of the rows): each row has saturated and unsaturated elements, no tile mixes
        # saturated with unsaturated rows
        b3 = pa["network.network.4.bias"]
        b3[::3] += (7.0 * np.where(np.arange(len(b3[::3])) % 2, -1.0, 1.0)).astype(np.float32)
    Nt = 0 if case == "nt0" else (N // 2) | 1
    s, a, _, _, _ = gu.gi.batch(seed + 5, 4 * N, S, A)
    a = (a * np.float32(ma)).astype(np.float32)
    if case == "row_scale":                 # one power of two per 32-row tile of the pool: 2^-12, 1, 2^12 in turn
        k = (np.arange(4 * N) // 32) % 3
        s = (s * np.exp2(12.0 * (k - 1))[:, None]).astype(np.float32)
    ok = FB.robust_rows(pa, pq, s, a, max_action=ma)
    keep = np.flatnonzero(ok)
    if case == "row_scale":                 # tile t of the batch takes rows of pool scale t % 3
        want = (np.arange(N) // 32) % 3
        pools = [list(keep[((keep // 32) % 3) == j]) for j in range(3)]
        idx = np.array([pools[j].pop(0) for j in want if pools[j]])
    else:
        idx = keep[:N]
    s, a = s[idx].copy(), a[idx].copy()
    Ng, Ntg = gmul * N, gmul * Nt
    fw = forward_ref(pa, pq, s, a, Nt, ma)
    v_true = None
    if case == "clamp":
        v_true = (np.minimum(fw["qb"][0], fw["qb"][1]) - np.resize(CLAMP_TARGETS, Nt) / 3.0).astype(np.float32)
    local = closed_forms(fw["pi"], fw["qp"], fw["qb"], fw["dqda"], a, h, N, Nt, Ng, Ntg, v_true=v_true)["stats"]
    cf = closed_forms(fw["pi"], fw["qp"], fw["qb"], fw["dqda"], a, h, N, Nt, Ng, Ntg, stats=gmul * local, v_true=v_true)
    grads, tape = actor_grads_ref(pa, s, fw, cf["dz3"])
    return dict(pa=pa, pq=pq, s=s, act=a, h=h, N=N, Nt=Nt, Ng=Ng, Ntg=Ntg, gmul=gmul, fw=fw, cf=cf, grads=grads, tape=tape,
                v_true=v_true, pool=4 * N, kept=int(keep.size), all_robust=bool(len(idx) == N))


@functools.lru_cache(maxsize=8)
def real_bounds(case, SA, N, gmul, split):
    c = real_case(case, SA, N, gmul)
    return actor_bounds(c["pa"], c["pq"], c["s"], c["act"], c["h"], N, c["Nt"], c["Ng"], c["Ntg"], c["fw"], c["cf"], c["tape"],
                        split, v_true=c["v_true"])


def ratios(got, ref, bound):
    """Worst |got - ref| / bound of one tensor (inf where the bound is 0 and the error is not)."""
    err = np.abs(FB.f64(got) - FB.f64(ref))
    bound = np.broadcast_to(FB.f64(bound), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r, initial=0.0))
