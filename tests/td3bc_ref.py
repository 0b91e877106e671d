"""CPU references of the TD3_BC baseline (the reference's algo/offline_offline/td3_bc.py), written from the algorithm:

  train_step / dara_relabel   an fp32 torch restatement of one `TD3BC.train` step after the batch is assembled (critic,
                              Polyak, actor with the BC weight's gradient, Adam), checked against the g23 fixtures
  closed_forms                fp64 numpy closed forms of the row-wise part the kernels compute: BwdSeed mode 4 (the frozen twin-Q
                              seed with the gradient through the BC weight, csrc/train.h), mode 3 with Nt = N, LossFinal kind 2
  td3bc_bounds                the per-element error bound of tests/actor_ref.py actor_bounds with the seed's bound extended by the
                              error of expf and of e / m

Shapes as tests/actor_ref.py: pi [N][A] = max_action tanh(z3), qp [2][N] twin Q at (s, pi), dqda [2][N][A] = dQ_m/da there,
act [N][A], stats[0] = the GLOBAL sum |min qp|.  h: dict(max_action, weight, bc_coef, q_weighted) -- q_weighted is the
reference's config['advantage'] == 1.
"""
import numpy as np
import torch

import actor_ref as AR
import f64_bounds as FB
from oracle import mobody_oracle as O

U = AR.U
EXP_SCALE = 1.0          # td3_bc.py:167 exp(1 * adv); MOBODY's bc_loss has 3
CLAMP = 100.0
VARIANTS = dict(default={}, adv=dict(advantage=1), adv_bc05=dict(advantage=1, bc_coef=0.05, trg_ratio=0.5),
                dara=dict(penalty_type="dara"))


# ---- fp32 restatement of the step ----------------------------------------------------------------------------------------
def policy_loss(ap, q_now, s, a, cfg, detach_weight=False, stats0=None, n_global=None):
    """update_policy, td3_bc.py:160-176.  detach_weight: the mutant whose BC weight carries no gradient.  stats0 / n_global:
    the global sum |q| and row count a data-parallel caller hands (default: this batch's)."""
    pi = O.actor(ap, s, cfg["max_action"], dtype=s.dtype)
    b1, b2 = O.twin_q(q_now, s, pi, dtype=s.dtype)
    qv = torch.min(b1, b2)
    n = float(n_global or s.shape[0])
    m = (qv.abs().sum().detach() if stats0 is None else torch.as_tensor(stats0, dtype=s.dtype)) / n
    p_w = cfg["weight"] / m
    w = torch.exp(EXP_SCALE * (qv / m)).clamp(max=CLAMP)
    if detach_weight:
        w = w.detach()
    sq = (pi - a) ** 2
    bc = (w * sq if cfg["advantage"] == 1 else sq).sum() / (n * a.shape[1])
    return p_w * (-qv).sum() / n + cfg["bc_coef"] * bc, dict(pi=pi, qv=qv, w=w, bc=bc)


def train_step(st, batch, cfg, detach_weight=False):
    """One TD3BC.train step (td3_bc.py:207-224) on the assembled batch; `st` is an oracle TrainState (no V net)."""
    s, a, s2, r, nd = [O.T(x) for x in batch]
    req = lambda d: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    qp = req(st.q)
    with torch.no_grad():                                              # update_q_functions :147-158
        t1, t2 = O.twin_q(st.q_targ, s2, O.actor(st.actor, s2, cfg["max_action"]))
        y = r + nd * cfg["gamma"] * torch.min(t1, t2)
    q1, q2 = O.twin_q(qp, s, a)
    q_loss = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
    gq = O._grads(q_loss, qp)
    st.t["q"] += 1
    for k in st.q:
        O.adam_update(st.q[k], gq[k], st.m["q"][k], st.s["q"][k], st.t["q"], cfg["critic_lr"])
    O.polyak(st.q_targ, st.q, cfg["tau"])
    ap = req(st.actor)
    loss, aux = policy_loss(ap, st.q, s, a, cfg, detach_weight)
    ga = O._grads(loss, ap)
    st.t["actor"] += 1
    for k in st.actor:
        O.adam_update(st.actor[k], ga[k], st.m["actor"][k], st.s["actor"][k], st.t["actor"], cfg["actor_lr"])
    return dict(q_loss=q_loss.detach(), pi_loss=loss.detach(), bc_loss=aux["bc"].detach(), q_grads=gq, actor_grads=ga,
                bc_w=aux["w"].detach())


class ClassifierState:
    def __init__(self, params):
        self.p = {k: O.T(v).clone() for k, v in params.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.s = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.t = 0


def dara_relabel(cls, src, tar, bs, perm, noise_sas, noise_sa, cfg):
    """penalty_type 'dara' of TD3BC.train (:187-200): one update_classifier step (:108-129) on src[:bs] | tar[:bs], permuted,
    with the recorded noise, then the noise-free penalty on the step's source rows.  Returns src_reward + 0.1 * penalty."""
    rows = [np.concatenate([x[:bs], y[:bs]], 0)[perm] for x, y in zip(src[:3], tar[:3])]
    label = np.concatenate([np.zeros(bs), np.ones(bs)])[perm]
    cp = {k: v.detach().clone().requires_grad_(True) for k, v in cls.p.items()}
    loss = O.classifier_loss(cp, *rows, label, noise_sas, noise_sa, cfg["gaussian_noise_std"])
    g = O._grads(loss, cp)
    cls.t += 1
    for k in cls.p:
        O.adam_update(cls.p[k], g[k], cls.m[k], cls.s[k], cls.t, cfg["actor_lr"])
    with torch.no_grad():
        pen = O.dara_delta_r(cls.p, src[0][:bs], src[1][:bs], src[2][:bs])
    return src[3][:bs] + 0.1 * pen.numpy()


def g23_rows(S, A):
    import golden_util as gu
    return gu.gi.batch(501, 64, S, A), gu.gi.batch(502, 64, S, A)


def g23_batch(cfg, bs, S, A, src_reward=None):
    """src(bs) | tar(int(trg_ratio * bs)) from the FixedRB presets of tests/golden/make_golden_td3bc.py."""
    src, tar = g23_rows(S, A)
    nt = int(cfg["trg_ratio"] * bs)
    parts = [[x[:bs].copy() for x in src], [x[:nt].copy() for x in tar]]
    if src_reward is not None:
        parts[0][3] = np.asarray(src_reward, np.float32)
    return tuple(np.concatenate([p[i] for p in parts], 0) for i in range(5))


def classifier_params():
    import golden_util as gu
    pc = {"sa_classifier." + k: v for k, v in gu.gi.mlp_params(701, 17 + 6, 2).items()}
    pc.update({"sas_classifier." + k: v for k, v in gu.gi.mlp_params(702, 2 * 17 + 6, 2).items()})
    return pc


# ---- fp64 closed forms ---------------------------------------------------------------------------------------------------
def closed_forms(pi, qp, dqda, act, h, N, Ng, stats=None, detach_weight=False):
    """Every row-wise quantity of the TD3_BC actor update, in the key names of actor_ref.closed_forms (Nt = N, Ntg = Ng)."""
    pi, qp, dqda, act = (np.asarray(x, np.float64) for x in (pi, qp, dqda, act))
    A = pi.shape[1]
    ma, bc_coef, ng = float(h["max_action"]), float(h["bc_coef"]), float(Ng)
    minq = np.minimum(qp[0], qp[1])
    local = np.array([np.abs(minq).sum(), 0.0])                              # k_actor_stats with Nt = 0
    stats = local if stats is None else np.asarray(stats, np.float64)
    m = stats[0] / ng
    p_w = h["weight"] / m
    df = pi - act
    sq = (df * df).sum(1)
    adv = EXP_SCALE * minq / m
    e = np.exp(np.minimum(adv, 700.0))                                       # (fp64 exp overflows past 709; the clamp is at ln 100)
    weighted = bool(h["q_weighted"])
    w = np.minimum(e, CLAMP) if weighted else np.ones(N)
    # mode 4: dq = -(weight / m) / Ng + [weighted, e <= 100] bc_coef (k e / m) sq / (Ng A); ties split 1/2
    through = (e <= CLAMP) & weighted & (not detach_weight)
    gw = np.where(through, bc_coef * (EXP_SCALE * e / m) * sq / (ng * A), 0.0)
    dq = -p_w / ng + gw
    g0 = np.where(qp[0] < qp[1], 1.0, np.where(qp[0] == qp[1], 0.5, 0.0))
    seed = dq * np.stack([g0, 1.0 - g0])
    dxa = seed[:, :, None] * dqda
    # mode 3 with Nt = N
    t = bc_coef * 2.0 / (ng * A) * w[:, None] * df
    d = dxa[0] + dxa[1] + t
    th = pi / ma
    f = 1.0 - th * th
    dz3 = d * ma * f
    L_BC = (w[:, None] * df * df).sum() / (ng * A)
    L_pi = p_w * (-minq).sum() / ng + bc_coef * L_BC
    return dict(p_w=p_w, m=m, e=e, gw=gw, dq=dq, sq=sq, seed=seed, dxa=dxa, bcw=w, adv=adv, w_unc=e, dz3=dz3, stats=local,
                L_pi=L_pi, L_BC=L_BC, d=d, t=t, f=f, df=df, w_row=w, minq=minq, through=through)


def td3bc_bounds(pa, pq, s, a, h, N, Ng, fw, cf, tape, split, stats_exact=False, resolved=None):
    """actor_ref.actor_bounds for the TD3_BC update.  Differences, all in the seed (u = 2^-24):
      q       the weight's argument is min qp itself: E_adv = E_q / m + |adv| (e_s + 3 u)        (division, relative error of m)
      E_e     = e (E_adv + (|adv| + 4) u)                                                         expf: argument error, 4 ulp
      E_w     = min(e, 100) (...) + 2^-126                                                        the 1-Lipschitz clamp
      E_sq    = 2 |pi - a| E_pi summed + (A + 3) u sq                                             A squares added in any order
      E_gw    = gw (E_e / e + e_s + E_sq / sq + 8 u)                                              bc_coef (k e / m) sq / (Ng A): 7 roundings
      E_dq    = (e_s + 4 u) p_w / Ng + E_gw + u |dq|                                              and dq's own sum
    A row within E_e of the clamp may take either side of the select: the whole term is added to its E_gw (`near`) -- unless
    the caller shows which side the kernel took (`resolved`, clamp_side_resolved: the a-priori band E_e comes from the
    worst-case forward bound of q and is wide where mean|q| is small).
    dxa's error is then E_dx of the frozen-Q backward at the seed + E_dq |dqda|."""
    s64, a64 = np.asarray(s, np.float64), np.asarray(a, np.float64)
    S, A = s64.shape[1], a64.shape[1]
    ma = float(h["max_action"])
    la = FB.net_weights(pa, "network.")
    pad = lambda L: np.maximum(L[0][1], 0).max()
    _, Ez3 = FB.e2e_bound(s64, la, FB.C_E2E, split, pad(la))
    fmax = 1.0 - np.tanh(np.maximum(np.abs(fw["z3"]) - Ez3, 0.0)) ** 2
    Epi = ma * fmax * Ez3 + 4 * U * np.abs(fw["pi"])
    x = np.concatenate([s64, fw["pi"]], 1)
    Eq, Edx = 0.0, []
    for mi, pre in enumerate(("network1.", "network2.")):
        lq = FB.net_weights(pq, pre)
        Eq = np.maximum(Eq, FB.e2e_bound(x, lq, FB.C_E2E, split, pad(lq))[1][:, 0] + (np.abs(fw["dqda"][mi]) * Epi).sum(1))
        z1 = x @ lq[0][0] + lq[0][1]
        z2 = np.maximum(z1, 0) @ lq[1][0] + lq[1][1]
        Edx.append(AR.dx_rounding(lq, z1, z2, cf["seed"][mi], S, split))
    m = abs(cf["m"])
    # k_actor_stats: at most N sequential adds, the forward error of every term; stats[1] = 0 exactly
    Bs = np.array([(N + 3) * U * np.abs(cf["minq"]).sum() + np.sum(Eq), 0.0])
    # relative error of the sum handed to the backward; stats_exact: the caller hands a crafted fp32 value the closed forms took too
    es = 0.0 if stats_exact else Bs[0] / max(abs(cf["stats"][0]), 1e-300)
    adv = cf["adv"]
    Eadv = Eq / m + np.abs(adv) * (es + 3 * U)
    weighted = bool(h["q_weighted"])
    e = cf["e"]
    Ee = e * (Eadv + (np.abs(adv) + 4) * U) if weighted else np.zeros(N)
    Ew = np.minimum(e, CLAMP) * (Eadv + (np.abs(adv) + 4) * U) + AR.TINY if weighted else np.zeros(N)
    Esq = (2 * np.abs(cf["df"]) * Epi).sum(1) + (A + 3) * U * cf["sq"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(cf["gw"] != 0, Ee / e + es + np.where(cf["sq"] > 0, Esq / cf["sq"], 0.0) + 8 * U, 0.0)
    Egw = np.abs(cf["gw"]) * rel
    # a row whose e lies within its own error of the clamp: the select may fall either way, the whole term is its error
    # (`resolved`: rows of those whose side of the select is known to be the closed form's -- clamp_side_resolved)
    near = (np.abs(e - CLAMP) <= Ee) & weighted
    apriori = near.copy()
    if resolved is not None:
        near = near & ~np.asarray(resolved, bool)
    Egw = Egw + np.where(near, h["bc_coef"] * (EXP_SCALE * e / m) * cf["sq"] / (Ng * A), 0.0)
    Edq = (es + 4 * U) * abs(cf["p_w"]) / Ng + Egw + U * np.abs(cf["dq"])
    g = np.abs(np.stack([cf["seed"][0], cf["seed"][1]])) / np.maximum(np.abs(cf["dq"]), 1e-300)       # 1, 1/2 or 0
    Edxa = [Edx[mi] + (g[mi] * Edq)[:, None] * np.abs(fw["dqda"][mi]) + U * np.abs(cf["dxa"][mi]) for mi in range(2)]
    wscale = h["bc_coef"] * 2.0 / (Ng * A)
    Et = np.abs(cf["t"]) * 6 * U + wscale * (Ew[:, None] * np.abs(cf["df"]) + cf["w_row"][:, None] * Epi)
    Ed = Edxa[0] + Edxa[1] + Et + 3 * U * (np.abs(cf["dxa"][0]) + np.abs(cf["dxa"][1]) + np.abs(cf["t"]))
    th = fw["pi"] / ma
    Ef = 2 * np.abs(th) * Epi / ma + 5 * U * th * th + U * cf["f"]
    E = ma * cf["f"] * Ed + np.abs(cf["d"]) * ma * Ef + 2 * U * np.abs(cf["dz3"])
    sq_terms = cf["w_row"][:, None] * cf["df"] ** 2
    E_LBC = ((N * A + 3) * U * sq_terms.sum() + (Ew[:, None] * cf["df"] ** 2 + 2 * cf["w_row"][:, None] * np.abs(cf["df"]) * Epi).sum()) \
        / (Ng * A) + 2 * U * cf["L_BC"]
    pw = abs(cf["p_w"])
    first = cf["p_w"] * (-cf["minq"]).sum() / Ng
    E_Lpi = pw / Ng * ((N + 3) * U * np.abs(cf["minq"]).sum() + np.sum(Eq)) + (es + 6 * U) * abs(first) \
        + h["bc_coef"] * E_LBC + 2 * U * (abs(first) + h["bc_coef"] * cf["L_BC"])
    (W1, b1), (W2, b2), _ = la
    z1, e1 = FB.layer_bound(s64, W1, b1, FB.C_E2E)
    _, e2 = FB.layer_bound(np.maximum(z1, 0), W2, b2, FB.C_E2E, split=split, pad=pad(la))
    gb = FB.grad_bounds(tape, FB.C_E2E, split, "network.", edz3=E, ex={2: e1, 4: e1 @ np.abs(W2) + e2})
    return dict(stats=Bs, L_pi=E_Lpi, L_BC=E_LBC, dz3=E, grads=gb, Ee=Ee, Eadv=Eadv, near=near, near_apriori=apriori)


def clamp_side_resolved(cf, q32, stats0_32, Ng):
    """Rows whose side of the clamp's select in the kernel is known and is the closed form's: q32 [2][N] is the fp32 twin Q the
    forward kernel computes for these rows, from which e is formed here in fp32 the way the seed forms it (two divisions, expf);
    a row counts when that e is further from 100 than 64 ulp of it (expf implementations differ by a few) and lies on the fp64
    side.  This only chooses the branch the bound is written for; a row on the other side keeps the whole term in its bound."""
    q = np.minimum(np.asarray(q32[0], np.float32), np.asarray(q32[1], np.float32))
    m = np.float32(stats0_32) / np.float32(Ng)
    with np.errstate(over="ignore"):
        e32 = np.exp(np.float32(EXP_SCALE) * (q / m), dtype=np.float32)
    clear = np.abs(e32.astype(np.float64) - CLAMP) > 64 * U * CLAMP
    return clear & ((e32 <= CLAMP) == (cf["e"] <= CLAMP))
