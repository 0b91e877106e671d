"""CPU references of the IQL baseline (the reference's algo/offline_offline/iql.py), written from the algorithm:

  train_step       an fp32 torch restatement of one `IQL.train` step after the batch is assembled (V, Q + Polyak, policy under the
                   cosine learning rate, Adam), every linear layer, exp and tanh rounded to fp32 once (mlp3), checked against the
                   g24 fixtures; two mutants (max_action inside the policy loss,
                   the advantage of AFTER V's update)
  cosine_lr        the closed form of CosineAnnealingLR (eta_min 0) for 1-based gradient step k
  expectile_seed / awr_seed   fp64 numpy closed forms of what BwdSeed modes 5 and 6 (csrc/train.h) form row-wise
  value_bounds / policy_bounds   per-element error bounds of the two phases against fp64, conventions of tests/f64_bounds.py and
                   tests/actor_ref.py, extended by the error of expf, of tanhf and of 1 - th^2

Shapes: qt [2][N] target twin-Q(s, a), v [N], adv [N], z [N][2A] the policy's linear outputs (mu | logstd), act [N][A].
"""
import math

import numpy as np
import torch

import actor_ref as AR
import f64_bounds as FB
import golden_util as gu
from oracle import mobody_oracle as O

U = AR.U
TINY = AR.TINY
LN100 = AR.LN100
CLAMP = 100.0
VARIANTS = dict(default=dict(), lam09_temp10=dict(lam=0.9, temp=10.0), short=dict(max_step=8))
STEPS = dict(default=2, lam09_temp10=2, short=6)


def iql_cfg(S, A, **over):
    """The keys the reference's IQL reads (config/mujoco/iql/*.yaml values)."""
    cfg = dict(gamma=0.99, tau=0.005, update_interval=2, state_dim=S, action_dim=A, hidden_sizes=256, max_action=1.0,
               critic_lr=3e-4, actor_lr=3e-4, lam=0.7, temp=3.0, max_step=500000)
    cfg.update(over)
    return cfg


def iql_params(S, A, seed, q_scale=1.0):
    """Policy (S -> 2A), twin-Q and V parameter dicts (nn.Linear names) as tests/golden/make_golden_iql.py generates them."""
    pa = {"network." + k: v for k, v in gu.gi.mlp_params(seed, S, 2 * A).items()}
    pq = {}
    for j, sd in ((1, seed + 1), (2, seed + 2)):
        p = gu.gi.mlp_params(sd, S + A, 1)
        p["network.4.weight"] = (p["network.4.weight"] * np.float32(q_scale)).astype(np.float32)
        p["network.4.bias"] = (p["network.4.bias"] * np.float32(q_scale)).astype(np.float32)
        pq.update({f"network{j}." + k: v for k, v in p.items()})
    pv = {"network." + k: v for k, v in gu.gi.mlp_params(seed + 3, S, 1).items()}
    return pa, pq, pv


def g24_rows(S, A):
    return gu.gi.batch(501, 64, S, A), gu.gi.batch(502, 64, S, A)


def g24_batch(bs, S, A):
    """src(bs) | tar(bs), iql.py:208-215."""
    src, tar = g24_rows(S, A)
    return tuple(np.concatenate([x[:bs], y[:bs]], 0) for x, y in zip(src, tar))


def cosine_lr(lr0, k, T_max):
    """Learning rate of 1-based gradient step k under CosineAnnealingLR(T_max), eta_min 0 (double)."""
    return lr0 * (1.0 + math.cos(math.pi * (k - 1) / T_max)) / 2.0


class _Tanh32(torch.autograd.Function):
    """fp32 tanh and its derivative as the correctly rounded values (evaluated in double, rounded once): the vectorised fp32
    exp / tanh of the CPU differ by a unit in the last place between instruction sets, and the policy weight of a clamped row
    multiplies that by 100; rounded this way the restatement gives the same bits on every machine and stays within one unit of
    whatever the machine that wrote the fixtures computed."""

    @staticmethod
    def forward(ctx, z):
        th = torch.tanh(z.double())
        ctx.save_for_backward(th)
        return th.float()

    @staticmethod
    def backward(ctx, g):
        (th,) = ctx.saved_tensors
        return g * (1.0 - th * th).float()


def _lin(x, W, b):
    """One fp32 linear layer, evaluated in double and rounded once (forward and, through autograd, backward)."""
    return torch.nn.functional.linear(x.double(), W.double(), b.double()).float()


def mlp3(p, x, pre):
    """MLPNetwork (iql.py:50-63) on fp32 tensors with correctly rounded layers.  An fp32 matmul's last bits depend on the CPU's
    instruction set and BLAS blocking; exp(temp adv) turns a last-bit difference of a Q value of magnitude 10 into 1e-6 of a
    row's policy weight, which the G7 tolerances do not absorb on small, cancelling gradient entries.  Rounded this way the
    restatement computes the same bits on every machine, each op within half a unit of the exact result."""
    h = torch.relu(_lin(x, p[pre + "network.0.weight"], p[pre + "network.0.bias"]))
    h = torch.relu(_lin(h, p[pre + "network.2.weight"], p[pre + "network.2.bias"]))
    return _lin(h, p[pre + "network.4.weight"], p[pre + "network.4.bias"])


def twin_q(p, s, a):
    x = torch.cat([s, a], 1)
    return mlp3(p, x, "network1."), mlp3(p, x, "network2.")


# ---- fp32 restatement of the step ----------------------------------------------------------------------------------------
def train_step(st, batch, cfg, mutant=None):
    """One IQL.train step (iql.py:217-237) on the assembled batch; `st` is an oracle TrainState whose `actor` is the 2A-output
    policy.  mutant: 'max_action' (tanh(mu) * max_action inside the policy loss) or 'post_adv' (adv from the updated V)."""
    s, a, s2, r, nd = [O.T(x) for x in batch]
    A = a.shape[1]
    req = lambda d: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    mse = torch.nn.functional.mse_loss
    vp = req(st.v)
    with torch.no_grad():                                              # update_v_function :174-185
        t1, t2 = twin_q(st.q_targ, s, a)
        q_t = torch.min(t1, t2)
    adv = q_t - mlp3(vp, s, "network.")
    v_loss = torch.mean(torch.abs(cfg["lam"] - (adv < 0).float()) * adv ** 2)
    gv = O._grads(v_loss, vp)
    st.t["v"] += 1
    for k in st.v:
        O.adam_update(st.v[k], gv[k], st.m["v"][k], st.s["v"][k], st.t["v"], cfg["critic_lr"])
    qp = req(st.q)
    with torch.no_grad():                                              # update_q_functions :187-196
        y = r + nd * cfg["gamma"] * mlp3(st.v, s2, "network.")
    q1, q2 = twin_q(qp, s, a)
    q_loss = mse(q1, y) + mse(q2, y)
    gq = O._grads(q_loss, qp)
    st.t["q"] += 1
    for k in st.q:
        O.adam_update(st.q[k], gq[k], st.m["q"][k], st.s["q"][k], st.t["q"], cfg["critic_lr"])
    O.polyak(st.q_targ, st.q, cfg["tau"])
    ap = req(st.actor)
    adv_pi = adv.detach()
    if mutant == "post_adv":
        with torch.no_grad():
            adv_pi = q_t - mlp3(st.v, s, "network.")
    w = torch.exp((cfg["temp"] * adv_pi).double()).float().clamp(max=CLAMP)        # update_policy :198-202 (exp rounded once)
    pred = _Tanh32.apply(mlp3(ap, s, "network.")[:, :A])                            # bc_loss :91-95
    if mutant == "max_action":
        pred = pred * cfg["max_action"]
    pi_loss = torch.mean(w * (pred - a) ** 2)
    ga = O._grads(pi_loss, ap)
    st.t["actor"] += 1
    lr = cosine_lr(cfg["actor_lr"], st.t["actor"], cfg["max_step"])
    for k in st.actor:
        O.adam_update(st.actor[k], ga[k], st.m["actor"][k], st.s["actor"][k], st.t["actor"], lr)
    return dict(v_loss=v_loss.detach(), q_loss=q_loss.detach(), pi_loss=pi_loss.detach(), adv=adv.detach().reshape(-1),
                grads=dict(v=gv, q=gq, actor=ga), lr=lr)


# ---- fp64 closed forms of the two seeds -----------------------------------------------------------------------------------
def expectile_seed(qt, v, lam, Ng):
    """BwdSeed mode 5: adv, dz3[N] (column 0 of the one-output V net) and the three scalars."""
    qt, v = np.asarray(qt, np.float64), np.asarray(v, np.float64)
    adv = np.minimum(qt[0], qt[1]) - v
    w = np.abs(lam - (adv < 0))
    return dict(adv=adv, w=w, dz3=-2.0 * w * adv / Ng, L_V=float((w * adv * adv).sum() / Ng), adv_mean=float(adv.sum() / Ng),
                v_mean=float(v.sum() / Ng))


def awr_seed(z, act, adv, temp, Ng):
    """BwdSeed mode 6: dz3[N][2A] (columns >= A exactly 0), w, e = exp(temp adv) and L_pi."""
    z, act, adv = np.asarray(z, np.float64), np.asarray(act, np.float64), np.asarray(adv, np.float64)
    A = act.shape[1]
    th = np.tanh(z[:, :A])
    x = temp * adv
    with np.errstate(over="ignore"):
        e = np.exp(x)
    w = np.minimum(e, CLAMP)
    df, f = th - act, 1.0 - th * th
    dz3 = np.zeros_like(z)
    dz3[:, :A] = 2.0 * w[:, None] * df * f / (Ng * A)
    return dict(th=th, x=x, e=e, w=w, df=df, f=f, dz3=dz3, L_pi=float((w[:, None] * df * df).sum() / (Ng * A)))


# ---- fp64 forwards, robust rows ---------------------------------------------------------------------------------------------
def net_forward(p, pre, x):
    """fp64 z1, z2, z3 of one packed net (nn.Linear dict, prefix `pre`)."""
    (W1, b1), (W2, b2), (W3, b3) = FB.net_weights(p, pre)
    x = np.asarray(x, np.float64)
    z1 = x @ W1 + b1
    z2 = np.maximum(z1, 0) @ W2 + b2
    return dict(z1=z1, z2=z2, z3=np.maximum(z2, 0) @ W3 + b3)


def robust(p, pre, x, thr=2.0 ** -18):
    """Rows whose hidden pre-activations keep |z| above thr of their rounding scale (FB.robust_rows' rule, one net)."""
    ok = np.ones(len(x), bool)
    h = np.asarray(x, np.float64)
    for (W, b) in FB.net_weights(p, pre)[:2]:
        zz = h @ W + b
        ok &= (np.abs(zz) >= thr * (np.abs(h) @ np.abs(W) + np.abs(b))).all(1)
        h = np.maximum(zz, 0)
    return ok


def grads_ref(p, x, fw, dz3):
    """(gradients, tape) of a one-member net from its output gradient: AR.actor_grads_ref for any prefix-`network.` net."""
    return AR.actor_grads_ref(p, x, fw, dz3)


def _pad(L):
    return np.maximum(L[0][1], 0).max()


def _input_errors(la, x, split):
    (W1, b1), (W2, b2), _ = la
    z1, e1 = FB.layer_bound(x, W1, b1, FB.C_E2E)
    _, e2 = FB.layer_bound(np.maximum(z1, 0), W2, b2, FB.C_E2E, split=split, pad=_pad(la))
    return {2: e1, 4: e1 @ np.abs(W2) + e2}


def value_bounds(pv, pq_targ, s, a, lam, N, Ng, fw_v, cf, tape, split):
    """Per-element bounds of mobody_iql_value against fp64: adv [N], L_V, the two logged means, grads {name: bound}.
    adv = fminf(qt0, qt1) - v carries the forward bounds of both nets (min is 1-Lipschitz) and one rounding; the weight
    |lam - 1[adv < 0]| is exact once the sign of adv is (the caller keeps rows with |adv| above `adv` of this dict) up to the
    rounding of lam - 1; the seed -2 w adv inv_ng is three products and the rounded 1 / N_global."""
    s64, a64 = np.asarray(s, np.float64), np.asarray(a, np.float64)
    lv = FB.net_weights(pv, "network.")
    _, Ev = FB.e2e_bound(s64, lv, FB.C_E2E, split, _pad(lv))
    Eq = 0.0
    x = np.concatenate([s64, a64], 1)
    for pre in ("network1.", "network2."):
        lq = FB.net_weights(pq_targ, pre)
        Eq = np.maximum(Eq, FB.e2e_bound(x, lq, FB.C_E2E, split, _pad(lq))[1][:, 0])
    adv, w = cf["adv"], cf["w"]
    Eadv = Eq + Ev[:, 0] + U * np.abs(adv)
    Edz = 2.0 * w * Eadv / Ng + 6 * U * np.abs(cf["dz3"])
    E_L = ((N + 3) * U * (w * adv * adv).sum() + (2 * w * np.abs(adv) * Eadv + w * Eadv ** 2).sum() + 3 * U * (w * adv * adv).sum()) / Ng \
        + 2 * U * cf["L_V"]
    E_am = ((N + 3) * U * np.abs(adv).sum() + Eadv.sum()) / Ng + 2 * U * abs(cf["adv_mean"])
    vv = fw_v["z3"][:, 0]
    E_vm = ((N + 3) * U * np.abs(vv).sum() + Ev[:, 0].sum()) / Ng + 2 * U * abs(cf["v_mean"])
    gb = FB.grad_bounds(tape, FB.C_E2E, split, "network.", edz3=Edz[:, None], ex=_input_errors(lv, s64, split))
    return dict(adv=Eadv, L_V=E_L, adv_mean=E_am, v_mean=E_vm, dz3=Edz, grads=gb)


def weight_error(cf, temp):
    """Bound of fminf(expf(temp * adv), 100) for an exact fp32 adv: the product temp * adv rounds once (a relative |x| u of e),
    expf a few units in the last place, the clamp is 1-Lipschitz; below the normal range expf may flush."""
    d = (np.abs(cf["x"]) + 4) * U
    with np.errstate(invalid="ignore"):
        above = cf["e"] * (1.0 - d) >= CLAMP                                  # clamped whatever the rounding: exactly 100
    return np.where(above, 0.0, np.minimum(cf["e"], CLAMP) * d + TINY)


def clamp_unresolved(cf, temp):
    """Rows whose e lies within its own error of 100: either side of the clamp may be taken (the bound above covers both --
    the clamp is continuous -- but a test states how many such rows its inputs leave)."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(cf["e"]) & (np.abs(cf["e"] - CLAMP) <= cf["e"] * (np.abs(cf["x"]) + 4) * U)


def policy_bounds(pa, s, act, adv, temp, N, Ng, fw, cf, tape, split):
    """Per-element bounds of mobody_iql_actor (gradient form) against fp64: L_pi and grads {name: bound}.
    th = tanhf(z) of the kernel's own z (forward bound E_z; tanh' <= 1 - tanh^2(|z| - E_z) on that interval; tanhf 4 u),
    1 - th th (the square, the difference, twice |th| E_th), w (weight_error), v = 2 w df (1 - th^2) inv: four products and the
    rounded 1 / (N_global A)."""
    s64 = np.asarray(s, np.float64)
    A = act.shape[1]
    la = FB.net_weights(pa, "network.")
    _, Ez = FB.e2e_bound(s64, la, FB.C_E2E, split, _pad(la))
    z = fw["z3"][:, :A]
    Ez = Ez[:, :A]
    fmax = 1.0 - np.tanh(np.maximum(np.abs(z) - Ez, 0.0)) ** 2
    th, df, f, w = cf["th"], cf["df"], cf["f"], cf["w"][:, None]
    Eth = fmax * Ez + 4 * U * np.abs(th)
    Edf = Eth + U * np.abs(df)
    Ef = 2 * np.abs(th) * Eth + Eth ** 2 + U * th * th + U * f
    Ew = weight_error(cf, temp)[:, None]
    inv2 = 2.0 / (Ng * A)
    E = np.zeros_like(cf["dz3"])
    E[:, :A] = inv2 * (Ew * np.abs(df) * f + w * Edf * f + w * np.abs(df) * Ef + Ew * Edf * f + w * Edf * Ef) + 6 * U * np.abs(cf["dz3"][:, :A])
    terms = w * df * df
    E_L = ((N * A + 3) * U * terms.sum() + (Ew * df * df + 2 * w * np.abs(df) * Edf + w * Edf ** 2).sum() + 3 * U * terms.sum()) / (Ng * A) \
        + 2 * U * cf["L_pi"]
    gb = FB.grad_bounds(tape, FB.C_E2E, split, "network.", edz3=E, ex=_input_errors(la, s64, split))
    return dict(L_pi=E_L, dz3=E, grads=gb)
