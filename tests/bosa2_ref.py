"""fp64 NumPy restatement of BOSA's critic / actor stage (the reference's algo/offline_offline/bosa.py:570-634), written from
the algorithm.  It reuses tests/bosa_ref.py and tests/wide_ref.py: every net is a wide_ref parameter dict W1 b1 W2 b2 W3 b3 with a
leading member axis -- the twin-Q net has two members (critic_1, critic_2), the actor one (output max_action * tanh).

loglik_grad_action: the exact derivative of the policy VAE's importance-sampling estimator (bosa_ref.loglik, :72-105) with
respect to its action input, the VAE's parameters and the latent noise held fixed -- what autograd gives the actor loss's
`neg_log_beta` term (:615-619) per row.  With p_k = softmax_k(w_k) and var = beta / 4:

    d ll / d a  =  sum_k p_k (-(a - u_k) / var)                                        the direct term
                +  J_enc,a^T [ sum_k g_k  |  pass (sum_k g_k eps_k std + 1) ]          through the encoder's two heads
    g_k         =  dz_k - p_k z_k                                                      -z_k: the log p(z) term
    dz_k        =  J_dec,z^T [ p_k (a - u_k) / var * max_action (1 - (u_k / max_action)^2) ]     the decoder's seed, row k B + b

The `+ 1` is the derivative of -log q(z | x)'s sum of log std with respect to the pre-clamp log_std, weighted by sum_k p_k = 1;
(z - mean) / std = eps does not move.  `pass` is torch's clamp backward on [-4, 15], both ends inclusive.

critic_step (:570-607), actor_step (:610-629) and polyak (:632-634) follow the reference line by line; every function takes
dtype = np.float32 to evaluate the same expressions in single precision (what a correct fp32 kernel may differ by).
"""
import numpy as np

import bosa_ref as BR
import wide_ref as WR


def _fwd(p, x, tanh=False, ma=1.0):
    """(out, h1, h2) in the dtype of the operands; x [E, rows, in]."""
    h1 = np.maximum(np.einsum("erk,ekn->ern", x, p["W1"]) + p["b1"][:, None], 0)
    h2 = np.maximum(np.einsum("erk,ekn->ern", h1, p["W2"]) + p["b2"][:, None], 0)
    o = np.einsum("erk,ekn->ern", h2, p["W3"]) + p["b3"][:, None]
    return (ma * np.tanh(o) if tanh else o), h1, h2


def _cast(p, dtype):
    return {k: np.asarray(v, dtype) for k, v in p.items()}


def twin_from_state_dict(sd, prefixes=("network1.", "network2.")):
    """nn.Linear state dict(s) (`<prefix>network.{0,2,4}.{weight [out, in], bias}`) -> a parameter dict with one member per prefix."""
    g = lambda k, f: np.stack([f(np.asarray(sd[p + k])) for p in prefixes])
    return {"W1": g("network.0.weight", np.transpose), "b1": g("network.0.bias", np.asarray), "W2": g("network.2.weight", np.transpose),
            "b2": g("network.2.bias", np.asarray), "W3": g("network.4.weight", np.transpose), "b3": g("network.4.bias", np.asarray)}


def to_state_dict(p, prefixes=("network1.", "network2.")):
    """Inverse of twin_from_state_dict."""
    out = {}
    for m, pre in enumerate(prefixes):
        for i, k in ((1, 0), (2, 2), (3, 4)):
            out["%snetwork.%d.weight" % (pre, k)], out["%snetwork.%d.bias" % (pre, k)] = p["W%d" % i][m].T, p["b%d" % i][m]
    return out


def loglik_grad_action(enc, dec, s, a, eps, beta, max_action=1.0, dtype=np.float64):
    """Policy VAE.  eps [B, n, Lz] (the reference's layout).  Returns (dll_da [B, A], ll [B], extras)."""
    f = lambda t: np.asarray(t, dtype)
    encp, decp = _cast(enc, dtype), _cast(dec, dtype)
    s, a, eps = f(s), f(a), f(eps)
    B, n, Lz = eps.shape
    A, S = a.shape[1], s.shape[1]
    var, ma = dtype(beta / 4.0), dtype(max_action)
    x = np.concatenate([s, a], 1)[None]
    out, eh1, eh2 = _fwd(encp, x)
    mean, pre = out[0, :, :Lz], out[0, :, Lz:]
    std = np.exp(np.clip(pre, dtype(BR.LOG_STD_MIN), dtype(BR.LOG_STD_MAX)))
    epk = eps.transpose(1, 0, 2)                                                   # [n, B, Lz]
    z = mean[None] + std[None] * epk
    xd = np.concatenate([np.tile(s, (n, 1)), z.reshape(n * B, Lz)], 1)[None]       # row k B + b
    u, dh1, dh2 = _fwd(decp, xd, True, ma)
    u = u[0].reshape(n, B, A)
    sd, c = np.sqrt(var), dtype(BR.LOG_SQRT_2PI)
    ln = lambda v, mu, sg: -((v - mu) ** 2) / (2 * sg ** 2) - np.log(sg) - c
    w = ln(a[None], u, sd).sum(-1) + ln(z, dtype(0), dtype(1)).sum(-1) - ln(z, mean[None], std[None]).sum(-1)    # [n, B]
    mx = w.max(0, keepdims=True)
    ex = np.exp(w - mx)
    ll = (mx + np.log(ex.sum(0, keepdims=True)))[0] - dtype(np.log(n))
    p = ex / ex.sum(0, keepdims=True)                                              # [n, B]
    resid = (a[None] - u) / var                                                    # [n, B, A]
    direct = -(p[:, :, None] * resid).sum(0)
    seed = p[:, :, None] * resid * ma * (1 - (u / ma) ** 2)
    gd = WR.backward(decp, xd, dh1, dh2, seed.reshape(1, n * B, A), dtype=dtype)
    dz = gd["dx"][0, :, S:].reshape(n, B, Lz)
    g = dz - p[:, :, None] * z
    passes = (pre >= BR.LOG_STD_MIN) & (pre <= BR.LOG_STD_MAX)
    denc = np.concatenate([g.sum(0), np.where(passes, (g * epk * std[None]).sum(0) + 1, 0)], 1).astype(dtype)
    ge = WR.backward(encp, x, eh1, eh2, denc[None], dtype=dtype)
    dxa = ge["dx"][0, :, S:S + A]
    return direct + dxa, ll, dict(w=w, p=p, pre=pre, direct=direct, dxa=dxa, denc=denc)


def critic_targets(q_targ, actor_targ, s2, r, nd, noise, gamma, max_action=1.0, dtype=np.float64):
    """:570-578.  noise [N, A]: the clipped target noise, already scaled.  Returns (y [N], a' [N, A])."""
    f = lambda t: np.asarray(t, dtype)
    s2, ma = f(s2), dtype(max_action)
    a2 = np.clip(_fwd(_cast(actor_targ, dtype), s2[None], True, ma)[0][0] + f(noise), -ma, ma)
    qn = _fwd(_cast(q_targ, dtype), np.broadcast_to(np.concatenate([s2, a2], 1), (2, len(s2), s2.shape[1] + a2.shape[1])))[0][:, :, 0].min(0)
    return f(r).reshape(-1) + f(nd).reshape(-1) * dtype(gamma) * qn, a2


def critic_step(q, s, a, y, mask, coef, dtype=np.float64, c=None):
    """:580-605 on the mixed rows [tar | src] (the source rows are the second half): the losses, the seed d loss / d q_m[row] and the
    twin-Q gradient.  c (or None): the seed's per-row constants as a caller rounded them, in place of coef / bs on the source rows.
    Returns (dict critic_loss critic_td_loss critic_cons_loss, seed [2, N], gradients as a parameter dict)."""
    f = lambda t: np.asarray(t, dtype)
    qp, y, mask = _cast(q, dtype), f(y), f(mask)
    N = len(y)
    bs = N - N // 2
    x = np.broadcast_to(np.concatenate([f(s), f(a)], 1), (2, N, s.shape[1] + a.shape[1]))
    out, h1, h2 = _fwd(qp, x)
    qv = out[:, :, 0]                                                              # [2, N]
    td = sum((dtype(0.5) * mask * (qv[m] - y) ** 2).mean() for m in (0, 1))        # :596
    cons = qv[0, N // 2:].mean() + qv[1, N // 2:].mean()                           # :597
    c = np.where(np.arange(N) >= N // 2, dtype(coef) / dtype(bs), dtype(0)).astype(dtype) if c is None else f(c)
    seed = (2 * (mask / 2)[None] * (qv - y[None]) / dtype(N) + c[None]).astype(dtype)
    g = WR.backward(qp, x, h1, h2, seed[:, :, None], dtype=dtype)
    g.pop("dx")
    return dict(critic_loss=td + dtype(coef) * cons, critic_td_loss=td, critic_cons_loss=cons), seed, g


def actor_step(actor, q, enc, dec, s, eps, beta, lamda, max_action=1.0, dtype=np.float64):
    """:612-628.  pi = actor(s), q = critic_1(s, pi) (member 0), norm_q = 1 / mean |q| detached, neg_log_beta = -ll(s, pi);
    actor_loss = -norm_q mean(q) + lamda mean(neg_log_beta).  Returns (dict of the logged scalars, the actor's gradient, extras)."""
    f = lambda t: np.asarray(t, dtype)
    ap, s, ma = _cast(actor, dtype), f(s), dtype(max_action)
    N, S = s.shape
    q1 = {k: f(v)[:1] for k, v in q.items()}
    pi, h1, h2 = _fwd(ap, s[None], True, ma)
    x = np.concatenate([s, pi[0]], 1)[None]
    qo, g1, g2 = _fwd(q1, x)
    qv = qo[0, :, 0]
    norm_q = 1 / np.abs(qv).mean()
    dq_da = WR.backward(q1, x, g1, g2, np.ones((1, N, 1), dtype), dtype=dtype)["dx"][0, :, S:]
    dll_da, ll, _ = loglik_grad_action(enc, dec, s, pi[0], eps, beta, max_action, dtype)
    dpi = -norm_q / dtype(N) * dq_da - dtype(lamda) / dtype(N) * dll_da
    dz3 = (dpi * ma * (1 - (pi[0] / ma) ** 2))[None].astype(dtype)
    g = WR.backward(ap, s[None], h1, h2, dz3, dtype=dtype)
    g.pop("dx")
    logs = dict(actor_loss=-norm_q * qv.mean() + dtype(lamda) * (-ll).mean(), neg_log_beta_mean=(-ll).mean(), neg_log_beta_max=(-ll).max(),
                lamda_policy=lamda)
    return logs, g, dict(pi=pi[0], q=qv, norm_q=norm_q, dpi=dpi, ll=ll)


def polyak(target, online, tau):
    """soft_update (:632-634): target <- tau online + (1 - tau) target, in fp64."""
    return {k: tau * np.asarray(online[k], np.float64) + (1.0 - tau) * np.asarray(target[k], np.float64) for k in target}


def dyna_mask(enc, dec, s, a, s2, eps, beta, epsilon):
    """:583-590: (mask [N] as 0 / 1, min over members of the dynamics estimator's ll)."""
    lo = BR.loglik(enc, dec, "dynamics", s, a, s2, eps, beta)[0].min(0)
    return (lo > np.log(epsilon)).astype(np.float64), lo


# the cases of tests/test_hip_bosa_stage2.py's mode-9 check: walker shapes, rows one past one and past eight 32-row tiles
MODE9_S, MODE9_A, MODE9_ROWS, MODE9_COEF = 17, 6, (33, 257), 0.1
# the row edges at walker shapes (the smallest N, exact 32-row tiles, the product's 256, 1024 and one past it) and other widths at
# N = 65 (a narrow net, pen's A = 24, ant's S = 111): (N, (S, A)), tests/bosa_actor_cases.py's EDGE_CASES
MODE9_EDGE_CASES = [(N, (MODE9_S, MODE9_A)) for N in (2, 32, 64, 256, 1024, 1025)] + [(65, SA) for SA in ((11, 3), (45, 24), (111, 8))]


def mode9_params(SA=(MODE9_S, MODE9_A)):
    """The twin-Q state dict of the mode-9 cases at (S, A)."""
    import iql_ref as IR
    return IR.iql_params(SA[0], SA[1], 431, 16.0)[1]


def mode9_case(N, rows=None, SA=(MODE9_S, MODE9_A), seed=501):
    """(rows[:N] of the five batch arrays, q_next [N], w [N] = BOSA's mask / 2, c [N]: coef / source rows on the second half).
    rows None: the seeded batch at (S, A) = SA."""
    if rows is None:
        import golden_util as gu
        rows = gu.gi.batch(seed, max(N, 64), SA[0], SA[1])
    rows = [np.asarray(x[:N]) for x in rows]
    rng = np.random.default_rng(N)
    q_next = rng.standard_normal(N).astype(np.float32) * np.float32(3)
    w = (rng.random(N) < 0.6).astype(np.float32) * np.float32(0.5)
    c = np.zeros(N, np.float32)
    c[N // 2:] = np.float32(MODE9_COEF / (N - N // 2))
    return rows, q_next, w, c


def grad_tolerance(g64):
    """The project's gradient tolerance over a net: rtol 1e-5 with atol 1e-5 x the largest entry of any of its tensors."""
    scale = max(np.abs(v).max() for v in g64.values())
    return {k: 1e-5 * np.abs(v) + 1e-5 * scale for k, v in g64.items()}


# ---- a whole stage-2 call, composed from the pieces above (what tests/golden/make_golden_bosa2.py and its fixture test run) ----------
ACTOR_KEYS = ("actor", "actor_target")
CRITIC_KEYS = ("critic", "critic_target")


def stage2_init(actor_sd, q_sd):
    """The five nets from nn.Linear state dicts (`network.*` for the actor, `network1.* / network2.*` for the twin-Q; the targets are
    copies) and zeroed Adam moments / step counts."""
    actor, q = WR.f64(twin_from_state_dict(actor_sd, ("",))), WR.f64(twin_from_state_dict(q_sd))
    zeros = lambda p: {k: np.zeros_like(v) for k, v in p.items()}
    return dict(actor=actor, actor_target={k: v.copy() for k, v in actor.items()}, critic=q, critic_target={k: v.copy() for k, v in q.items()},
                mq=zeros(q), vq=zeros(q), ma=zeros(actor), va=zeros(actor), tq=0, ta=0, total_it=0)


def stage2_call(st, vae_pol, vae_dyn, mixed, noise, cfg):
    """One train() call of the critic / actor stage (:553, :565-634) on the mixed rows (s, a, s2, r, not_done), in place on `st`.
    noise: dict target [N, A] (raw normal draws), dynamics [n, E, N, Lz] and -- on an actor call -- policy [N, n, Lz].
    Returns the logged scalars plus mask [N] and min_ll [N]."""
    s, a, s2, r, nd = mixed
    st["total_it"] += 1
    ma = cfg["max_action"]
    tn = np.clip(np.asarray(noise["target"], np.float64) * cfg["expl_noise"], -cfg["noise_clip"], cfg["noise_clip"])
    y, _ = critic_targets(st["critic_target"], st["actor_target"], s2, r, nd, tn, cfg["gamma"], ma)
    mask, lo = dyna_mask(*vae_dyn, s, a, s2, noise["dynamics"], cfg["vae_dyna_beta"], cfg["epsilon_dyna_exp"])
    logs, _, g = critic_step(st["critic"], s, a, y, mask, cfg["conservation_coef"])
    logs = dict(logs, critic_mask_ratio=mask.mean())
    st["tq"] += 1
    for k in WR.KEYS:
        st["critic"][k], st["mq"][k], st["vq"][k] = WR.adam(st["critic"][k], g[k], st["mq"][k], st["vq"][k], st["tq"], cfg["critic_lr"])
    if st["total_it"] % cfg["update_interval"] == 0:
        alog, ga, ex = actor_step(st["actor"], st["critic"], *vae_pol, s, noise["policy"], cfg["vae_policy_beta"], cfg["lamda_policy"], ma)
        logs.update(alog)
        st["ta"] += 1
        for k in WR.KEYS:
            st["actor"][k], st["ma"][k], st["va"][k] = WR.adam(st["actor"][k], ga[k], st["ma"][k], st["va"][k], st["ta"], cfg["actor_lr"])
        st["critic_target"] = polyak(st["critic_target"], st["critic"], cfg["tau"])
        st["actor_target"] = polyak(st["actor_target"], st["actor"], cfg["tau"])
        logs["pi"] = ex["pi"]
    logs.update(mask=mask, min_ll=lo)
    return logs


STAGE2_SCALARS = ("critic_mask_ratio", "critic_loss", "critic_td_loss", "critic_cons_loss", "actor_loss", "neg_log_beta_mean", "neg_log_beta_max",
                  "lamda_policy")
