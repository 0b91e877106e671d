"""Inputs, fp64 references and tolerances shared by tests/test_bosa_actor_ref.py (CPU) and tests/test_hip_bosa_actor.py (GPU): the cases
of the estimator's gradient (mobody_bosa_loglik_grad), of BOSA's actor phase (mobody_bosa_actor_forward / _backward) and of the
class's stage-2 call against the g28 fixtures.  Every reference is computed once and cached."""
import functools

import numpy as np

import bosa2_ref as B2
import bosa_ref as BR
import golden_util as gu
import wide_ref as WR

BETA = 0.5
VAE_SEED = 22                       # tests/test_bosa2_ref.py's: both clamp branches are reached on the fixture variants' rows
# (variant, num_samples, rows, max_action): rows = 2 bs of the variant and 33, so that n B is 99 and 330 and never a multiple of 64
LLG_CASES = [(tag, n, B, ma) for tag in ("tiny", "small", "pen") for n in (1, 3, 10) for B in (2 * BR.VARIANTS[tag][4], 33) for ma in (1.0, 2.0)]


def llg_id(c):
    return "%s-n%d-B%d-ma%g" % c


@functools.lru_cache(maxsize=None)
def llg_case(tag, n, B, ma):
    """(S, A, H, enc, dec, s, a, eps) in fp32; a is the point of evaluation, inside (-ma, ma)."""
    S, A, H, _, _ = BR.VARIANTS[tag]
    enc, dec = BR.vae_params(VAE_SEED, "policy", S, A, H)
    s, a, _ = BR.batch(4, S, A, B)
    eps = np.random.default_rng(n).standard_normal((B, n, 2 * A)).astype(np.float32)
    return S, A, H, enc, dec, s, (np.float32(ma) * a).astype(np.float32), eps


@functools.lru_cache(maxsize=None)
def llg_reference(tag, n, B, ma):
    """(dll_da [B, A], ll [B], extras) of tests/bosa2_ref.loglik_grad_action in fp64."""
    _, _, _, enc, dec, s, a, eps = llg_case(tag, n, B, ma)
    return B2.loglik_grad_action(enc, dec, s, a, eps, BETA, ma)


def llg_tolerances(d64, ll64, w64):
    """(dll_da: the project's gradient tolerance rtol 1e-5 / atol 1e-5 x max |dll_da|, ll: BR.estimator_tolerance); w64 [n, B]."""
    return 1e-5 * np.abs(d64) + 1e-5 * np.abs(d64).max(), BR.estimator_tolerance(ll64[None], w64[None])[0]


# ---- the actor phase: walker shapes, one row past one and past eight 32-row tiles -----------------------------------------------------
ACTOR_S, ACTOR_A, ACTOR_H, ACTOR_ROWS, ACTOR_N_SAMPLES, ACTOR_LAMDA = 17, 6, 72, (33, 257), 3, 0.25


@functools.lru_cache(maxsize=None)
def actor_case(N, ma=1.0, shift=0.0, qcut=0.0):
    """(actor state dict, twin-Q state dict, enc, dec, s [N, S], eps [N, n, Lz]).  shift: subtracted from critic_2's output bias, so that
    member 1 lies below member 0 on every row and a min-Q implementation differs.  qcut in (0, 1): critic_1's output bias is moved so
    that this fraction of the rows has q_0 < 0 -- without it every q_0 of these nets has one sign and -mean(q) / mean|q| is +-1."""
    S, A = ACTOR_S, ACTOR_A
    pa = gu.gi.mlp_params(611, S, A)
    pq = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(611 + j, S + A, 1).items()}
    pq["network2.network.4.bias"] = pq["network2.network.4.bias"] - np.float32(shift)
    if qcut:
        pq["network1.network.4.bias"] = pq["network1.network.4.bias"] - np.float32(np.quantile(actor_reference(N, ma, shift)[2]["q"], qcut))
    enc, dec = BR.vae_params(VAE_SEED, "policy", S, A, ACTOR_H)
    s = gu.gi.batch(612, max(N, 64), S, A)[0][:N]
    eps = np.random.default_rng(N).standard_normal((N, ACTOR_N_SAMPLES, 2 * A)).astype(np.float32)
    return pa, pq, enc, dec, s, eps


@functools.lru_cache(maxsize=None)
def actor_reference(N, ma=1.0, shift=0.0, lamda=ACTOR_LAMDA, dtype=np.float64, qcut=0.0):
    """(logs, actor gradient as a parameter dict, extras) of tests/bosa2_ref.actor_step."""
    pa, pq, enc, dec, s, eps = actor_case(N, ma, shift, qcut)
    return B2.actor_step(B2.twin_from_state_dict(pa, ("",)), B2.twin_from_state_dict(pq), enc, dec, s, eps, BETA, lamda, ma, dtype=dtype)


def pre_tanh_seed(ex, ma, dtype=np.float64):
    """d loss / d(pre-tanh) [N, A] per element, what the actor's backward is seeded with: dpi * max_action (1 - (pi / max_action)^2)."""
    ma = dtype(ma)
    return ex["dpi"] * ma * (1 - (ex["pi"] / ma) ** 2)


def seed_tolerance(d64):
    """Per element: rtol 1e-5 / atol 1e-5 x the largest entry."""
    return 1e-5 * np.abs(d64) + 1e-5 * np.abs(d64).max()


# ---- a stage-2 call of the class against g28 ---------------------------------------------------------------------------------------
def g28_setup(tag):
    """(g, cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed rows) as tests/test_bosa2_ref.py builds them."""
    g = gu.load("g28_bosa2_" + tag)
    S, A, H, E, bs = BR.VARIANTS[tag]
    seed, setting = int(g["seed"]), (float(g["log_std_bias"]), float(g["log_std_scale"]))
    cfg = BR.bosa_cfg(S, A, H, E, vae_iteration=0, epsilon_dyna_exp=float(g["epsilon_dyna_exp"]))
    vaes = BR.vae_params(seed, "policy", S, A, H, 1, *setting), BR.vae_params(seed + 50, "dynamics", S, A, H, E, *setting)
    actor_sd = gu.gi.mlp_params(seed + 1, S, A)
    q_sd = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(seed + 1 + j, S + A, 1).items()}
    src, tar = gu.gi.batch(501, 64, S, A), gu.gi.batch(502, 64, S, A)
    mixed = [np.concatenate([t_[:bs], s_[:bs]]) for s_, t_ in zip(src, tar)]
    mixed[4] = g["not_done"]
    return g, cfg, vaes, actor_sd, q_sd, mixed


def g28_noise(g, call):
    return {k: g["c%d_noise_%s" % (call, k)] for k in ("target", "dynamics", "policy") if "c%d_noise_%s" % (call, k) in g}


def scalar_terms(logs, cfg):
    """The sum of the magnitudes of the terms each logged scalar adds (its atol is 1e-5 x this), from the scalars themselves: a mean's
    magnitude stands in for the mean of magnitudes, which can only make the bound tighter."""
    coef, lam = cfg["conservation_coef"], cfg["lamda_policy"]
    t = dict(critic_mask_ratio=0.0, critic_cons_loss=abs(logs["critic_cons_loss"]))
    t["critic_loss"] = t["critic_td_loss"] = abs(logs["critic_td_loss"]) + coef * abs(logs["critic_cons_loss"])
    if "actor_loss" in logs:
        t.update(neg_log_beta_mean=abs(logs["neg_log_beta_mean"]), neg_log_beta_max=abs(logs["neg_log_beta_max"]), lamda_policy=0.0,
                 actor_loss=abs(logs["actor_loss"] - lam * logs["neg_log_beta_mean"]) + lam * abs(logs["neg_log_beta_mean"]))
    return t


def stage2_calls(tag, dtype=np.float64):
    """The four g28 calls composed from tests/bosa2_ref.py's pieces as stage2_call composes them; the state advances in fp64 and each
    call's scalars are evaluated in `dtype` on it.  Yields (call, logs in dtype, logs in fp64, state)."""
    g, cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed = g28_setup(tag)
    s, a, s2, r, nd = mixed
    st = B2.stage2_init(actor_sd, q_sd)
    ma = cfg["max_action"]
    for call in (1, 2, 3, 4):
        noise = g28_noise(g, call)
        st["total_it"] += 1
        tn = np.clip(np.asarray(noise["target"], np.float64) * cfg["expl_noise"], -cfg["noise_clip"], cfg["noise_clip"])
        mask, _ = B2.dyna_mask(*vae_dyn, s, a, s2, noise["dynamics"], cfg["vae_dyna_beta"], cfg["epsilon_dyna_exp"])
        out = {}
        for dt in (dtype, np.float64):
            y, _ = B2.critic_targets(st["critic_target"], st["actor_target"], s2, r, nd, tn, cfg["gamma"], ma, dtype=dt)
            logs, _, gq = B2.critic_step(st["critic"], s, a, y, mask, cfg["conservation_coef"], dtype=dt)
            out[dt] = dict(logs, critic_mask_ratio=mask.mean())
        st["tq"] += 1
        for k in WR.KEYS:
            st["critic"][k], st["mq"][k], st["vq"][k] = WR.adam(st["critic"][k], gq[k], st["mq"][k], st["vq"][k], st["tq"], cfg["critic_lr"])
        if st["total_it"] % cfg["update_interval"] == 0:
            for dt in (dtype, np.float64):
                alog, ga, _ = B2.actor_step(st["actor"], st["critic"], *vae_pol, s, noise["policy"], cfg["vae_policy_beta"], cfg["lamda_policy"], ma,
                                            dtype=dt)
                out[dt].update(alog)
            st["ta"] += 1
            for k in WR.KEYS:
                st["actor"][k], st["ma"][k], st["va"][k] = WR.adam(st["actor"][k], ga[k], st["ma"][k], st["va"][k], st["ta"], cfg["actor_lr"])
            st["critic_target"] = B2.polyak(st["critic_target"], st["critic"], cfg["tau"])
            st["actor_target"] = B2.polyak(st["actor_target"], st["actor"], cfg["tau"])
        yield call, {k: float(v) for k, v in out[dtype].items()}, {k: float(v) for k, v in out[np.float64].items()}, st
