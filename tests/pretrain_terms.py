"""One loss term of a dynamics pre-training batch at a time, in fp64 (tests/test_pretrain_terms.py on the CPU,
tests/test_hip_pretrain_terms.py against csrc/pretrain.hip).

The gradient of the SUMMED loss hides its small terms: reconstruction is weighted 100x, the KL 0.05 / 16, the source
domain's reward loss 0.01x, and a tolerance of 1e-5 of a sub-network's largest gradient passes a wrong divisor in any of the
small ones.  `mobody_pretrain_grads` takes encoder_loss_coef / transition_coef / reward_coef and so does
oracle.dyn_learn_losses: a term is a coefficient triple, and each tensor is judged against the scale of THAT term alone.

  TERMS       name -> (encoder_loss_coef, transition_coef, reward_coef); "kl_latent" is "enc" with transition1.weight = 0, so
              that the decoder ignores its input and only the KL and latent-consistency terms reach zs* and za_*.
  GEOMETRIES  (S, A, b): every remainder of k_pre_za_reduce's 4-way unrolled chunk loop (nch = ceil(b / 8) in 1, 2, 3, 4, 9),
              an exact and a ragged last 8-row group, A > S (the action-copy loop of k_pre_trans_loss), Np3 > 2S (the
              padding-zero loops run more than once), and a wide state.
  rule_ratio  the acceptance rule of test_mopo_grads_vs_fp64_restatement: per tensor
              max|got - ref64| <= 3 max|ref32 - ref64| + 1e-6 max|ref64| + 1e-12.
  MUTANTS     one swapped expression of the restatement each, and the (term, geometry, domain) in which the rule sees it.
"""
import functools

import numpy as np
import torch

import golden_util as gu
from oracle import mobody_oracle as O

L = 16
TERMS = {"enc": (1.0, 0.0, 0.0), "trans": (0.0, 1.0, 0.0), "reward": (0.0, 0.0, 1.0), "all": (1.0, 1.0, 1.0),
         "kl_latent": (1.0, 0.0, 0.0)}
GEOMETRIES = [(17, 6, b) for b in (1, 7, 8, 9, 12, 23, 32, 65)] + [(5, 8, 23), (3, 1, 9), (111, 8, 12)]
NETS = {"zs": ("zs1", "zs2", "zs3"), "tr": ("transition1", "transition2", "transition3"),
        "rw": ("reward_model1", "reward_model2", "reward_model3")}

# mutant -> (term, geometry, use_trg) where the rule must reject it by more than 4x on some tensor
MUTANTS = {
    "std_biased": ("reward", (17, 6, 12), False),          # ensemble std divides by 7, not 6
    "std_detached": ("reward", (17, 6, 12), False),        # drops the k (m_e - avg) term of k_pre_fake_bwd
    "z4_grad": ("kl_latent", (17, 6, 12), False),          # z4 = encode_state(s') sampled WITH gradient
    "kl_half": ("kl_latent", (17, 6, 12), False),          # 0.05 / 2
    "kl_s2_dropped": ("kl_latent", (17, 6, 12), False),    # KL of s' missing
    "kl_exp_half": ("kl_latent", (17, 6, 12), False),      # exp(0.5 logvar) where exp(logvar) is meant
    "reward_src_factor_in_trg": ("reward", (17, 6, 12), True),   # 0.01 applied in the target domain
    "za_z3_for_z5": ("trans", (17, 6, 12), False),         # the action encoder of the transition loss fed z3
    "reward_act_tail_zeroed": ("reward", (5, 8, 23), False),     # action columns j >= S of the reward head's input left 0
    "recon_z2_unweighted": ("enc", (17, 6, 12), False),    # 100 x on the z1 reconstruction row only
}
# Against the summed-loss tolerance the suite had (full loss, source step, 1e-5 of the sub-network's largest gradient):
# these pass it (std_detached at 0.44 of the tolerance; the 0.01 mutant does not act on a source step at all) ...
OLD_TOLERANCE_BLIND = ("std_detached", "reward_src_factor_in_trg")
# ... and these do not, measured worst |diff| / tolerance at (17, 6, 12): std_biased 28 (reward_model3.weight -- the reward
# head sees the changed fake next state directly, at its own scale), kl_half 59, kl_s2_dropped 59, kl_exp_half 309 (zs3.bias).
OLD_TOLERANCE_SEES = ("std_biased", "kl_half", "kl_s2_dropped", "kl_exp_half")


def expected_nonzero(term, use_trg):
    """Layers whose gradient the term reaches (the reward head only through reward_coef; both losses of the reward term reach
    the encoder, the action encoder and the decoder through the fake next state)."""
    pre = "za_trg" if use_trg else "za_src"
    if term == "kl_latent":
        return list(NETS["zs"]) + [pre + "1", pre + "2"]
    names = list(NETS["zs"]) + list(NETS["tr"]) + [pre + "1", pre + "2"]
    return names + (list(NETS["rw"]) if term in ("reward", "all") else [])


def judged(term, name):
    """kl_latent is judged on the state encoder and the action encoders only (its decoder is a mutilated one)."""
    return term != "kl_latent" or name.startswith("zs") or name.startswith("za_")


@functools.lru_cache(maxsize=None)
def case_inputs(S, A, b, term):
    """(params, rows, noise) of a geometry: seeded, fp32 arrays.  Treat as read-only (shared between tests)."""
    p = gu.gi.dyn_params(300 + 7 * S + A, S, A)
    if term == "kl_latent":
        p = dict(p)
        p["transition1.weight"] = np.zeros_like(p["transition1.weight"])
    rows = gu.gi.pretrain_batch(400 + 13 * S + b, b, S, A)
    rng = np.random.default_rng(500 + 17 * S + b)
    noise = [rng.standard_normal((7, b, L)).astype(np.float32) for _ in range(6)] + \
            [rng.standard_normal((7, b, S)).astype(np.float32)]
    return p, rows, noise


def mutated_losses(p, obs, act, next_obs, rew, noise, use_trg, encoder_loss_coef, transition_coef, reward_coef, dtype, mutate,
                   aux=None):
    """oracle.dyn_learn_losses restated once more with one expression swapped (`mutate`, a key of MUTANTS; "none" = the
    oracle's own expressions, pinned equal to it by test_pretrain_terms).  aux (a dict) receives mean6 and its ensemble std."""
    T = O.T
    s, a, s2, r = T(obs, dtype), T(act, dtype), T(next_obs, dtype), T(rew, dtype)
    n = [T(x, dtype) for x in noise]
    pre = "za_trg" if use_trg else "za_src"

    def enc(x, eps):
        mu, lv = O.dyn_encode_state(p, x)
        return mu + eps * torch.exp(0.5 * lv), mu, lv

    def za(zs):
        g = O.swish(O._el(p, pre + "1", torch.cat([zs, a], -1)))
        return O._el(p, pre + "2", g)[..., :L]

    ckl = 0.025 if mutate == "kl_half" else 0.05
    var = (lambda lv: (0.5 * lv).exp()) if mutate == "kl_exp_half" else (lambda lv: lv.exp())
    kl = lambda mu, lv: ckl * (-0.5 * (1 + lv - mu.pow(2) - var(lv)).mean(dim=(1, 2))).sum()
    z1, mu1, lv1 = enc(s, n[0])
    z2, mu2, lv2 = enc(s2, n[1])
    rec1 = ((O.dyn_decode_transition(p, z1) - s) ** 2).mean(dim=(1, 2)).sum()
    rec2 = ((O.dyn_decode_transition(p, z2) - s2) ** 2).mean(dim=(1, 2)).sum()
    recon = rec1 + rec2
    kl_loss = kl(mu1, lv1) + (0.0 if mutate == "kl_s2_dropped" else kl(mu2, lv2))
    z3, _, _ = enc(s, n[2])
    if mutate == "z4_grad":
        z4, _, _ = enc(s2, n[3])
    else:
        with torch.no_grad():
            z4, _, _ = enc(s2, n[3])
    rec_w = 100 * rec1 + rec2 if mutate == "recon_z2_unweighted" else 100 * recon
    enc_loss = rec_w + kl_loss + (((z3 + za(z3)) - z4) ** 2).mean(dim=(1, 2)).sum()
    z5, _, _ = enc(s, n[4])
    trans = ((O.dyn_decode_transition(p, z5 + za(z3 if mutate == "za_z3_for_z5" else z5)) - s2) ** 2).mean(dim=(1, 2)).sum()
    loss = transition_coef * trans + (5 if use_trg else 1) * encoder_loss_coef * enc_loss
    z6, _, _ = enc(s, n[5])
    mean6 = O.dyn_decode_transition(p, z6 + za(z6))
    std = torch.std(mean6, dim=0, keepdim=True, unbiased=mutate != "std_biased")
    if aux is not None:
        aux["mean6"], aux["std"] = mean6.detach(), std.detach()
    fake = mean6 + n[6] * (std.detach() if mutate == "std_detached" else std)
    ar = a
    if mutate == "reward_act_tail_zeroed":
        ar = a.clone()
        ar[..., s.shape[-1]:] = 0
    rl = ((O.dyn_reward(p, s, ar, fake)[0] - r) ** 2).mean(dim=(1, 2)).sum() + \
         ((O.dyn_reward(p, s, ar, s2)[0] - r) ** 2).mean(dim=(1, 2)).sum()
    src_only = not use_trg or mutate == "reward_src_factor_in_trg"
    loss = loss + reward_coef * (0.01 * rl if src_only else rl)
    return loss, trans, enc_loss, recon, kl_loss


def term_grads(p, rows, noise, use_trg, coefs, dtype, b_global=None, mutate=None, aux=None):
    """Losses and gradients of one term under autograd: (losses5 float64 array, {`layer.weight|bias`: ndarray or None}).
    b_global: the local share of a data-parallel rank, i.e. everything scaled by b / b_global (include/mobody_hip.h)."""
    pr = {k: O.T(v, dtype).detach().clone().requires_grad_(True) for k, v in p.items()
          if k.split(".")[0] in O.TRAINED_LAYERS and k.split(".")[1] in ("weight", "bias")}
    if mutate is None:
        losses = O.dyn_learn_losses(pr, *rows, noise, use_trg, *coefs, dtype=dtype)
    else:
        losses = mutated_losses(pr, *rows, noise, use_trg, *coefs, dtype, mutate, aux)
    names = list(pr)
    gs = torch.autograd.grad(losses[0], [pr[k] for k in names], allow_unused=True)
    share = 1.0 if b_global is None else rows[0].shape[1] / float(b_global)
    grads = {k: (None if g is None else g.detach().double().numpy() * share if dtype == torch.float64 else
                 (g.detach() * torch.tensor(share, dtype=dtype)).numpy()) for k, g in zip(names, gs)}
    return np.array([float(x.detach()) for x in losses], np.float64) * share, grads


@functools.lru_cache(maxsize=None)
def reference(S, A, b, term, use_trg, b_global=None):
    """(losses64, grads64, grads32) of a case; computed once and shared (read-only) by every test and both MFMA modes."""
    p, rows, noise = case_inputs(S, A, b, term)
    l64, g64 = term_grads(p, rows, noise, use_trg, TERMS[term], torch.float64, b_global)
    _, g32 = term_grads(p, rows, noise, use_trg, TERMS[term], torch.float32, b_global)
    return l64, g64, g32


def fake_std(S, A, b, term, use_trg):
    """(mean6, std_e(mean6)) of a case in fp64: the operands of the fake next state."""
    p, rows, noise = case_inputs(S, A, b, term)
    aux = {}
    with torch.no_grad():
        mutated_losses(O.to_torch(p, torch.float64), *rows, noise, use_trg, *TERMS[term], torch.float64, "none", aux)
    return aux["mean6"], aux["std"]


def blob_view(name, g):
    """The part of a reference-layout gradient that the blob holds: za_*2 keeps its mu half only."""
    if g is not None and name.startswith("za_") and name.split(".")[0].endswith("2"):
        return g[..., :L]
    return g


def is_zero(g):
    return g is None or not np.any(g)


def rule_bound(ref64, ref32):
    ref64 = np.asarray(ref64, np.float64)
    return 3.0 * np.abs(np.asarray(ref32, np.float64) - ref64).max() + 1e-6 * np.abs(ref64).max() + 1e-12


def rule_ratio(got, ref64, ref32):
    """max|got - ref64| / bound of the acceptance rule (<= 1 passes).  A tensor whose fp64 gradient is None or all zero must
    be exactly zero: ratio 0 or inf."""
    got = np.asarray(got, np.float64)
    if is_zero(ref64):
        return 0.0 if not np.any(got) else np.inf
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref64).max() / rule_bound(ref64, ref32))


def old_tolerance_passes(got, want):
    """The summed-loss rule of test_pretrain_grads_vs_oracle_shapes: |got - want| <= 1e-5 max|g| of the tensor's sub-network
    + 1e-5 |want|, `want` the fp32 oracle's gradients."""
    sub = lambda k: k[:2]
    scale = {}
    for k, v in want.items():
        if v is not None:
            scale[sub(k)] = max(scale.get(sub(k), 0.0), float(np.abs(v).max()))
    for k, v in want.items():
        if v is None:
            continue
        if not (np.abs(np.asarray(got[k], np.float64) - v) <= 1e-5 * scale[sub(k)] + 1e-5 * np.abs(v)).all():
            return False
    return True
