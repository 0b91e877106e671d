"""fp64 NumPy restatement of BOSA's VAE stage (the reference's algo/offline_offline/bosa.py:23-133, :203-327, :516-550), written from
the algorithm: the VAE step's forward, loss and gradients for both VAEs, torch's Adam, and the importance-sampling estimator.

A VAE is two wide nets (tests/wide_ref.py), `enc` and `dec`, each a dict W1 b1 W2 b2 W3 b3 with a leading member axis; the encoder's
output columns [0, Lz) are the mean head, [Lz, 2 Lz) the log_std head.  kind 'policy': one member, Lz = 2 A, encoder on [s | a],
decoder on [s | z] with max_action * tanh, target a.  kind 'dynamics': E members, Lz = 2 S, encoder on [s | a | s'] (the same rows
for every member), decoder on [s | a | z_e], linear, target s'.
"""
import numpy as np

import wide_ref as WR

LOG_STD_MIN, LOG_STD_MAX = -4.0, 15.0
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def dims(kind, S, A):
    """(encoder in, latent, decoder in, decoder out)."""
    return (S + A, 2 * A, S + 2 * A, A) if kind == "policy" else (2 * S + A, 2 * S, 3 * S + A, S)


def vae_params(seed, kind, S, A, hidden, members=1, log_std_bias=-4.0, log_std_scale=2.0):
    """Seeded fp32 parameters, weights scaled by 1 / sqrt(fan_in); the log_std head's weights are scaled by log_std_scale and its
    bias moved by log_std_bias, so that pre-clamp values fall on both sides of -4."""
    ein, Lz, din, dout = dims(kind, S, A)
    E = 1 if kind == "policy" else members
    enc, dec = WR.params(seed, ein, hidden, 2 * Lz, E), WR.params(seed + 1, din, hidden, dout, E)
    enc["W3"][:, :, Lz:] *= np.float32(log_std_scale)
    enc["b3"][:, Lz:] += np.float32(log_std_bias)
    return enc, dec


def enc_input(kind, s, a, s2):
    return np.concatenate([s, a] if kind == "policy" else [s, a, s2], axis=1).astype(np.float64)


def encode(enc, kind, s, a, s2):
    """(mean, pre-clamp log_std, std, x, h1, h2), each [E, B, .]."""
    x = enc_input(kind, s, a, s2)
    out, h1, h2 = WR.forward(enc, x)
    Lz = out.shape[2] // 2
    mean, pre = out[:, :, :Lz], out[:, :, Lz:]
    return mean, pre, np.exp(np.clip(pre, LOG_STD_MIN, LOG_STD_MAX)), x, h1, h2


def dec_input(kind, s, a, z):
    """[E, rows, in]: the batch's own tensors repeat every B rows (rows = copies * B)."""
    E, rows, _ = z.shape
    rep = lambda t: np.broadcast_to(np.tile(np.asarray(t, np.float64), (rows // t.shape[0], 1)), (E, rows, t.shape[1]))
    return np.concatenate([rep(s), z] if kind == "policy" else [rep(s), rep(a), z], axis=2)


def vae_step(enc, dec, kind, s, a, s2, eps, beta, max_action=1.0):
    """One VAE training step's forward and backward (vae_policy_train / vae_dyna_train, :516-550).  eps [E, B, Lz].
    Returns (losses (recon, KL, loss), gradients (genc, gdec) as parameter dicts, extras)."""
    mean, pre, std, x, h1, h2 = encode(enc, kind, s, a, s2)
    E, B, Lz = mean.shape
    z = mean + std * np.asarray(eps, np.float64)
    xd = dec_input(kind, s, a, z)
    u, g1, g2 = WR.forward(dec, xd, "tanh" if kind == "policy" else "raw", max_action)
    target = np.asarray(a if kind == "policy" else s2, np.float64)[None]
    recon = ((u - target) ** 2).mean()
    kl = -0.5 * (1.0 + np.log(std ** 2) - mean ** 2 - std ** 2).mean()
    du = 2.0 * (u - target) / u.size
    dz3 = du * max_action * (1.0 - (u / max_action) ** 2) if kind == "policy" else du
    gdec = WR.backward(dec, xd, g1, g2, dz3)
    dz = gdec.pop("dx")[:, :, -Lz:]
    n = mean.size
    passes = (pre >= LOG_STD_MIN) & (pre <= LOG_STD_MAX)                      # torch's clamp backward: both ends inclusive
    denc = np.concatenate([dz + beta * mean / n, np.where(passes, dz * eps * std + beta * (std ** 2 - 1.0) / n, 0.0)], axis=2)
    genc = WR.backward(enc, x, h1, h2, denc)
    genc.pop("dx")
    return (recon, kl, recon + beta * kl), (genc, gdec), dict(mean=mean, pre=pre, std=std, z=z, u=u, dz=dz, denc=denc)


def reparam(encout, eps, beta, dz=None):
    """The row-wise piece alone: encout [n, 2 Lz], eps [n, Lz] -> (z, KL, d(L + beta KL)/d encout or None)."""
    encout, eps = np.asarray(encout, np.float64), np.asarray(eps, np.float64)
    Lz = eps.shape[1]
    mean, pre = encout[:, :Lz], encout[:, Lz:]
    std = np.exp(np.clip(pre, LOG_STD_MIN, LOG_STD_MAX))
    z = mean + std * eps
    kl = -0.5 * (1.0 + np.log(std ** 2) - mean ** 2 - std ** 2).mean()
    if dz is None:
        return z, kl, None
    dz, n = np.asarray(dz, np.float64), mean.size
    passes = (pre >= LOG_STD_MIN) & (pre <= LOG_STD_MAX)
    return z, kl, np.concatenate([dz + beta * mean / n, np.where(passes, dz * eps * std + beta * (std ** 2 - 1.0) / n, 0.0)], axis=1)


def log_normal(x, mu, sd):
    return -((x - mu) ** 2) / (2.0 * sd ** 2) - np.log(sd) - LOG_SQRT_2PI


def loglik(enc, dec, kind, s, a, s2, eps, beta, max_action=1.0):
    """importance_sampling_estimator (:72-105, :257-298).  eps in the reference's layout: [B, n, Lz] (policy) or [n, E, B, Lz]
    (dynamics).  Returns (ll [E, B], w [E, n, B])."""
    mean, pre, std, _, _, _ = encode(enc, kind, s, a, s2)
    E, B, Lz = mean.shape
    eps = np.asarray(eps, np.float64)
    eps = eps.transpose(1, 0, 2)[:, None] if kind == "policy" else eps               # -> [n, E, B, Lz]
    n = eps.shape[0]
    z = mean[None] + std[None] * eps
    xd = dec_input(kind, s, a, z.transpose(1, 0, 2, 3).reshape(E, n * B, Lz))          # row s B + b
    u = WR.forward(dec, xd, "tanh" if kind == "policy" else "raw", max_action)[0].reshape(E, n, B, -1)
    x = np.asarray(a if kind == "policy" else s2, np.float64)
    w = (log_normal(x[None, None], u, np.sqrt(beta / 4.0)).sum(-1) + log_normal(z, 0.0, 1.0).sum(-1).transpose(1, 0, 2)
         - log_normal(z, mean[None], std[None]).sum(-1).transpose(1, 0, 2))
    mx = w.max(1, keepdims=True)
    return (mx + np.log(np.exp(w - mx).sum(1, keepdims=True)))[:, 0] - np.log(n), w


def batch(seed, S, A, B):
    """Seeded fp32 (state, action in (-1, 1), next_state) rows."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(B, S), np.tanh(f(B, A)), f(B, S)


def estimator_case(kind, S, A, E, B, n):
    """The estimator tests' inputs: (s, a, s2, eps in the reference's layout, far).  Row `far` has its target far from any
    decoding, so every w of it lies below -1e4."""
    s, a, s2 = batch(9, S, A, B)
    far = B - 1
    if kind == "policy":
        a[far] = 60.0
    else:
        s2[far] = 60.0
    Lz = dims(kind, S, A)[1]
    eps = np.random.default_rng(n).standard_normal((B, n, Lz) if kind == "policy" else (n, E, B, Lz)).astype(np.float32)
    return s, a, s2, eps, far


def estimator_tolerance(ll64, w64):
    """rtol 1e-5 with atol 1e-5 x max_s |w_s| of the row, [E, B]."""
    return 1e-5 * np.abs(ll64) + 1e-5 * np.abs(w64).max(1)


def mask_threshold(ll64, tol):
    """A log_eps for the mask test: the middle of the widest gap between neighbouring fp64 minima over members around their
    median.  Returns (threshold, gap, the larger tolerance of the two rows on either side of the gap); the test is meaningful
    only where the gap exceeds ten times that tolerance."""
    order = np.argsort(ll64.min(0))
    lo64 = ll64.min(0)[order]
    mid = len(lo64) // 2
    cand = range(max(mid - 3, 0), min(mid + 3, len(lo64) - 1))
    j = max(cand, key=lambda i: lo64[i + 1] - lo64[i])
    return 0.5 * (lo64[j] + lo64[j + 1]), lo64[j + 1] - lo64[j], tol[:, order[j:j + 2]].max()


# shapes whose B crosses the estimator's workgroup boundaries (k_bosa_ll_reduce: one thread per row, 256 per workgroup;
# k_bosa_mask_mean: a 256-strided loop): name -> ((S, A, hidden, members, B), num_samples)
LL_BOUNDARY_CASES = {"tiny-b257": ((3, 1, 8, 1, 257), 64), "small-b513": ((17, 6, 72, 2, 513), 4), "odd-b300": ((17, 6, 72, 5, 300), 2)}
# the VAE step (dynamics) with more than 256 per-workgroup partial sums of both losses: 5 x 300 x 90 latent elements = 528
# partial sums, 5 x 300 x 45 output elements = 264 (k_bosa_finish's strided loops take a second trip past 256)
VAE_BOUNDARY_SHAPE = (45, 24, 72, 5, 300)
# its parameter seed: of 135 000 pre-clamp log_std values some fall within 1e-5 of -4 at most seeds, where the kernel's fp32 gate
# and the restatement's could differ; at this one the nearest is 2.2e-5 away in the step whose gradients are compared (asserted in
# tests/test_bosa_ref.py)
VAE_BOUNDARY_SEED = 22



NET_KEYS = ("encoder_shared.0", "encoder_shared.2", "mean", "log_std", "decoder.0", "decoder.2", "decoder.4")


def state_dict(enc, dec, kind):
    """The two nets as the reference module's state_dict (NumPy): VAE_Policy's nn.Linear keys (`.weight [out, in]`, `.bias`) or
    VAE_Dynamics_Ensemble's EnsembleFC keys (`.W [E, in, out]`, `.b [E, 1, out]`), in the module's parameter order."""
    Lz = enc["W3"].shape[2] // 2
    parts = [("encoder_shared.0", enc["W1"], enc["b1"]), ("encoder_shared.2", enc["W2"], enc["b2"]),
             ("mean", enc["W3"][:, :, :Lz], enc["b3"][:, :Lz]), ("log_std", enc["W3"][:, :, Lz:], enc["b3"][:, Lz:]),
             ("decoder.0", dec["W1"], dec["b1"]), ("decoder.2", dec["W2"], dec["b2"]), ("decoder.4", dec["W3"], dec["b3"])]
    sd = {}
    for name, W, b in parts:
        if kind == "policy":
            sd[name + ".weight"], sd[name + ".bias"] = np.ascontiguousarray(W[0].T), np.ascontiguousarray(b[0])
        else:
            sd[name + ".W"], sd[name + ".b"] = np.ascontiguousarray(W), np.ascontiguousarray(b[:, None, :])
    return sd


def from_state_dict(sd, kind):
    """Inverse of state_dict: (enc, dec) parameter dicts."""
    g = {}
    for name in NET_KEYS:
        if kind == "policy":
            g[name] = (np.asarray(sd[name + ".weight"]).T[None], np.asarray(sd[name + ".bias"])[None])
        else:
            g[name] = (np.asarray(sd[name + ".W"]), np.asarray(sd[name + ".b"])[:, 0])
    cat = lambda a, b, ax: np.concatenate([a, b], axis=ax)
    enc = dict(W1=g["encoder_shared.0"][0], b1=g["encoder_shared.0"][1], W2=g["encoder_shared.2"][0], b2=g["encoder_shared.2"][1],
               W3=cat(g["mean"][0], g["log_std"][0], 2), b3=cat(g["mean"][1], g["log_std"][1], 1))
    dec = dict(W1=g["decoder.0"][0], b1=g["decoder.0"][1], W2=g["decoder.2"][0], b2=g["decoder.2"][1], W3=g["decoder.4"][0], b3=g["decoder.4"][1])
    return enc, dec


# fixture variants (tests/golden/make_golden_bosa.py): name -> (S, A, hidden, members, batch_size); the mixed batch has 2 bs rows
VARIANTS = {"small": (17, 6, 72, 2, 8), "odd": (17, 6, 72, 5, 33), "tiny": (3, 1, 8, 1, 2), "pen": (45, 24, 72, 2, 4)}


def bosa_cfg(S, A, hidden, members, **over):
    """The reference's config/mujoco/bosa/walker2d.yaml, at a fixture variant's shape."""
    c = dict(batch_size=128, actor_lr=3e-4, critic_lr=3e-4, gamma=0.99, state_dim=S, action_dim=A, hidden_sizes=256, max_action=1.0, tau=0.005,
             update_interval=2, expl_noise=0.2, noise_clip=0.5, vae_policy_lr=1e-3, vae_policy_hidden_dim=hidden, vae_policy_beta=0.5,
             vae_dyna_lr=1e-3, vae_dyna_ensemble=members, vae_dyna_hidden_dim=hidden, vae_dyna_beta=0.5, vae_iteration=100000, lamda_policy=0.1,
             lamda_dyna=0.1, epsilon_policy_exp=0.01, epsilon_dyna_exp=0.01, conservation_coef=0.1, num_samples=1)
    c.update(over)
    return c
