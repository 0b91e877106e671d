"""CPU references of the DARA baseline (the reference's algo/offline_offline/dara.py), written from the algorithm:

  dara_cfg / classifier_params / g25_rows / g25_batch / step_noise   the config, weights, rows and (un-permuted) classifier noise
                   of the g25 fixtures (tests/golden/make_golden_dara.py)
  classifier_step  fp64 numpy restatement of one classifier update's loss and gradients (dara.py:131-144, :202-223): noisy inputs,
                   both heads' forwards, the double-softmax cross-entropy (aux_ref.double_softmax_ce_ref), the backward
                   (aux_ref.mlp3_backward_ref)
  ClassifierState  the two heads with ONE Adam over both (fp64), stepping through a fixture
  relabel          fp64 penalty of a noise-free pass (aux_ref.dara_penalty_ref) and the relabeled source rewards

Shapes: rows (s [N][S], a [N][A], s2 [N][S]) of [src | tar], labels 0 for row < n_src else 1; parameter dicts carry nn.Linear names
under the prefixes `sa_classifier.` / `sas_classifier.`.
"""
import numpy as np

import aux_ref as R
import golden_util as gu
import iql_ref as IR

VARIANTS = dict(default=dict(), eta2=dict(dara_eta=2.0), short=dict(max_step=8))
STEPS = dict(default=2, eta2=2, short=6)
HEADS = ("sa_classifier.", "sas_classifier.")
LAYERS = ("network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias", "network.4.weight", "network.4.bias")
# Classifier.parameters() order: what the reference's single optimizer and its state_dict enumerate
PARAM_ORDER = tuple(h + k for h in HEADS for k in LAYERS)


def dara_cfg(S, A, **over):
    """The keys the reference's DARA reads (config/mujoco/dara/*.yaml values; dara_eta comes from the command line)."""
    cfg = IR.iql_cfg(S, A, gaussian_noise_std=1.0, eta=0.1, dara_eta=0)
    cfg.update(over)
    return cfg


def eta_of(cfg):
    return cfg["dara_eta"] if cfg["dara_eta"] != 0 else cfg["eta"]


def classifier_params(S, A, seed_sa=703, seed_sas=704, c_scale=1.0):
    """Both heads as tests/golden/make_golden_dara.py generates them (output layers scaled by c_scale)."""
    pc = {}
    for pre, sd, n_in in ((HEADS[0], seed_sa, S + A), (HEADS[1], seed_sas, 2 * S + A)):
        p = gu.gi.mlp_params(sd, n_in, 2)
        p["network.4.weight"] = (p["network.4.weight"] * np.float32(c_scale)).astype(np.float32)
        p["network.4.bias"] = (p["network.4.bias"] * np.float32(c_scale)).astype(np.float32)
        pc.update({pre + k: v for k, v in p.items()})
    return pc


g25_rows, g25_batch = IR.g24_rows, IR.g24_batch


def step_noise(g, step):
    """(noise_sas, noise_sa) of a fixture step in the order of the UN-permuted rows src | tar: the reference adds row i of its
    draw to batch row perm[i]; the loss is a mean over rows, so the permutation itself drops out."""
    perm = np.asarray(g[f"s{step}_perm"])
    out = []
    for k in ("noise_sas", "noise_sa"):
        e = np.asarray(g[f"s{step}_{k}"])
        u = np.empty_like(e)
        u[perm] = e
        out.append(u)
    return tuple(out)


def head_weights(pc, pre):
    """(W1, W2, W3, b1, b2, b3) of one head, nn.Linear shapes, float64, with a leading member axis of 1 on the weights."""
    f = lambda k: np.asarray(pc[pre + k], np.float64)
    return (f("network.0.weight")[None], f("network.2.weight")[None], f("network.4.weight")[None],
            f("network.0.bias"), f("network.2.bias"), f("network.4.bias"))


def head_forward(pc, pre, x):
    W1, W2, W3, b1, b2, b3 = head_weights(pc, pre)
    x = np.asarray(x, np.float64)
    h1 = np.maximum(x @ W1[0].T + b1, 0)
    h2 = np.maximum(h1 @ W2[0].T + b2, 0)
    return dict(x=x, h1=h1, h2=h2, z=h2 @ W3[0].T + b3)


def inputs(rows, noise, std):
    """x_sas [N][2S+A], x_sa [N][S+A] with the noise added (noise None: the exact concatenation)."""
    s, a, s2 = [np.asarray(x, np.float64) for x in rows[:3]]
    x_sas, x_sa = np.concatenate([s, a, s2], 1), np.concatenate([s, a], 1)
    if noise is not None:
        x_sas = x_sas + std * np.asarray(noise[0], np.float64)
        x_sa = x_sa + std * np.asarray(noise[1], np.float64)
    return x_sas, x_sa


def classifier_step(pc, rows, noise, std, n_src=None, n_global=None):
    """fp64 loss and gradients of one classifier update.  Returns dict(loss_sa, loss_sas, grads {param name: array}, z_sa, z_sas,
    dz_sa, dz_sas, x_sa, x_sas)."""
    x_sas, x_sa = inputs(rows, noise, std)
    N = x_sas.shape[0]
    n_src = N // 2 if n_src is None else n_src
    lab = (np.arange(N) >= n_src).astype(np.int64)
    out = dict(grads={}, x_sas=x_sas, x_sa=x_sa)
    for pre, x, nm in ((HEADS[0], x_sa, "sa"), (HEADS[1], x_sas, "sas")):
        fw = head_forward(pc, pre, x)
        loss, dz, _ = R.double_softmax_ce_ref(fw["z"], lab)
        if n_global is not None:                               # the local share of a global mean
            loss, dz = loss * N / n_global, dz * N / n_global
        W1, W2, W3, _, _, _ = head_weights(pc, pre)
        gr = R.mlp3_backward_ref(W1, W2, W3, x, fw["h1"][None], fw["h2"][None], dz[None])
        for src, name in R.GRAD_KEYS:
            out["grads"][pre + name] = gr[src][0]
        out.update({"loss_" + nm: loss, "z_" + nm: fw["z"], "dz_" + nm: dz})
    return out


class ClassifierState(object):
    """Both heads in float64 and the ONE Adam over them (dara.py:192): a shared step count, torch's update rule."""

    def __init__(self, pc, lr):
        self.p = {k: np.asarray(v, np.float64).copy() for k, v in pc.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.t, self.lr = 0, lr

    def step(self, rows, noise, std):
        out = classifier_step(self.p, rows, noise, std)
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for k, g in out["grads"].items():
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(bc2) + 1e-8)
        return out


def relabel(pc, rows, n_src, eta):
    """(penalty [n_src], relabeled reward [N]) of a noise-free pass on the source rows (dara.py:281-292)."""
    x_sas, x_sa = inputs([np.asarray(x)[:n_src] for x in rows[:3]], None, 0.0)
    pen, raw = R.dara_penalty_ref(head_forward(pc, HEADS[1], x_sas)["z"], head_forward(pc, HEADS[0], x_sa)["z"])
    reward = np.asarray(rows[3], np.float64).reshape(-1).copy()
    reward[:n_src] += eta * pen
    return pen, reward, raw


# ---- per-element bounds of mobody_dara_classifier (gradient form) against fp64 --------------------------------------------------
U = 2.0 ** -24
TINY = 2.0 ** -120


def as_net(pc, pre):
    """One head under the `network.` prefix tests/f64_bounds.py and tests/actor_ref.py read (Policy's naming)."""
    return {"network." + k[len(pre):]: v for k, v in pc.items() if k.startswith(pre)}


def inputs32(rows, noise, std):
    """The kernel's own fp32 inputs: x = v + e * std, each operation rounded once (the library is built without contraction)."""
    s, a, s2 = [np.asarray(x, np.float32) for x in rows[:3]]
    x_sas, x_sa = np.concatenate([s, a, s2], 1), np.concatenate([s, a], 1)
    if noise is not None and std != 0:
        x_sas = x_sas + np.asarray(noise[0], np.float32) * np.float32(std)
        x_sa = x_sa + np.asarray(noise[1], np.float32) * np.float32(std)
    return x_sas.astype(np.float32), x_sa.astype(np.float32)


def head_reference(pc, pre, x, n_src, n_global):
    """fp64 forward, seed (BwdSeed mode 7), loss share and gradients of one head on the rows x, with the tape of grad_bounds."""
    import actor_ref as AR
    pn = as_net(pc, pre)
    fw = IR.net_forward(pn, "network.", x)
    N = len(x)
    lab = (np.arange(N) >= n_src).astype(np.int64)
    loss, dz, rows = R.double_softmax_ce_ref(fw["z3"], lab)
    dz, loss = dz * N / n_global, loss * N / n_global
    grads, tape = AR.actor_grads_ref(pn, x, fw, dz)
    return dict(pn=pn, fw=fw, lab=lab, loss=loss, dz=dz, rows=rows, grads=grads, tape=tape)


def head_bounds(ref, x, N, n_global, split):
    """Bounds of one head's loss share and gradients.  The forward error E_z of the two logits (f64_bounds.e2e_bound) reaches the
    seed through delta = z0 - z1 alone: p0 = sigma(delta), dp0 / d delta = p0 p1 <= 1/4; q0 = sigma(2 p0 - 1), dq0 / dp0 = 2 q0 q1
    <= 1/2; dz0 N = f(p0) = p0 p1 (g0 - g1) with |g0 - g1| = |q0 - q1 -+ 1| <= 1.47, so |f'| <= 1.47 + 1/4 and |d (dz N) / d delta|
    <= 0.43; the row loss -log q_label moves by at most (1 - q_label) 2 / 4 <= 0.37 per unit of delta.  Both are taken as 1/2.  On
    top come the row-wise roundings of ce_on_probs for an exact z (tests/test_hip_aux_rowwise.py: (32 u p + 6 u |t|) / N + 3 u |dz|
    per element, 39 u + N u mean|l| for the loss)."""
    import f64_bounds as FB
    la = FB.net_weights(ref["pn"], "network.")
    pad = np.maximum(la[0][1], 0).max()
    _, Ez = FB.e2e_bound(np.asarray(x, np.float64), la, FB.C_E2E, split, pad)
    Ed = Ez[:, 0] + Ez[:, 1]
    p = R.softmax2_ref(ref["fw"]["z3"])
    q = R.softmax2_ref(p)
    g = q.copy(); g[np.arange(N), ref["lab"]] -= 1.0
    t = g - (g * p).sum(-1, keepdims=True)
    Edz = 0.5 * Ed[:, None] / n_global + (32 * U * p + 6 * U * np.abs(t)) / n_global + 3 * U * np.abs(ref["dz"]) + TINY
    E_loss = (0.5 * Ed.sum() + N * U * np.abs(ref["rows"]).sum() + 39 * U * N) / n_global + 2 * U * abs(ref["loss"])
    Efull = np.zeros_like(ref["dz"]) + Edz
    gb = FB.grad_bounds(ref["tape"], FB.C_E2E, split, "network.", edz3=Efull, ex=IR._input_errors(la, np.asarray(x, np.float64), split))
    return dict(loss=E_loss, dz=Edz, grads=gb)
