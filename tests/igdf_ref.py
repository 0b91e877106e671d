"""CPU references of the IGDF baseline (the reference's algo/offline_offline/igdf.py), written from the algorithm:

  igdf_cfg / info_params / g26_rows    the config, encoder weights and rows of the g26 fixtures (tests/golden/make_golden_igdf.py)
  contrast / contrast_full   fp64 loss and gradients (with respect to the representations) of the in-batch contrastive loss of
                   update_info (igdf.py:427-440), in the 2n-1-row form the kernels use and in the reference's n^2-row form
  info_step / InfoState     fp64 restatement of one update_info step: both encoders' forwards, `contrast`, the backward
                   (aux_ref.mlp3_backward_ref), ONE Adam over both encoders
  scores / select_key / select / filter_batch   fp64 restatement of the data filter of train() (:494-524)
  train_step       iql_ref.train_step's fp32 restatement of IQL's three phases on the filtered batch with the row-weighted critic
                   loss (:468-479), and four mutants: 'unweighted_q' (plain mse), 'weighted_v' (the weights on V's loss too),
                   'descending' (kept rows in descending score order), 'lowest_k' (the k LOWEST scores kept)

Shapes: phi [n][Z], psi_tar [n][Z], psi_src [n-1][Z]; rows = (s, a, s2, r, nd); parameter dicts carry nn.Linear names under the
prefixes `encoder_sa.` / `encoder_ss.`.
"""
import numpy as np
import torch

import aux_ref as R
import golden_util as gu
import iql_ref as IR
from oracle import mobody_oracle as O

VARIANTS = dict(default=dict(), all=dict(xi=1.0), one=dict(xi=0.04, importance_weight=3.0), odd=dict(), short=dict(max_step=8))
BS = dict(default=32, all=32, one=32, odd=33, short=32)
STEPS = dict(default=2, all=2, one=2, odd=2, short=6)
INFO_STEPS = 3
ENCS = ("encoder_sa.", "encoder_ss.")
LAYERS = ("network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias", "network.4.weight", "network.4.bias")
PARAM_ORDER = tuple(h + k for h in ENCS for k in LAYERS)      # ContrastiveInfo.parameters() order
MUTANTS = ("unweighted_q", "weighted_v", "descending", "lowest_k")


def igdf_cfg(S, A, **over):
    """The keys the reference's IGDF reads (config/*/igdf/*.yaml values; info_update_step is 7000 there)."""
    cfg = IR.iql_cfg(S, A, info_update_step=INFO_STEPS, repr_dim=64, ensemble_size=1, repr_norm=False, repr_norm_temp=False,
                     ortho_init=False, output_gain="None", importance_weight=1.0, xi=0.75)
    cfg.update(over)
    return cfg


def kept_rows(bs, xi):
    return int(bs * float(xi))


def info_params(S, A, seed_sa, seed_ss, Z=64, scale=1.0):
    """Both encoders as tests/golden/make_golden_igdf.py generates them (output layers scaled by `scale`)."""
    p = {}
    for pre, sd, n_in in ((ENCS[0], seed_sa, S + A), (ENCS[1], seed_ss, S)):
        q = gu.gi.mlp_params(sd, n_in, Z)
        q["network.4.weight"] = (q["network.4.weight"] * np.float32(scale)).astype(np.float32)
        q["network.4.bias"] = (q["network.4.bias"] * np.float32(scale)).astype(np.float32)
        p.update({pre + k: v for k, v in q.items()})
    return p


g26_rows = IR.g24_rows


def enc_weights(p, pre):
    f = lambda k: np.asarray(p[pre + k], np.float64)
    return (f("network.0.weight")[None], f("network.2.weight")[None], f("network.4.weight")[None],
            f("network.0.bias"), f("network.2.bias"), f("network.4.bias"))


def enc_forward(p, pre, x):
    W1, W2, W3, b1, b2, b3 = enc_weights(p, pre)
    x = np.asarray(x, np.float64)
    h1 = np.maximum(x @ W1[0].T + b1, 0)
    h2 = np.maximum(h1 @ W2[0].T + b2, 0)
    return dict(x=x, h1=h1, h2=h2, z=h2 @ W3[0].T + b3)


# ---- the contrastive loss -------------------------------------------------------------------------------------------------------
def bce_logits(l, y):
    """binary_cross_entropy_with_logits, element-wise, in the stable form max(l, 0) - l y + log1p(exp(-|l|))."""
    l = np.asarray(l, np.float64)
    return np.maximum(l, 0) - l * y + np.log1p(np.exp(-np.abs(l)))


def sigmoid(l):
    l = np.asarray(l, np.float64)
    e = np.exp(-np.abs(l))
    return np.where(l >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def contrast(phi, psi_tar, psi_src):
    """(loss, dphi [n][Z], dpsi_tar [n][Z], dpsi_src [n-1][Z], logits [n][n]) of the 2n-1-row form."""
    phi, psi_tar, psi_src = [np.asarray(x, np.float64) for x in (phi, psi_tar, psi_src)]
    n = len(phi)
    logits = np.concatenate([(phi * psi_tar).sum(1, keepdims=True), phi @ psi_src.T], 1)
    y = np.zeros((n, n)); y[:, 0] = 1.0
    loss = bce_logits(logits, y).sum() / (n * n)
    G = sigmoid(logits) - y
    G[:, 0] = -sigmoid(-logits[:, 0])                                  # sigma(l) - 1 without the cancellation
    G /= n * n
    dphi = G[:, :1] * psi_tar + G[:, 1:] @ psi_src
    return loss, dphi, G[:, :1] * phi, G[:, 1:].T @ phi, logits


def contrast_full(enc_ss, phi, tar_s2, src_s2):
    """The reference's form (igdf.py:427-440): encoder_ss on all n^2 next states ss[i] = [tar_s2[i] | src_s2], logits[i][j] =
    phi_i . psi(ss[i][j]); `enc_ss` maps rows to (representations, a function taking their gradient to parameter gradients).
    Returns (loss, logits, dpsi [n][n][Z], G [n][n])."""
    phi = np.asarray(phi, np.float64)
    n = len(phi)
    ss = np.concatenate([np.asarray(tar_s2, np.float64)[:, None, :], np.broadcast_to(np.asarray(src_s2, np.float64)[None], (n, n - 1, src_s2.shape[1]))], 1)
    psi = enc_ss(ss.reshape(n * n, -1)).reshape(n, n, -1)
    logits = np.einsum("iz,ijz->ij", phi, psi)
    y = np.zeros((n, n)); y[:, 0] = 1.0
    loss = bce_logits(logits, y).sum() / (n * n)
    G = (sigmoid(logits) - y) / (n * n)
    return loss, logits, G[:, :, None] * phi[:, None, :], G


def info_step(p, tar_rows, src_s2):
    """fp64 loss and parameter gradients of one update_info step on tar (s, a, s2)[n] and src s2 [n-1]."""
    s, a, s2 = [np.asarray(x, np.float64) for x in tar_rows[:3]]
    n = len(s)
    fa = enc_forward(p, ENCS[0], np.concatenate([s, a], 1))
    fs = enc_forward(p, ENCS[1], np.concatenate([s2, np.asarray(src_s2, np.float64)], 0))
    loss, dphi, dpt, dps, logits = contrast(fa["z"], fs["z"][:n], fs["z"][n:])
    out = dict(loss=loss, grads={}, phi=fa["z"], psi=fs["z"], dphi=dphi, dpsi=np.concatenate([dpt, dps], 0), logits=logits)
    for pre, fw, dz in ((ENCS[0], fa, dphi), (ENCS[1], fs, out["dpsi"])):
        W1, W2, W3, _, _, _ = enc_weights(p, pre)
        gr = R.mlp3_backward_ref(W1, W2, W3, fw["x"], fw["h1"][None], fw["h2"][None], dz[None])
        for src, name in R.GRAD_KEYS:
            out["grads"][pre + name] = gr[src][0]
    return out


class InfoState(object):
    """Both encoders in float64 and the ONE Adam over them (igdf.py:407): a shared step count, torch's update rule."""

    def __init__(self, p, lr):
        self.p = {k: np.asarray(v, np.float64).copy() for k, v in p.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.t, self.lr = 0, lr

    def step(self, tar_rows, src_s2):
        out = info_step(self.p, tar_rows, src_s2)
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for k, g in out["grads"].items():
            self.m[k] = 0.9 * self.m[k] + 0.1 * g
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            self.p[k] = self.p[k] - (self.lr / bc1) * self.m[k] / (np.sqrt(self.v[k]) / np.sqrt(bc2) + 1e-8)
        return out


# ---- the data filter ------------------------------------------------------------------------------------------------------------
def scores(p, src_rows):
    """score_i = phi_i . psi_i / (|phi_i| |psi_i|) on the source rows (igdf.py:500-504), fp64."""
    s, a, s2 = [np.asarray(x, np.float64) for x in src_rows[:3]]
    phi = enc_forward(p, ENCS[0], np.concatenate([s, a], 1))["z"]
    psi = enc_forward(p, ENCS[1], s2)["z"]
    return (phi * psi).sum(1) / (np.linalg.norm(phi, axis=1) * np.linalg.norm(psi, axis=1))


def select_key(score):
    """The integer key of the selection's total order (csrc/igdf.hip igdf_key): grows with the float, -0 below +0, every
    non-finite score 0, below the most negative finite one."""
    u = np.asarray(score, np.float32).view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return np.where((u & 0x7F800000) == 0x7F800000, 0, key).astype(np.uint64)


def select(score, k, mutant=None):
    """Positions of the k largest scores in ascending order (argsort(score)[-k:]), ties to the lower index first."""
    order = np.argsort(select_key(score), kind="stable")
    if mutant == "lowest_k":
        return order[:k]
    kept = order[len(order) - k:]
    return kept[::-1] if mutant == "descending" else kept


def filter_batch(p, src_rows, tar_rows, k, iw, mutant=None):
    """(batch of N = k + n_tar rows [kept src | tar], w [N], score [n_src], kept [k])."""
    sc = scores(p, src_rows)
    kept = select(sc, k, mutant)
    batch = tuple(np.concatenate([np.asarray(x)[kept], np.asarray(y)], 0) for x, y in zip(src_rows, tar_rows))
    w = np.concatenate([np.exp(iw * sc[kept]), np.ones(len(tar_rows[0]))])
    return batch, w, sc, kept


# ---- IQL's three phases with the weighted critic loss ---------------------------------------------------------------------------
def train_step(st, batch, w, cfg, mutant=None):
    """iql_ref.train_step on the filtered batch with L_Q = mean(w (q1 - y)^2) + mean(w (q2 - y)^2) (igdf.py:478)."""
    s, a, s2, r, nd = [O.T(x) for x in batch]
    wt = torch.from_numpy(np.asarray(w, np.float32)).reshape(-1, 1)
    A = a.shape[1]
    req = lambda d: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    vp = req(st.v)
    with torch.no_grad():
        t1, t2 = IR.twin_q(st.q_targ, s, a)
        q_t = torch.min(t1, t2)
    adv = q_t - IR.mlp3(vp, s, "network.")
    lv = torch.abs(cfg["lam"] - (adv < 0).float()) * adv ** 2
    v_loss = torch.mean(wt * lv if mutant == "weighted_v" else lv)
    gv = O._grads(v_loss, vp)
    st.t["v"] += 1
    for k in st.v:
        O.adam_update(st.v[k], gv[k], st.m["v"][k], st.s["v"][k], st.t["v"], cfg["critic_lr"])
    qp = req(st.q)
    with torch.no_grad():
        y = r + nd * cfg["gamma"] * IR.mlp3(st.v, s2, "network.")
    q1, q2 = IR.twin_q(qp, s, a)
    wq = torch.ones_like(wt) if mutant == "unweighted_q" else wt
    q_loss = (wq * (q1 - y) ** 2).mean() + (wq * (q2 - y) ** 2).mean()
    gq = O._grads(q_loss, qp)
    st.t["q"] += 1
    for k in st.q:
        O.adam_update(st.q[k], gq[k], st.m["q"][k], st.s["q"][k], st.t["q"], cfg["critic_lr"])
    O.polyak(st.q_targ, st.q, cfg["tau"])
    ap = req(st.actor)
    wpi = torch.exp((cfg["temp"] * adv.detach()).double()).float().clamp(max=IR.CLAMP)
    pred = IR._Tanh32.apply(IR.mlp3(ap, s, "network.")[:, :A])
    pi_loss = torch.mean(wpi * (pred - a) ** 2)
    ga = O._grads(pi_loss, ap)
    st.t["actor"] += 1
    lr = IR.cosine_lr(cfg["actor_lr"], st.t["actor"], cfg["max_step"])
    for k in st.actor:
        O.adam_update(st.actor[k], ga[k], st.m["actor"][k], st.s["actor"][k], st.t["actor"], lr)
    return dict(v_loss=v_loss.detach(), q_loss=q_loss.detach(), pi_loss=pi_loss.detach(), adv=adv.detach().reshape(-1),
                grads=dict(v=gv, q=gq, actor=ga), lr=lr)
