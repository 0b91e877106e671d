"""fp64 references, in plain numpy, of the generic MLP gradient entry and of the auxiliary row-wise kernels
(tests/test_hip_aux_grad.py, tests/test_hip_aux_rowwise.py; each closed form is itself checked against torch.autograd in
tests/test_aux_ref.py).  Also the split-K row geometry of the weight-gradient launch and the input generators of the
exact-integer sweep, so that their preconditions can be checked without a GPU.

Shapes follow nn.Linear (mobody.py:35-48 MLPNetwork): W1 [M][256][in], W2 [M][256][256], W3 [M][out][256] for M members,
x [rows][in] shared by the members, h1 / h2 / dz [M][rows][256], dz3 [M][rows][out].
"""
import numpy as np

HID = 256
TWO24 = 2.0 ** 24


def _f64(a):
    return np.asarray(a, np.float64)


# ---- generic three-layer ReLU MLP backward (csrc/dara.hip mobody_mlp3_backward) ------------------------------------
def mlp3_backward_ref(W1, W2, W3, x, h1, h2, dz3):
    """Gradients of z3 = W3 relu(W2 relu(W1 x + b1) + b2) + b3 from dz3 and the saved post-ReLU activations, masks h > 0.
    Returns a dict of [M, ...] float64 arrays: dW1 db1 dW2 db2 dW3 db3 dz2 dz1, and under "abs_<name>" the same
    contraction over absolute values (sum |a| |b|), the scale every rounding-error bound is built from."""
    W1, W2, W3, x, h1, h2, dz3 = map(_f64, (W1, W2, W3, x, h1, h2, dz3))
    M = W2.shape[0]
    assert W1.shape[0] == M and W1.shape[2] == x.shape[1] and h1.shape == h2.shape == (M, x.shape[0], HID)
    out = {k: [] for k in ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dz2", "dz1")}
    out.update({"abs_" + k: [] for k in list(out)})
    ax = np.abs(x)
    for m in range(M):
        m2, m1 = h2[m] > 0, h1[m] > 0
        dz2 = (dz3[m] @ W3[m]) * m2                      # [rows,out] [out,256]
        a_dz2 = (np.abs(dz3[m]) @ np.abs(W3[m])) * m2
        dz1 = (dz2 @ W2[m]) * m1                         # h2pre = h1 W2^T  ->  dh1 = dz2 W2
        a_dz1 = (np.abs(dz2) @ np.abs(W2[m])) * m1
        ah1, ah2, adz3, adz2, adz1 = np.abs(h1[m]), np.abs(h2[m]), np.abs(dz3[m]), np.abs(dz2), np.abs(dz1)
        for k, v in (("dz2", dz2), ("abs_dz2", a_dz2), ("dz1", dz1), ("abs_dz1", a_dz1),
                     ("dW3", dz3[m].T @ h2[m]), ("abs_dW3", adz3.T @ ah2), ("db3", dz3[m].sum(0)), ("abs_db3", adz3.sum(0)),
                     ("dW2", dz2.T @ h1[m]), ("abs_dW2", adz2.T @ ah1), ("db2", dz2.sum(0)), ("abs_db2", adz2.sum(0)),
                     ("dW1", dz1.T @ x), ("abs_dW1", adz1.T @ ax), ("db1", dz1.sum(0)), ("abs_db1", adz1.sum(0))):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


GRAD_KEYS = (("dW1", "network.0.weight"), ("db1", "network.0.bias"), ("dW2", "network.2.weight"),
             ("db2", "network.2.bias"), ("dW3", "network.4.weight"), ("db3", "network.4.bias"))


# ---- split-K row geometry of the weight-gradient launch (csrc/train.h wgrad_nsplit, csrc/mlp_bwd.hip launch_wgrad) ----
def wgrad_nsplit(rows, members):
    cap = 32 if members == 1 else 16 if members == 2 else max(32 // members, 1)
    s = min(max(rows // (128 if members == 1 else 256), 1), cap)
    while rows > 2048 * 4 * s:
        s *= 2
    return s


def wgrad_geometry(rows, members):
    """nsplit, rows_per_wave, the (nrows, nblk, tail) of each of the 4 * nsplit wave slices as wgrad_tile forms them,
    and the set of named row-loop branches this row count takes."""
    ns = wgrad_nsplit(rows, members)
    rpw_raw = -(-rows // (4 * ns))
    rpw = (rpw_raw + 15) & ~15
    waves = []
    for g in range(4 * ns):
        n = max(0, min(rows, (g + 1) * rpw) - g * rpw)
        waves.append((n, n // 8, n % 8))
    b = set()
    for n, nblk, tail in waves:
        if n == 0:
            b.add("empty_wave")
            continue
        if nblk == 0:
            b.add("tail_only")                         # no whole block: only the masked pass
        if nblk == 1:
            b.add("one_block" if tail == 0 else "one_block_tail")      # `nblk & 1` pass, the pipeline loop does not run
        if nblk >= 2:
            b.add("pipeline")
            b.add("nblk_even" if nblk % 2 == 0 else "nblk_odd")        # even: block nblk-1 re-loaded and unused; odd: tail pass
        if nblk >= 1 and tail > 0:
            b.add("blocks_and_tail")
    if rpw != rpw_raw:
        b.add("rpw_rounded")
    for s in range(ns):
        if all(w[0] == 0 for w in waves[4 * s:4 * s + 4]):
            b.add("empty_slice")
    if any(w[0] == 1 for w in waves):
        b.add("one_row_wave")
    b.add("nsplit=%d" % ns)
    if ns > 1:
        b |= {x + "@split" for x in b if x in ("nblk_even", "nblk_odd")}
    if ns == (32 if members == 1 else 16 if members == 2 else max(32 // members, 1)):
        b.add("nsplit_cap")
    if rows % 32:
        b.add("bias_tile_ragged")
    return {"nsplit": ns, "rows_per_wave": rpw, "waves": waves, "branches": b, "ntiles": -(-rows // 32)}


# ---- generators of the exact-integer sweep -------------------------------------------------------------------------
def int_case(seed, in_dim, out_dim, members, rows):
    """Small-integer x, h1, h2, dz3 (h has entries <= 0 so that the masks bite) and sparse weights in {-1, 0, 1}: every
    partial sum of every output is an integer far below 2^24, so any fp32 summation order gives the same bits."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (rows, in_dim))
    h1 = rng.integers(-2, 5, (members, rows, HID))
    h2 = rng.integers(-2, 5, (members, rows, HID))
    dz3 = rng.integers(-2, 3, (members, rows, out_dim))
    sparse = lambda shape, p: rng.integers(-1, 2, shape) * (rng.random(shape) < p)
    W1 = sparse((members, HID, in_dim), 0.1)
    W2 = sparse((members, HID, HID), 4.0 / HID)
    W3 = sparse((members, out_dim, HID), min(1.0, 2.0 / out_dim))
    f = lambda a: a.astype(np.float32)
    return {"W1": f(W1), "W2": f(W2), "W3": f(W3), "x": f(x), "h1": f(h1), "h2": f(h2), "dz3": f(dz3)}


def int_exact_ok(ref):
    """The precondition of bit equality, from the reference alone: every sum of |a||b| below 2^24 and every value an integer."""
    worst = max(float(ref["abs_" + k].max()) for k in ("dz2", "dz1", "dW1", "db1", "dW2", "db2", "dW3", "db3"))
    whole = all(np.array_equal(ref[k], np.rint(ref[k])) for k in ("dz2", "dz1", "dW1", "db1", "dW2", "db2", "dW3", "db3"))
    return worst, whole and worst < TWO24


# ---- DARA classifier pieces (mobody.py:11-33, 146-181, 373-379) ----------------------------------------------------
def softmax2_ref(z):
    z = _f64(z)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def double_softmax_ce_ref(z, labels):
    """The reference's loss of one head: F.cross_entropy(Softmax(z), label) -- cross_entropy applies its own log_softmax to
    the head's probabilities -- mean over the N rows.  Returns (loss, dL/dz [N, 2], the per-row losses)."""
    z = _f64(z)
    lab = np.asarray(labels, np.int64)
    n = z.shape[0]
    p = softmax2_ref(z)
    q = softmax2_ref(p)
    rows = -np.log(q[np.arange(n), lab])
    g = q.copy()
    g[np.arange(n), lab] -= 1.0                         # dL/dp * N
    # through the head's softmax, p_i (g_i - sum_j g_j p_j), in its two-class form without the cancellation at p_i -> 1
    d0 = p[:, 0] * p[:, 1] * (g[:, 0] - g[:, 1]) / n
    dz = np.stack([d0, -d0], -1)
    return rows.sum() / n, dz, rows


def dara_loss_grad_ref(z_sas, z_sa, labels):
    """(loss_sa, loss_sas, dz_sas, dz_sa) as mobody_dara_loss_grad returns them."""
    l_sas, d_sas, _ = double_softmax_ce_ref(z_sas, labels)
    l_sa, d_sa, _ = double_softmax_ce_ref(z_sa, labels)
    return l_sa, l_sas, d_sas, d_sa


def dara_penalty_ref(z_sas, z_sa):
    """delta = clamp(log p~sas[1] - log p~sa[1] - log p~sas[0] + log p~sa[0], -10, 10), p~ = softmax(head probabilities) + 1e-10.
    Returns (delta, the value before the clamp)."""
    s = np.log(softmax2_ref(softmax2_ref(z_sas)) + 1e-10)
    u = np.log(softmax2_ref(softmax2_ref(z_sa)) + 1e-10)
    raw = s[:, 1] - u[:, 1] - s[:, 0] + u[:, 0]
    return np.clip(raw, -10.0, 10.0), raw


EXPECTILE = 0.7       # csrc/train.hip k_v_loss; the reference's update_v_function calls asymmetric_l2_loss(adv, 0.7), mobody.py:241


def value_loss_ref(qt, v, n_global, tau=EXPECTILE):
    """adv = min(Qt1, Qt2) - V; L = sum |tau - 1[adv < 0]| adv^2 / n_global.  Returns (loss, dL/dV [N]).
    At adv == 0 the indicator is 0 (the reference's `u < 0`), and the gradient is 0 on either side."""
    qt, v = _f64(qt), _f64(v)
    adv = np.minimum(qt[0], qt[1]) - v
    w = np.abs(tau - (adv < 0))
    return (w * adv * adv).sum() / n_global, -2.0 * w * adv / n_global


def par_penalty_ref(ns_true, ns_model, reward, coef):
    """reward - coef * mean_d (s'_true - s'_model)^2  (mobody.py:428-434).  Returns (reward, mean e^2)."""
    e = _f64(ns_true) - _f64(ns_model)
    mse = (e * e).mean(-1)
    return _f64(reward).reshape(-1) - coef * mse, mse
