"""fp64 NumPy restatement of the packed wide MLP (csrc/wide.hip), written from the algorithm: in -> hidden -> hidden ->
out with ReLU on both hidden layers, `members` independent copies, its gradients and torch's Adam.  Parameters are a dict
W1 [E, in, H], b1 [E, H], W2 [E, H, H], b2 [E, H], W3 [E, H, out], b3 [E, out] (EnsembleFC's orientation, bosa.py:176-200).
"""
import numpy as np

U = 2.0 ** -24
KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")

# (in_dim, out_dim) of BOSA's four nets (bosa.py:38-55, :218-235) at the walker (S = 17, A = 6) and pen (S = 45, A = 24) shapes
NET_SHAPES = {"walker": {"pol_enc": (23, 24), "pol_dec": (29, 6), "dyn_enc": (40, 68), "dyn_dec": (57, 17)},
              "pen": {"pol_enc": (69, 96), "pol_dec": (93, 24), "dyn_enc": (114, 180), "dyn_dec": (159, 45)}}


def params(seed, in_dim, hidden, out_dim, members, bias_scale=0.1):
    """Seeded fp32 parameters: weights N(0, 1) / sqrt(fan_in), biases N(0, bias_scale^2)."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (k, n) in enumerate(((in_dim, hidden), (hidden, hidden), (hidden, out_dim)), 1):
        p["W%d" % i] = (rng.standard_normal((members, k, n)) / np.sqrt(k)).astype(np.float32)
        p["b%d" % i] = (bias_scale * rng.standard_normal((members, n))).astype(np.float32)
    return p


def f64(p):
    return {k: np.asarray(v, np.float64) for k, v in p.items()}


def bcast(x, members):
    """[rows, w] or [E, rows, w] -> [E, rows, w] in fp64."""
    x = np.asarray(x, np.float64)
    return np.broadcast_to(x, (members,) + x.shape[-2:]) if x.ndim == 2 else x


def layer(x, W, b):
    """One layer's pre-activation [E, rows, out] and the companion sum |x| |W| + |b| of the sequential-sum error bound."""
    return np.einsum("erk,ekn->ern", x, W) + b[:, None, :], np.einsum("erk,ekn->ern", np.abs(x), np.abs(W)) + np.abs(b)[:, None, :]


def forward(p, x, out_mode="raw", max_action=1.0):
    """(out, h1, h2), everything fp64."""
    p = f64(p)
    x = bcast(x, p["W1"].shape[0])
    h1 = np.maximum(layer(x, p["W1"], p["b1"])[0], 0.0)
    h2 = np.maximum(layer(h1, p["W2"], p["b2"])[0], 0.0)
    z = layer(h2, p["W3"], p["b3"])[0]
    return (max_action * np.tanh(z) if out_mode == "tanh" else z), h1, h2


def backward(p, x, h1, h2, dz3):
    """Gradients (dict as the parameters, plus "dx" [E, rows, in]) from the gradient dz3 of the last layer's pre-activation
    and the forward's activations; the ReLU masks are h > 0 of the activations GIVEN (the kernel's own saves in the tests, so
    that a pre-activation within rounding of 0 cannot flip a unit between the two computations)."""
    p = f64(p)
    E = p["W1"].shape[0]
    x, h1, h2, dz3 = bcast(x, E), np.asarray(h1, np.float64), np.asarray(h2, np.float64), np.asarray(dz3, np.float64)
    g = {"W3": np.einsum("erk,ern->ekn", h2, dz3), "b3": dz3.sum(1)}
    dz2 = np.einsum("ern,ekn->erk", dz3, p["W3"]) * (h2 > 0)
    g["W2"], g["b2"] = np.einsum("erk,ern->ekn", h1, dz2), dz2.sum(1)
    dz1 = np.einsum("ern,ekn->erk", dz2, p["W2"]) * (h1 > 0)
    g["W1"], g["b1"] = np.einsum("erk,ern->ekn", x, dz1), dz1.sum(1)
    g["dx"] = np.einsum("ern,ekn->erk", dz1, p["W1"])
    return g


def adam(p, g, m, v, t, lr):
    """torch.optim.Adam's defaults, one step in fp64 on flat arrays; returns (p, m, v)."""
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - 0.999 ** t) + 1e-8
    return p - (lr / (1.0 - 0.9 ** t)) * m / denom, m, v
