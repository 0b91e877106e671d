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

# The corners of mobody_wide_layout's domain (in 1..256, hidden 8..1024, out 1..256, members 1..8) and the shapes without padding:
# (hidden, rows, members, (in, out), output mode, source widths, index of the per-member source or None).  The minimum and the
# maximum of every dimension, an in_dim that is a multiple of 16 with out_dim a multiple of 64 (no padding anywhere), row counts of
# exactly one 16-row chunk, one and two 64-row tiles, and out_dim = 65: one column into a second 64-wide tile.
CORNER_CASES = [
    (32, 64, 8, (1, 1), "raw", (1,), None),
    (64, 128, 1, (16, 64), "tanh", (16,), None),
    (1024, 17, 2, (256, 256), "raw", (100, 100, 56), 1),
    (8, 16, 8, (256, 1), "raw", (256,), 0),
    (1024, 1, 1, (1, 256), "tanh", (1,), None),
    (96, 65, 3, (17, 65), "raw", (17,), None),
]


def case_inputs(case, seed=11):
    """Seeded parameters and sources of a case: (p, sources, x [E, rows, in] in fp64)."""
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    assert sum(widths) == in_dim
    p = params(seed, in_dim, hidden, out_dim, E)
    rng = np.random.default_rng(seed + 1)
    srcs = [rng.standard_normal(((E, rows, w) if i == per_member else (rows, w))).astype(np.float32) for i, w in enumerate(widths)]
    return p, srcs, np.concatenate([bcast(s, E) for s in srcs], axis=2)


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


def backward(p, x, h1, h2, dz3, dtype=np.float64):
    """Gradients (dict as the parameters, plus "dx" [E, rows, in]) from the gradient dz3 of the last layer's pre-activation
    and the forward's activations; the ReLU masks are h > 0 of the activations GIVEN (the kernel's own saves in the tests, so
    that a pre-activation within rounding of 0 cannot flip a unit between the two computations).  dtype = np.float32 evaluates
    the same expressions in single precision (tests/test_wide_ref.py: what a correct fp32 kernel may differ by)."""
    p = {k: np.asarray(v, dtype) for k, v in p.items()}
    E = p["W1"].shape[0]
    x, h1, h2, dz3 = (np.asarray(t, dtype) for t in (bcast(x, E), h1, h2, dz3))
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
