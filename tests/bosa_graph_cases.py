"""Inputs and the NumPy restatement shared by tests/test_bosa_graph_ref.py (CPU) and tests/test_hip_bosa_graph.py (GPU): BOSA's
bootstrap value (bosa.py:570-577) and the eight logged words of its second stage (bosa.py:591-627), written from the algorithm.  Every
function takes the dtype it computes in: float64 is the reference, float32 shows what a correct fp32 implementation reaches."""
import numpy as np

TARGET_SHAPES = ((17, 6), (11, 3), (3, 1), (111, 8))        # (S, A)
TARGET_ROWS = (2, 33, 256, 257, 1025)                        # 256 | 257: a workgroup's last thread and the next one's first; 1025: the
#                                                              grid-stride loop of 4 x 256 threads takes its second trip
SPLIT_ROWS = (33, 257)
WORDS_ROWS = (2, 33, 257, 1025)
WS_SHAPES = ((17, 6), (3, 1), (111, 8))
EXPL, CLIP = 0.1, 0.5                                        # config/mujoco/bosa/*.yaml's expl_noise and noise_clip
CONS, LAMDA = 0.1, 0.25
RTOL = ATOL = 1e-5                                           # the scalars' bounds of tests/test_hip_bosa_actor.py


def round4(n):
    return (n + 3) // 4 * 4


def target_workspace_floats(S, A, N):
    """mobody_bosa_target_workspace's closed form: a' [N][A] and the twin Q [2][N], each piece rounded up to 4 floats."""
    return round4(N * A) + round4(2 * N)


def mlp_params(seed, in_dim, out_dim, members):
    """nn.Linear-like nets in fp32: per member (W1 [256, in], b1, W2 [256, 256], b2, W3 [out, 256], b3)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(members):
        p = []
        for i, o in ((in_dim, 256), (256, 256), (256, out_dim)):
            b = 1.0 / np.sqrt(i)
            p += [rng.uniform(-b, b, (o, i)).astype(np.float32), rng.uniform(-b, b, o).astype(np.float32)]
        out.append(p)
    return out


def state_dict(params, prefixes):
    return {pre + "network.%d.%s" % (li, wb): p[2 * j + k] for pre, p in zip(prefixes, params) for j, li in enumerate((0, 2, 4))
            for k, wb in enumerate(("weight", "bias"))}


def mlp(p, x, dtype):
    W1, b1, W2, b2, W3, b3 = (t.astype(dtype) for t in p)
    h = np.maximum(x.astype(dtype) @ W1.T + b1, 0)
    h = np.maximum(h @ W2.T + b2, 0)
    return h @ W3.T + b3


def clamp(x, lo, hi):
    """torch.clamp: a NaN stays a NaN."""
    return np.where(np.isnan(x), x, np.minimum(np.maximum(x, lo), hi))


def target_action(pi, noise, expl, clip, ma, dtype=np.float64):
    """a' = clamp(pi + clamp(noise * expl, -clip, clip), -ma, ma); expl, clip, ma enter as the float32 the kernels get."""
    f = lambda v: dtype(np.float32(v))
    pi, noise = pi.astype(dtype), noise.astype(dtype)
    return clamp(pi + clamp(noise * f(expl), -f(clip), f(clip)), -f(ma), f(ma))


def target_value(actor, critic, s2, noise, expl, clip, ma, dtype=np.float64):
    """q_next [N] = min_m Q_m(s', a'), NaN where a member is NaN."""
    pi = dtype(np.float32(ma)) * np.tanh(mlp(actor[0], s2, dtype))
    a2 = target_action(pi, noise, expl, clip, ma, dtype)
    x = np.concatenate([s2.astype(dtype), a2], 1)
    q = np.stack([mlp(p, x, dtype)[:, 0] for p in critic])
    return np.where(np.isnan(q).any(0), np.nan, q.min(0)), a2


def target_inputs(S, A, N, seed=0):
    rng = np.random.default_rng(1000 * S + 10 * A + N + seed)
    return rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal((N, A)).astype(np.float32)


EDGE_EXPL = 1.0          # the clamp-edge runs scale the noise by one, so that the planted values ARE the clamp's inputs


def clamp_edge_inputs(A, clip=CLIP):
    """(noise [18, A], sign [18]): planted noise 0, +-clip, +-clip (1 + 2^-20), +-10 and +-clip / 4, each against a target actor whose
    output sits at +max_action (sign +1, even rows) and at -max_action (odd rows).  With expl_noise = 1, clip = 0.5 and max_action 1 or
    2 every intermediate is a float32, so the fp64 restatement's values are the exact expectation."""
    f32 = np.float32
    c = f32(clip)
    vals = np.array([0, c, -c, c * (1 + 2.0 ** -20), -c * (1 + 2.0 ** -20), 10, -10, 0.25 * c, -0.25 * c], np.float64)
    assert (vals.astype(f32).astype(np.float64) == vals).all()
    noise = np.repeat(vals.astype(f32), 2)[:, None].repeat(A, 1)
    sign = np.tile(np.array([1, -1], f32), len(vals))
    return np.ascontiguousarray(noise), sign


def words_inputs(N, seed=0):
    """mask, closs (loss, conservative term), ll with max(-ll) in the LAST row, aloss, dll [N, 6]."""
    rng = np.random.default_rng(77 + N + seed)
    mask = (rng.random(N) > 0.3).astype(np.float32)
    ll = (-3.0 + rng.standard_normal(N)).astype(np.float32)
    ll[-1] = ll.min() - np.float32(1.5)
    closs = np.array([1.7 + rng.random(), -0.4 + rng.random()], np.float32)
    aloss = np.array([-1.0 + 0.1 * rng.random(), 0.0], np.float32)
    dll = rng.standard_normal((N, 6)).astype(np.float32)
    return mask, closs, ll, aloss, dll


def words(mask, closs, ll, aloss, cons, lamda, dtype=np.float64):
    """(the eight words, the largest term of each) in STAGE2_LOG order; words[7] = lamda."""
    f = lambda v: dtype(np.float32(v))
    c0, c1 = dtype(closs[0]), dtype(closs[1])
    nl = -ll.astype(dtype)
    if dtype is np.float32:                                  # sequential fp32 sum: the plainest correct implementation
        acc = np.float32(0)
        for v in nl:
            acc = np.float32(acc + v)
        mean = np.float32(acc / np.float32(len(nl)))
    else:
        mean = nl.mean()
    mx = np.nan if np.isnan(nl).any() else nl.max()
    w = np.array([mask.astype(dtype).mean(), c0, c0 - f(cons) * c1, c1, dtype(aloss[0]) + f(lamda) * mean, mean, mx, f(lamda)], dtype)
    terms = np.array([1.0, abs(c0), max(abs(c0), abs(f(cons) * c1)), abs(c1), max(abs(dtype(aloss[0])), abs(f(lamda) * mean)), np.abs(nl).max(),
                      np.abs(nl).max(), abs(f(lamda))], np.float64)
    return w, terms


def words_tolerance(w64, terms):
    return RTOL * np.abs(w64) + ATOL * terms
