"""NumPy twin of the "bf16x3" product (csrc/tile_bf.h) and the input cases of tests/test_hip_bf16x3.py.

"bf16x3" carries an fp32 operand as three bf16 terms x = t0 + t1 + t2, each the round-to-nearest-even bf16 of the fp32
remainder (split_terms<3> for activations and gradients, bf_split<3> for the weight planes: the same arithmetic), and a
product keeps the six term pairs (i, j) with i + j < 3.  The twin models that operand error only: the kept pairs are
summed in fp64, the fp32 add order of the MFMA accumulators is not modelled (tests/f64_bounds.py carries it in c).
`pairs=` selects other pair sets: the mutants tests/test_bf16x3_ref.py shows the bound to reject."""
import numpy as np

KEPT = tuple((i, j) for i in range(3) for j in range(3) if i + j < 3)
DROPPED = tuple((i, j) for i in range(3) for j in range(3) if i + j >= 3)
MUTANTS = {"pair_11_dropped": tuple(p for p in KEPT if p != (1, 1)),
           "pairs_02_20_dropped": tuple(p for p in KEPT if p not in ((0, 2), (2, 0))),
           "two_planes": ((0, 0), (0, 1), (1, 0))}
S, A, HID = 17, 6, 256
# rows of the weight-gradient geometry test: a partial 8-row half block and a partial 16-row block in front of the masked tail,
# one block more or less per wave, several waves, several workgroups
WGRAD_ROWS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65, 257, 513, 769, 1025)


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32.  Inf stays Inf, NaN stays NaN."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r)


def split3(x):
    """The three bf16 terms of fp32 `x` ([3, ...] fp32); the remainders are formed in fp32, as the kernels form them."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = bf16_rne(x)
        r1 = (x - t0).astype(np.float32)
        t1 = bf16_rne(r1)
        t2 = bf16_rne((r1 - t1).astype(np.float32))
    return np.stack([t0, t1, t2])


def gemm(a, b, pairs=KEPT):
    """a [.., rows, K] @ b [.., K, N] as the split core forms it: the term pairs `pairs`, summed exactly (fp64)."""
    ta, tb = split3(a).astype(np.float64), split3(b).astype(np.float64)
    return sum(ta[i] @ tb[j] for i, j in pairs)


def exact_case(a, b):
    """Precondition of a bit-exact bf16x3 GEMM a @ b: (lossless split and every dropped pair exactly zero, every kept product
    a multiple of one power of two with the sum of their magnitudes below 2^24 of it: every partial sum in every order is
    then exact in fp32).  Returns (dropped_is_zero, partial_sums_exact)."""
    ta, tb = split3(a).astype(np.float64), split3(b).astype(np.float64)
    lossless = np.array_equal(ta.sum(0), np.asarray(a, np.float64)) and np.array_equal(tb.sum(0), np.asarray(b, np.float64))
    dropped = sum(np.abs(ta[i]) @ np.abs(tb[j]) for i, j in DROPPED)

    def quantum(t):                               # the largest power of two dividing every non-zero term
        t = np.abs(t[t != 0])
        if t.size == 0:
            return 1.0
        m, e = np.frexp(t)
        mi = (m * 2.0 ** 53).astype(np.int64)
        return float(np.min(np.ldexp(1.0, e - 53) * (mi & -mi)))
    q = quantum(ta) * quantum(tb)
    total = sum(np.abs(ta[i]) @ np.abs(tb[j]) for i, j in KEPT)
    return bool(lossless and not dropped.any()), bool(np.max(total, initial=0.0) < 2.0 ** 24 * q)


# ---- the input cases of the forward tests -----------------------------------------------------------------------------------
def worst_terms(rng, shape):
    """Positive fp32 values whose second and third bf16 terms both sit near their maximum with the first term's sign:
    (1 + 2^-8 (1 - d1) + 2^-17 (1 - d2)) 2^e with small d1, d2 and e in {-1, 0, 1}.  t1 / t0 ~ 2^-8 and t2 / t0 ~ 2^-17, so in
    a product of two such values the pair (1, 1) is ~2^-16 and the pairs (0, 2) + (2, 0) are ~2^-16 of it, all positive."""
    d1 = rng.integers(1, 3, shape) * 2.0 ** -6                    # t1 = 2^-9 (2 - d1 2^1 ...) keeps 8 significand bits
    d2 = rng.integers(1, 5, shape) * 2.0 ** -5
    v = (1.0 + 2.0 ** -8 * (1.0 - d1) + 2.0 ** -17 * (1.0 - d2)) * 2.0 ** rng.integers(-1, 2, shape)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v.astype(np.float32)


def coherent_nets(pa, pq, rng):
    """Layer 1 becomes a selection (one input per hidden unit, weight 2^e, no bias): h1 is the input itself, exactly, in every
    mode.  W2 is all positive worst_terms() values (b2 = 0): with inputs >= 0 every dropped term of a layer-2 sum has one sign
    and they add up linearly, not like sqrt(K)."""
    pa, pq = ({k: v.copy() for k, v in p.items()} for p in (pa, pq))
    for p, pre, n_in in ((pq, "network1.", S + A), (pq, "network2.", S + A), (pa, "network.", S)):
        W1 = np.zeros((HID, n_in), np.float32)
        W1[np.arange(HID), np.arange(HID) % n_in] = 2.0 ** (np.arange(HID) % 3 - 1)
        p[pre + "network.0.weight"], p[pre + "network.0.bias"] = W1, np.zeros(HID, np.float32)
        p[pre + "network.2.weight"], p[pre + "network.2.bias"] = worst_terms(rng, (HID, HID)), np.zeros(HID, np.float32)
        W3 = p[pre + "network.4.weight"]
        p[pre + "network.4.weight"] = (W3 * 2.0 ** -8).astype(np.float32)          # keeps the actor's pre-tanh at unit scale
    return pa, pq


def forward_case(pattern):
    """(pa, pq, s, a) of one forward pattern: FWD_PATTERNS of tests/test_hip_f16_scaling.py, drawn as that file draws them,
    and "coherent" (96 rows, the last tile is whole; see coherent_nets)."""
    from test_hip_f16_scaling import q_params, rows_pattern
    rng = np.random.default_rng(len(pattern))
    if pattern == "coherent":
        pa, pq = coherent_nets(*q_params(301, "zero"), rng)
        return pa, pq, worst_terms(rng, (96, S)), worst_terms(rng, (96, A))
    rows, f, b1m = rows_pattern(pattern, rng)
    pa, pq = q_params(301, b1m)
    s = (rng.standard_normal((rows, S)) * f[:, None]).astype(np.float32)
    a = (rng.uniform(-1, 1, (rows, A)) * f[:, None]).astype(np.float32)
    return pa, pq, s, a


PLANTED = ((3, 255.875), (40, 256.0), (100, 300.0), (200, 4096.0), (17, -65536.0))      # (output unit n, value)
PLANTED_IN = (5, 77, 9, 130, 200)                                                       # their input units, unless given


def wide_w2(rng, ks=PLANTED_IN, shape=(HID, HID)):
    """W2 [out][in] with magnitudes 2^uniform(-12, 12), random signs and the exact elements PLANTED at the input units `ks`: at
    and past what an f16x2 plane can hold (255.875 is the first weight whose plane entry is Inf)."""
    W = (2.0 ** rng.uniform(-12, 12, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    for (n, v), k in zip(PLANTED, ks):
        W[n, k] = v
    return W


def planted_inputs(p, pre):
    """The five layer-1 units of largest bias (live on most rows): where the planted weights of a member read."""
    return np.argsort(p[pre + "network.0.bias"])[-len(PLANTED):]


def wide_q_params(seed=321):
    from test_hip_f16_scaling import q_params
    rng = np.random.default_rng(5)
    pa, pq = q_params(seed, "keep")
    for pre in ("network1.", "network2."):
        pq[pre + "network.2.weight"] = wide_w2(rng, planted_inputs(pq, pre))
    return pa, pq


def critic_gemms(c):
    """(name, a, b) of every bf16x3 GEMM of the critic step on an int_critic_case (tests/test_hip_twinq_rank1.py): layer 2 of
    Q(s, a), of the target Q(s2, pi = 0) and of the actor at s2, the backward dz2 W2^T and the weight gradient h1^T dz2."""
    s, a, s2 = c["batch"][:3]
    x2 = np.concatenate([s2, np.zeros_like(a)], 1)
    out = [("actor fwd", h1_fp32(c["pa"], "network.", s2), c["pa"]["network.network.2.weight"].T)]
    for m, pre in enumerate(("network1.", "network2.")):
        o, W2 = c["out"][m], c["pq"][pre + "network.2.weight"].T
        out += [(f"q{m} fwd", o["h1"], W2), (f"q{m} target fwd", h1_fp32(c["pq"], pre, x2), W2), (f"q{m} dx", o["dz2"], W2.T),
                (f"q{m} wgrad", o["h1"].T, o["dz2"])]
    return out


def assert_critic_case_exact(c, tag=""):
    """The precondition of comparing a bf16x3 critic step with the integer closed form bit for bit (exact_case, per GEMM)."""
    for what, x, y in critic_gemms(c):
        assert np.array_equal(np.asarray(x, np.float32), x) and np.array_equal(np.asarray(y, np.float32), y), f"{tag} {what}: not fp32"
        zero, exact = exact_case(x, y)
        assert zero, f"{tag} {what}: a dropped term pair is not zero"
        assert exact, f"{tag} {what}: a partial sum needs more than 24 bits"
        assert np.array_equal(gemm(x, y), np.asarray(x, np.float64) @ np.asarray(y, np.float64)), f"{tag} {what}"


def h1_fp32(p, pre, x):
    """Layer 1 on the host in fp32 (the kernels' layer 1 is exact fp32 in every mode; the CPU tests need an h1 of that kind,
    not the kernel's own bits)."""
    W1, b1 = p[pre + "network.0.weight"], p[pre + "network.0.bias"]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum((x.astype(np.float64) @ W1.T.astype(np.float64) + b1).astype(np.float32), 0)
