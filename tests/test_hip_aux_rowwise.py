"""The row-wise kernels around the generic MLP gradient, each against its fp64 reference (tests/aux_ref.py) at the sizes
where a 256-thread block boundary or a partial-sum count changes.

Bounds (u = 2^-24; expf / logf of the device library within 2 ulp; every step below is one fp32 rounding unless noted).

ce_on_probs (csrc/dara.hip), head logits z -> p = softmax(z) -> q = softmax(p), g = q - onehot, t_i = g_i - sum_j g_j p_j,
dz_i = p_i t_i / N:
  p:  z - max (exact for the larger logit, whose e = 1), expf, e0 + e1, 1 / sum, e * inv.  With d = |z0 - z1| the small
      e carries (d + 2) u relative error and d e^-d <= 0.37, so both |dp_i| <= 6 u absolutely, for every d (for d > 87 the
      small e underflows to 0: an absolute error below 2^-126, the `TINY` term).
  q:  the same five steps on p, |p0 - p1| <= 1: 6 u q from its own steps + q0 q1 |d(p0 - p1)| <= 0.25 * 12 u:  |dq| <= 9 u
  g:  one subtraction, |g| < 0.74:  |dg| <= 10 u
  dot = g0 p0 + g1 p1:  dg (p0 + p1) + sum |g_j| dp_j + 2 u sum |g_j| p_j <= (10 + 8.8 + 2) u <= 21 u
  t_i = g_i - dot:  <= (10 + 21 + 1) u = 32 u
  dz_i = (1/N) p_i t_i (1/N rounded, two products):  |err| <= (32 u p_i + 6 u |t_i|) / N + 3 u |dz_i| + TINY
  row loss -logf(q_label), q in [0.2689, 0.7311]:  |dq| / q + 2 u |log q| + ... <= 37 u
  loss = sum / N:  the sequential-sum bound N u mean|l| (the kernels' tree is far shorter) + the rows' 37 u + 2 u.
dara_penalty: four logf(q + 1e-10f) of such q: per log (6 u q + 3 u) / q + 2 u * 1.32 + 1 u <= 21 u, three adds of values
  below 2.7: |d delta| <= 4 * 21 u + 6 u = 90 u;  reward += coef * delta adds u |coef delta| + u |reward|.
k_v_loss: adv = min(qt) - v (one rounding, sign exact), w = |0.7f - 1[adv < 0]| (<= 2.2 u relative at 0.3), l = w adv adv,
  dz = -2 w adv / Ng: both within 7 u relative; loss = sum l / Ng within (N + 9) u sum |l| / Ng.
k_par_penalty: (S + 2) u coef mean(e^2) (S - 1 adds, the product, the division, the scaling) plus one rounding of the new reward.
  That leaves no room for the rounding of the differences e = s'_true - s'_model themselves (2 u of e^2): an all-fp32 row
  loop is only good for (S + 4) u and missed this bound at S = 1, so the kernel forms the mean in double and rounds once.
"""
import numpy as np
import pytest
import torch

import aux_ref as R
import f64_bounds as FB
from oracle import mobody_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -120
NS = [1, 63, 64, 65, 255, 256, 257, 1000, 65537]
SA = [(3, 1), (17, 6), (45, 24), (111, 8)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def T(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=dev, dtype=dtype).contiguous()


def logits(kind, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return (3.0 * rng.standard_normal((N, 2))).astype(np.float32)
    if kind == "saturated":                              # the head at +-80, either class
        z = np.where(rng.random((N, 1)) < 0.5, [[80.0, -80.0]], [[-80.0, 80.0]])
        return z.astype(np.float32)
    if kind == "equal":
        return np.repeat(rng.standard_normal((N, 1)), 2, 1).astype(np.float32)
    if kind == "huge":                                   # both at 1e4: needs the max-subtraction
        return np.full((N, 2), 1e4, np.float32)
    if kind == "huge_apart":                             # 1e4 and 1e4 - 3
        return np.tile(np.float32([1e4, 1e4 - 3.0]), (N, 1))
    raise KeyError(kind)


def ce_bounds(z, labels):
    """fp64 loss / dz of one head and their bounds (module docstring)."""
    N = z.shape[0]
    loss, dz, rows = R.double_softmax_ce_ref(z, labels)
    p = R.softmax2_ref(z)
    q = R.softmax2_ref(p)
    g = q.copy(); g[np.arange(N), labels] -= 1.0
    t = g - (g * p).sum(-1, keepdims=True)
    b_dz = (32 * U * p + 6 * U * np.abs(t)) / N + 3 * U * np.abs(dz) + TINY
    b_loss = N * U * np.abs(rows).mean() + 39 * U
    return loss, dz, b_loss, b_dz


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ["random", "saturated", "equal", "huge", "huge_apart"])
def test_dara_loss_grad_vs_fp64(kind, N, dev):
    from mobody_amd import ops
    z_sas, z_sa = logits(kind, N, 5 + N), logits("random" if kind == "huge" else kind, N, 6 + N)
    rng = np.random.default_rng(N)
    modes = [("labels", rng.integers(0, 2, N), 0)] + [("n_src", None, n) for n in sorted({0, N // 3, N})]
    for mode, lab, n_src in modes:
        labels = lab if lab is not None else (np.arange(N) >= n_src).astype(np.int64)
        dz_sas, dz_sa, loss = ops.dara_loss_grad(T(z_sas, dev), T(z_sa, dev), n_src, lab)
        loss = loss.cpu().numpy()
        for name, z, got_dz, got_l in (("sas", z_sas, dz_sas, loss[1]), ("sa", z_sa, dz_sa, loss[0])):
            want_l, want_dz, b_l, b_dz = ce_bounds(z, labels)
            got_dz = got_dz.cpu().numpy()
            what = f"{kind} N={N} {mode}={n_src} {name}"
            assert got_dz.shape == (N, 16) and (got_dz[:, 2:] == 0).all(), what + ": dz columns 2..15 not exactly 0"
            FB.check(got_dz[:, :2], want_dz, b_dz, what + " dz")
            FB.check(got_l, want_l, b_l, what + " loss")


@pytest.mark.parametrize("N", NS)
def test_dara_penalty_vs_fp64(N, dev):
    from mobody_amd import ops
    kinds = ["random", "saturated", "equal", "huge", "huge_apart"]
    z_sas = np.concatenate([logits(k, N, 11 + i) for i, k in enumerate(kinds)])[np.random.default_rng(N).permutation(5 * N)][:N]
    z_sa = logits("random", N, 12)
    want, raw = R.dara_penalty_ref(z_sas, z_sa)
    # From the reference alone: softmax of probabilities lies in [1/(1+e), e/(1+e)], each log-ratio in [-1, 1], so
    # |delta| <= 2 and the clamp at +-10 (mobody.py:378) can never bind on softmax-of-softmax inputs -- also not at +-80 / 1e4.
    for z in [logits(k, 64, 3) for k in kinds]:
        assert np.abs(R.dara_penalty_ref(z, z[::-1].copy())[1]).max() <= 2.0
    assert np.abs(raw).max() <= 2.0 and np.array_equal(want, raw)
    zs, za = T(z_sas, dev), T(z_sa, dev)
    b_d = 90 * U
    delta = ops.dara_penalty(zs, za, 0.0)                                  # delta_out only
    assert delta.shape == (N, 1)
    FB.check(delta.cpu().numpy()[:, 0], want, b_d, f"delta N={N}")
    r0 = np.random.default_rng(N + 1).standard_normal(N).astype(np.float32)
    for coef in (0.0, 0.1, -2.5):
        cf = float(np.float32(coef))
        for want_delta in (False, True):                                   # reward only; both
            reward = T(r0.copy().reshape(N, 1), dev)
            keep = reward
            d2 = ops.dara_penalty(zs, za, cf, reward, want_delta=want_delta)
            assert reward.data_ptr() == keep.data_ptr()                     # in place
            new = r0.astype(np.float64) + cf * want
            FB.check(reward.cpu().numpy()[:, 0], new, abs(cf) * b_d + U * np.abs(cf * want) + U * np.abs(new), f"reward coef={coef} N={N}")
            if coef == 0.0:
                assert np.array_equal(reward.cpu().numpy()[:, 0], r0)
            if want_delta:
                assert torch.equal(d2, delta)
            else:
                assert d2 is None


@pytest.mark.parametrize("S,A", SA)
@pytest.mark.parametrize("N", [1, 257, 1000])
def test_dara_inputs(S, A, N, dev):
    from mobody_amd import ops
    rng = np.random.default_rng(S + N)
    s, a, s2 = (rng.standard_normal(sh).astype(np.float32) for sh in ((N, S), (N, A), (N, S)))
    sd, ad, s2d = T(s, dev), T(a, dev), T(s2, dev)
    cat_sas, cat_sa = np.concatenate([s, a, s2], 1), np.concatenate([s, a], 1)
    x_sas, x_sa = ops.dara_inputs(sd, ad, s2d, 0.0)                         # std = 0: the exact concatenation
    assert np.array_equal(x_sas.cpu().numpy(), cat_sas) and np.array_equal(x_sa.cpu().numpy(), cat_sa)
    std = float(np.float32(0.3))
    e_sas, e_sa = rng.standard_normal(cat_sas.shape).astype(np.float32), rng.standard_normal(cat_sa.shape).astype(np.float32)
    x_sas, x_sa = ops.dara_inputs(sd, ad, s2d, std, T(e_sas, dev), T(e_sa, dev))
    for got, v, e in ((x_sas, cat_sas, e_sas), (x_sa, cat_sa, e_sa)):
        # v + std e with or without FMA contraction: within one ulp (at the larger of |result| and |std e|, the product's rounding)
        prod = std * e.astype(np.float64)
        want = v.astype(np.float64) + prod
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(prod)).astype(np.float32)).astype(np.float64)
        FB.check(got.cpu().numpy(), want, ulp, f"explicit noise S={S} A={A} N={N}")
    seed, call = 1234 + S, 7
    n_sas = ops.rng_normal(seed, 4, call, N * (2 * S + A), dev).view(N, 2 * S + A)       # STREAM_CLS_SAS / STREAM_CLS_SA
    n_sa = ops.rng_normal(seed, 5, call, N * (S + A), dev).view(N, S + A)
    dev_sas, dev_sa = ops.dara_inputs(sd, ad, s2d, std, seed=seed, call=call)
    exp_sas, exp_sa = ops.dara_inputs(sd, ad, s2d, std, n_sas.contiguous(), n_sa.contiguous())
    assert torch.equal(dev_sas, exp_sas) and torch.equal(dev_sa, exp_sa)
    assert not torch.equal(dev_sas, T(cat_sas, dev))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("mult", [1, 3])
def test_value_loss_grad_vs_fp64(N, mult, dev):
    from mobody_amd import ops
    rng = np.random.default_rng(N)
    qt = (5.0 * rng.standard_normal((2, N))).astype(np.float32)
    v = (qt.min(0) + rng.standard_normal(N)).astype(np.float32)
    v[::7] = qt.min(0)[::7]                                # the expectile's kink: adv == 0 exactly
    Ng = mult * N
    want_l, want_dv = R.value_loss_ref(qt, v, Ng)
    adv = np.minimum(qt[0], qt[1]).astype(np.float64) - v
    assert (adv == 0).sum() >= 1 and (want_dv[adv == 0] == 0).all() and (N < 63 or ((adv < 0).any() and (adv > 0).any()))
    dz3, loss = ops.value_loss_grad(T(qt, dev), T(v, dev), Ng)
    dz3 = dz3.cpu().numpy()
    assert dz3.shape == (N, 16) and (dz3[:, 1:] == 0).all(), "dz3 columns 1..15 not exactly 0"
    FB.check(dz3[:, 0], want_dv, 7 * U * np.abs(want_dv), f"dV N={N} Ng={Ng}")
    FB.check(loss.cpu().numpy()[0], want_l, (N + 9) * U * abs(want_l), f"V loss N={N} Ng={Ng}")


@pytest.mark.parametrize("S", [1, 3, 17, 45, 111])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 65537])
def test_par_penalty_vs_fp64(S, N, dev):
    from mobody_amd import ops
    rng = np.random.default_rng(S * N)
    t, m = rng.standard_normal((N, S)).astype(np.float32), rng.standard_normal((N, S)).astype(np.float32)
    r0 = rng.standard_normal((N, 1)).astype(np.float32)
    coef = float(np.float32(0.1))
    want, mse = R.par_penalty_ref(t, m, r0, coef)
    reward = T(r0, dev)
    p0 = reward.data_ptr()
    ops.par_penalty(T(t, dev), T(m, dev), reward, coef)
    assert reward.data_ptr() == p0 and reward.shape == (N, 1)
    FB.check(reward.cpu().numpy()[:, 0], want, (S + 2) * U * coef * mse + U * np.abs(want), f"par S={S} N={N}")


# keep / alive_out of one row, written out from mobody.py:635-653:  nonterm_mask = ~terminals; observations =
# next_observations[nonterm_mask] (a row stays alive iff it was alive and did not terminate), and with filter_bad_rollout
# idx = penalty <= env_filter  (NaN and +Inf compare False, -Inf and the equal value True).
ENV_FILTER = 0.75
PENALTIES = [("below", 0.5, 1), ("equal", ENV_FILTER, 1), ("above", 1.0, 0), ("nan", float("nan"), 0),
             ("+inf", float("inf"), 0), ("-inf", float("-inf"), 1)]
MASK_TABLE = [  # (alive_in or None, terminal, filter, penalty name) -> (keep, alive_out)
    ((al, te, fi, pn), (int((al is None or al == 1) and (not fi or pk == 1)), int((al is None or al == 1) and te == 0)))
    for al in (0, 1, None) for te in (0, 1) for fi in (False, True) for pn, _, pk in PENALTIES]


def test_rollout_mask_table_is_written_out():
    want = {(1, 0, True, "equal"): (1, 1), (1, 0, True, "above"): (0, 1), (1, 1, True, "below"): (1, 0), (0, 0, False, "below"): (0, 0),
            (None, 0, True, "nan"): (0, 1), (None, 1, True, "-inf"): (1, 0), (1, 0, True, "+inf"): (0, 1), (1, 0, False, "nan"): (1, 1),
            (0, 1, True, "-inf"): (0, 0), (None, 0, False, "+inf"): (1, 1)}
    tab = dict(MASK_TABLE)
    assert len(tab) == 72 and all(tab[k] == v for k, v in want.items())


@pytest.mark.parametrize("B_min", [1, 255, 256, 257, 65537])
@pytest.mark.parametrize("use_filter", [False, True])
@pytest.mark.parametrize("alive_mode", ["array", "null", "aliased"])
def test_rollout_mask_exhaustive(alive_mode, use_filter, B_min, dev):
    from mobody_amd import ops
    pv = dict((n, v) for n, v, _ in PENALTIES)
    full = [(k, w) for k, w in MASK_TABLE if k[2] == use_filter and ((k[0] is None) == (alive_mode == "null"))]
    assert len(full) == (12 if alive_mode == "null" else 24)
    # B = 1: every table row as a launch of its own; otherwise the table tiled to B rows
    batches = [[r] for r in full] if B_min == 1 else [(full * -(-B_min // len(full)))[:B_min]]
    for rows in batches:
        B = len(rows)
        terminal = T([k[1] for k, _ in rows], dev, torch.uint8)
        penalty = T(np.float32([pv[k[3]] for k, _ in rows]), dev)
        alive_in = None if alive_mode == "null" else T([k[0] for k, _ in rows], dev, torch.uint8)
        keep = torch.full((B,), 7, dtype=torch.uint8, device=dev)
        alive_out = alive_in if alive_mode == "aliased" else torch.full((B,), 7, dtype=torch.uint8, device=dev)
        ops.rollout_mask(alive_in, terminal, penalty, ENV_FILTER, use_filter, keep, alive_out)
        want_keep, want_alive = np.uint8([w[0] for _, w in rows]), np.uint8([w[1] for _, w in rows])
        assert np.array_equal(keep.cpu().numpy(), want_keep), (alive_mode, use_filter, B)
        assert np.array_equal(alive_out.cpu().numpy(), want_alive), (alive_mode, use_filter, B)


SIZES = [1, 2, 3, 1000, 10 ** 6, 2 ** 31 - 1]


@pytest.mark.parametrize("size", SIZES)
def test_rng_index_and_sample_indices(size, dev):
    from mobody_amd import ops
    seed, stream, n = 99, 3, 65537 if size == 1000 else 1000
    got = ops.rng_index(seed, stream, 11, n, size, dev).cpu().numpy()
    want = O.rng_index(seed, stream, 11, n, size)          # multiply-high of the CPU twin's Philox words
    assert got.min() >= 0 and got.max() < size and np.array_equal(got.astype(np.int64), want)
    if size > 3:
        assert got.max() > size // 2
    size_dev = torch.tensor([size], dtype=torch.int64, device=dev)
    for counter, off, call in ((None, 11, 11), (5, 6, 11), (2 ** 32 - 2, 5, 3), (2 ** 32 + 9, 2 ** 32 + 2, 11), (40, -29, 11)):
        cdev = None if counter is None else torch.tensor([counter], dtype=torch.int64, device=dev)
        out = ops.sample_indices(seed, stream, cdev, off, n, size_dev).cpu().numpy()
        w = O.rng_index(seed, stream, call, n, size)
        assert out.min() >= 0 and out.max() < size and np.array_equal(out.astype(np.int64), w), (size, counter, off)
    if size > 3:
        assert not np.array_equal(want, O.rng_index(seed, stream, 3, n, size))       # call 3 (past 2^32) differs from call 11


@pytest.mark.parametrize("n", [1, 2, 64])
def test_counter_add(n, dev):
    from mobody_amd import ops
    base = (2 ** 32 + 5) + (2 ** 33) * np.arange(70, dtype=np.int64)
    buf = torch.from_numpy(base.copy()).to(dev)
    for inc in (1, 2 ** 32 + 3, -7):
        before = buf.cpu().numpy().copy()
        ops.counter_add(buf[:n], inc)
        after = buf.cpu().numpy()
        assert np.array_equal(after[:n], before[:n] + inc) and np.array_equal(after[n:], before[n:]), (n, inc)
    assert (buf.cpu().numpy() > 2 ** 32).all()
