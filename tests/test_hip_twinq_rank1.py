"""The rank-1 output layer of the twin-Q backward launches (csrc/mlp_bwd.hip k_mlp3_bwd, BwdSeed modes 1 and 2): a seed that
fills column 0 of a one-output net makes dz3 W3^T the product seed[row] * W3^T[0][col], formed in registers instead of by a
K = Np3 GEMM; the frozen-Q pass of the actor update (mode 2) also stores no bias-gradient partials.  Every test fills the
whole workspace, and every output, with NaN sentinels before the call.

1. test_critic_rank1_*: mobody_critic_step (seed mode 1) on integer nets with power-of-two scalars equals the integer closed
   form bit for bit at 1, 31, 32, 33 and 65 rows, exact zeros in the padding; real-valued nets at 33 and 65 rows against fp64
   with f64_bounds.grad_bounds.  The GEMM form of the same tile is reachable through mobody_mlp3_backward (seed mode 0: dz3
   from memory, K = Np3 GEMM) only with activations the caller supplies -- the critic's saved activations live in its private
   workspace -- so the `==` comparison of the two forms is made where the activations are identical by construction: the
   integer nets, whose activations and dz3 are exact in every evaluation; exact fp32 mode.
2. test_backward_follows_handed_stats (seed mode 2 on the way): the data-parallel contract.  stats <- 1.7 x what the forward
   wrote, N_global = 2 N, Nt_global = 2 Nt, then the backward; gradients and both losses per element against the fp64 closed
   form evaluated with the substituted stats, bounds of actor_ref.actor_bounds (those of tests/test_hip_actor_fp64.py).
   Before the GPU is touched the same bounds are shown to REJECT a closed form that takes p_w, the BC weights, or both from
   the local sums (every shape with Nt > 0; the smallest violation factor is printed).
3. test_backward_repeatable: two backward calls on one forward give the same bits (nothing the forward left is consumed,
   and the bias partials the frozen-Q pass no longer writes are read by nobody); with bc_coef = 0, stats[0] x 4 gives exactly
   a quarter of the blob.
"""
import functools

import numpy as np
import pytest
import torch

import actor_ref as AR
import aux_ref as R
import f64_bounds as FB
import golden_util as gu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SA2 = [(17, 6), (11, 3)]
DP_CASES = [(sa, N, Nt) for sa in SA2 for N in (33, 257) for Nt in (0, 7, N)]
RANK1_ROWS = (1, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def same_bits(got, want, what):
    """Bit equality of fp32 `got` with the fp64 `want` rounded once (a zero's sign is not a bit of the sum)."""
    got = np.asarray(got, np.float32) + np.float32(0)
    want = np.asarray(want, np.float64).astype(np.float32) + np.float32(0)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first {i}: got {got[i]!r} want {want[i]!r}")


class ActorRun:
    """pack -> transposes -> NaN sentinels (stats, gradient, losses, the whole workspace) -> actor_forward; backward() may be
    called any number of times on that one forward."""

    def __init__(self, p, mode, dev, Ng=None, Ntg=None):
        from mobody_amd import _lib, ops, packing
        self.ops, self.packing, self.dev, self.mode, self.p = ops, packing, dev, mode, p
        S, A, N, Nt = p["s"].shape[1], p["act"].shape[1], p["N"], p["Nt"]
        self.S, self.A = S, A
        self.actor = packing.pack_mlp([{k[len("network."):]: v for k, v in p["pa"].items()}], S, A, dev)
        self.q = packing.pack_mlp(p["pq"], S + A, 1, dev, prefixes=["network1.", "network2."])
        self.actor_T = ops.mlp_transpose(self.actor, S, A, 1, precision=mode)
        self.q_T = ops.mlp_transpose(self.q, S + A, 1, 2, precision=mode)
        self.dims = ops.train_dims(S, A, N, Nt, p["Ng"] if Ng is None else Ng, p["Ntg"] if Ntg is None else Ntg)
        self.ws = ops.train_workspace(self.dims, dev)
        self.ws.fill_(float("nan"))
        self.s = torch.from_numpy(p["s"]).to(dev).contiguous()
        self.a = torch.from_numpy(p["act"]).to(dev).contiguous()
        self.L = _lib.mlp_layout(S, A, 1)
        self.stats = nan(2, dev)
        ops.actor_forward(self.dims, self.hyp(), self.actor, self.q, self.s, self.a, self.stats, self.ws, actor_blob_T=self.actor_T,
                          q_blob_T=self.q_T)
        torch.cuda.synchronize()

    def hyp(self, **over):
        h = dict(self.p["h"], **over)
        cfg = dict(gamma=0.99, tau=0.005, mfma=self.mode, **{k: h[k] for k in ("max_action", "weight", "bc_coef", "q_weighted", "scale_Q")})
        return self.ops.hyper(cfg)

    def backward(self, stats, **over):
        grad, loss = nan(self.L.total_floats, self.dev), nan(2, self.dev)
        v_true = torch.from_numpy(self.p["v_true"]).to(self.dev) if self.p.get("v_true") is not None else None
        self.ops.actor_backward(self.dims, self.hyp(**over), self.actor, self.actor_T, self.q, self.q_T, self.s, self.a, stats, grad, loss,
                                self.ws, v_true=v_true)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grad).all()), f"{int((~torch.isfinite(grad)).sum())} entries of the gradient blob unwritten / non-finite"
        return grad, loss

    def tensors(self, grad):
        L, S, A = self.L, self.S, self.A
        w1 = self.packing.wide_unpack(grad[L.w1:L.w1 + L.Kp1 * 256], L.Kp1)
        w3 = grad[L.w3:L.w3 + 256 * L.Np3].view(256, L.Np3)
        b3 = grad[L.b3:L.b3 + L.Np3]
        assert bool((w1[S:] == 0).all()), "dW1 padding rows k >= S are not exactly 0"
        assert bool((w3[:, A:] == 0).all()) and bool((b3[A:] == 0).all()), "dW3 / db3 padding columns are not exactly 0"
        return {"network." + k: v.cpu().numpy() for k, v in self.packing.unpack_mlp(grad, S, A, 1)[0].items()}


# ---- 2. the backward follows the stats it is handed (frozen-Q pass: seed mode 2) --------------------------------------------------------------------
STATS_MUL = 1.7


@functools.lru_cache(maxsize=None)
def dp_case(SA, N, Nt):
    """N robust rows (FB.robust_rows) out of a pool of 4 N, the fp64 reference with stats = 1.7 x local at N_global = 2 N,
    Nt_global = 2 Nt, and the references of the three wrong readings (local sums for p_w, for the BC weights, for both)."""
    S, A = SA
    seed = 1200 + 31 * DP_CASES.index((SA, N, Nt))
    pa, pq, _ = gu.policy_params(seed, S, A)
    h = dict(max_action=1.0, weight=2.5, bc_coef=1.0, q_weighted=1, scale_Q=1, advantage=0)
    s, a, _, _, _ = gu.gi.batch(seed + 5, 4 * N, S, A)
    keep = np.flatnonzero(FB.robust_rows(pa, pq, s, a))
    assert keep.size >= N, "too few robust rows in the pool"
    s, a = s[keep[:N]].copy(), a[keep[:N]].copy()
    Ng, Ntg = 2 * N, 2 * Nt
    fw = AR.forward_ref(pa, pq, s, a, Nt, 1.0)
    args = (fw["pi"], fw["qp"], fw["qb"], fw["dqda"], a, h, N, Nt, Ng, Ntg)
    local = AR.closed_forms(*args)["stats"]
    sub = STATS_MUL * local
    cf = AR.closed_forms(*args, stats=sub)
    grads, tape = AR.actor_grads_ref(pa, s, fw, cf["dz3"])
    wrong = {}
    for name, st in (("p_w from the local sum", [local[0], sub[1]]), ("BC weights from the local sum", [sub[0], local[1]]),
                     ("both from the local sums", local)):
        cw = AR.closed_forms(*args, stats=np.asarray(st))
        wrong[name] = dict(AR.actor_grads_ref(pa, s, fw, cw["dz3"])[0], L_pi=cw["L_pi"], L_BC=cw["L_BC"])
    return dict(pa=pa, pq=pq, s=s, act=a, h=h, N=N, Nt=Nt, Ng=Ng, Ntg=Ntg, fw=fw, cf=cf, grads=grads, tape=tape, v_true=None,
                wrong=wrong)


@functools.lru_cache(maxsize=None)
def dp_bounds(SA, N, Nt, split):
    c = dp_case(SA, N, Nt)
    return AR.actor_bounds(c["pa"], c["pq"], c["s"], c["act"], c["h"], N, Nt, c["Ng"], c["Ntg"], c["fw"], c["cf"], c["tape"], split)


def wrong_readings_violate(SA, N, Nt, split):
    """Smallest, over the three wrong readings, of the worst |wrong - right| / bound over every checked output."""
    c, bd = dp_case(SA, N, Nt), dp_bounds(SA, N, Nt, split)
    ref = dict(c["grads"], L_pi=c["cf"]["L_pi"], L_BC=c["cf"]["L_BC"])
    bound = dict(bd["grads"], L_pi=bd["L_pi"], L_BC=bd["L_BC"])
    return min(max(AR.ratios(w[k], ref[k], bound[k]) for k in ref) for w in c["wrong"].values())


@pytest.mark.parametrize("case", DP_CASES, ids=lambda c: f"S{c[0][0]}A{c[0][1]}-N{c[1]}-Nt{c[2]}")
def test_backward_follows_handed_stats(case, mfma, dev):
    SA, N, Nt = case
    split = mfma == "f16x2"
    c, bd = dp_case(*case), dp_bounds(SA, N, Nt, split)
    if Nt > 0:
        worst = wrong_readings_violate(SA, N, Nt, split)
        print(f"{case} {mfma}: a closed form on the local sums misses the bound by at least x{worst:.3g}")
        assert worst > 1.0, "the bound would accept a backward that used the local sums"
    run = ActorRun(c, mfma, dev)                       # dims carry N_global = 2 N, Nt_global = 2 Nt
    grad, loss = run.backward(run.stats * STATS_MUL)
    g, loss = run.tensors(grad), loss.cpu().numpy()
    got = dict(g, L_pi=loss[0], L_BC=loss[1])
    ref = dict(c["grads"], L_pi=c["cf"]["L_pi"], L_BC=c["cf"]["L_BC"])
    bound = dict(bd["grads"], L_pi=bd["L_pi"], L_BC=bd["L_BC"])
    print(case, mfma, {k: f"{AR.ratios(got[k], ref[k], bound[k]):.3g}" for k in ref})
    for k in ref:
        FB.check(got[k], ref[k], bound[k], f"{case} {mfma} {k}")


# ---- 3. the backward is repeatable on one forward ----------------------------------------------------------------------
@pytest.mark.parametrize("case", [((17, 6), 257, 7), ((11, 3), 33, 33)], ids=lambda c: f"S{c[0][0]}A{c[0][1]}-N{c[1]}-Nt{c[2]}")
def test_backward_repeatable(case, mfma, dev):
    run = ActorRun(dp_case(*case), mfma, dev)
    bits = lambda t: t.view(torch.int32)
    stats = run.stats.clone()
    g1, l1 = run.backward(stats)
    g2, l2 = run.backward(stats)
    assert torch.equal(bits(g1), bits(g2)) and torch.equal(bits(l1), bits(l2)), "a second backward on the same forward differs"
    # bc_coef = 0: the gradient is linear in p_w = weight / (stats[0] / N_global), and a factor 4 is exact in every rounding
    f1, _ = run.backward(stats, bc_coef=0.0)
    f2, _ = run.backward(stats, bc_coef=0.0)
    assert torch.equal(bits(f1), bits(f2)), "a second backward (bc_coef = 0) on the same forward differs"
    s4 = stats.clone()
    s4[0] *= 4.0
    f4, _ = run.backward(s4, bc_coef=0.0)
    assert float(f1[f1 != 0].abs().min()) > 2.0 ** -120, "a quarter would leave the normal range"
    assert bool((f4 == f1 * 0.25).all()), f"{int((f4 != f1 * 0.25).sum())} elements are not exactly a quarter"
    g3, _ = run.backward(stats)
    assert torch.equal(bits(g1), bits(g3)), "the backward changed what the forward left (q, pi or the sign words)"


# ---- 1. the rank-1 output layer (critic, seed mode 1) ------------------------------------------------------------------
GAMMA = 0.5


def critic_ref(pq, pa, s, a, s2, r, nd, Ng, max_action=1.0, q_next=None):
    """fp64 TD regression of the twin Q (mobody.py:190-207): per-member gradient dicts, tapes, the loss and d = q - y."""
    s, a, s2 = (np.asarray(x, np.float64) for x in (s, a, s2))
    r, nd = np.asarray(r, np.float64)[:, 0], np.asarray(nd, np.float64)[:, 0]
    x = np.concatenate([s, a], 1)
    if q_next is None:
        la = FB.net_weights(pa, "network.")
        pi2 = max_action * np.tanh(np.maximum(np.maximum(s2 @ la[0][0] + la[0][1], 0) @ la[1][0] + la[1][1], 0) @ la[2][0] + la[2][1])
        x2 = np.concatenate([s2, pi2], 1)
        qn = np.minimum(*[FB.input_gradient(FB.net_weights(pq, pre), x2)[0][:, 0] for pre in ("network1.", "network2.")])
    else:
        qn = np.asarray(q_next, np.float64)[:, 0]
    y = r + nd * GAMMA * qn
    out = []
    for pre in ("network1.", "network2."):
        (W1, b1), (W2, b2), (W3, b3) = FB.net_weights(pq, pre)
        z1 = x @ W1 + b1
        z2 = np.maximum(z1, 0) @ W2 + b2
        q = (np.maximum(z2, 0) @ W3 + b3)[:, 0]
        d = q - y
        dz3 = (2.0 * d / Ng)[:, None]
        h1, h2 = np.maximum(z1, 0), np.maximum(z2, 0)
        ref = R.mlp3_backward_ref(W1.T[None], W2.T[None], W3.T[None], x, h1[None], h2[None], dz3[None])
        tape = {pre + "network.0": [dict(x=x, z=z1, dz=ref["dz1"][0])], pre + "network.2": [dict(x=h1, z=z2, dz=ref["dz2"][0])],
                pre + "network.4": [dict(x=h2, z=q[:, None], dz=dz3)],
                "_W": {pre + f"network.{i}.weight": W.T for i, W in ((0, W1), (2, W2), (4, W3))}}
        out.append(dict(grads={pk: ref[rk][0] for rk, pk in R.GRAD_KEYS}, abs={pk: ref["abs_" + rk][0] for rk, pk in R.GRAD_KEYS},
                        tape=tape, d=d, q=q, dz3=dz3, dz2=ref["dz2"][0], h1=h1, h2=h2, z1=z1, z2=z2, y=y))
    loss = sum((o["d"] ** 2).sum() for o in out) / Ng
    return out, loss, dict(r=r, ndq=nd * GAMMA * qn)


def run_critic(pa, pq, batch, S, A, N, Ng, mode, dev, q_next=None):
    """pack -> transposes -> NaN sentinels (gradient, loss, workspace) -> critic_step.  Returns (blob, per-member dicts, loss)."""
    from mobody_amd import _lib, ops, packing
    cfg = dict(gamma=GAMMA, tau=0.005, mfma=mode, max_action=1.0, weight=2.0, bc_coef=1.0, q_weighted=1, scale_Q=1)
    actor = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
    q = packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."])
    actor_T = ops.mlp_transpose(actor, S, A, 1, precision=mode)
    q_T = ops.mlp_transpose(q, S + A, 1, 2, precision=mode)
    dims, hyp = ops.train_dims(S, A, N, 0, Ng, 0), ops.hyper(cfg)
    ws = ops.train_workspace(dims, dev)
    ws.fill_(float("nan"))
    L = _lib.mlp_layout(S + A, 1, 2)
    grad, loss = nan(L.total_floats, dev), nan(1, dev)
    b = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in batch)
    qn = torch.from_numpy(np.ascontiguousarray(q_next)).to(dev) if q_next is not None else None
    ops.critic_step(dims, hyp, actor, q, q_T, q.clone(), b, grad, loss, ws, q_next=qn, actor_blob_T=actor_T, qtarg_blob_T=q_T.clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()), f"{int((~torch.isfinite(grad)).sum())} entries of the gradient blob unwritten / non-finite"
    for m in range(2):
        base = m * L.member_floats
        w1 = packing.wide_unpack(grad[base + L.w1:base + L.w1 + L.Kp1 * 256], L.Kp1)
        w3 = grad[base + L.w3:base + L.w3 + 256 * L.Np3].view(256, L.Np3)
        b3 = grad[base + L.b3:base + L.b3 + L.Np3]
        assert bool((w1[S + A:] == 0).all()), "dW1 padding rows are not exactly 0"
        assert bool((w3[:, 1:] == 0).all()) and bool((b3[1:] == 0).all()), "dW3 / db3 padding columns are not exactly 0"
    g = [{k: v.cpu().numpy() for k, v in d.items()} for d in packing.unpack_mlp(grad, S + A, 1, 2)]
    return grad, g, float(loss.cpu()[0]), (q_T, L)


def f16_bits_ok(x):
    """At most 11 significant bits below the largest magnitude of the value's 32-row tile (as actor_ref.f16_bits_ok)."""
    x = np.abs(np.asarray(x, np.float64))
    tm = FB.tile_max(x)
    m, e = np.frexp(x)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = np.ldexp(1.0, e - 53) * (mi & -mi)
    return not np.any((x > 0) & (tm / np.where(x > 0, low, 1.0) >= 2.0 ** 11))


@functools.lru_cache(maxsize=None)
def int_critic_case(SA, N):
    """Integer twin-Q and actor (pi = 0 exactly), integer batch, gamma = 1/2, N_global = pow2ceil(N): every intermediate is an
    integer multiple of one power of two, every sum of |terms| below 2^24 of it (asserted)."""
    S, A = SA
    seed = 40 + N + 7 * S
    rng = np.random.default_rng(seed)
    pa, pq = AR.int_nets(S, A, seed)
    s, s2 = (rng.integers(-3, 4, (N, S)).astype(np.float32) for _ in range(2))
    a = rng.integers(-2, 3, (N, A)).astype(np.float32)
    r = rng.integers(-3, 4, (N, 1)).astype(np.float32)
    nd = (np.arange(N)[:, None] % 5 != 0).astype(np.float32)
    Ng = AR.pow2ceil(N)
    out, loss, _ = critic_ref(pq, pa, s, a, s2, r, nd, Ng)
    quantum = GAMMA * 2.0 / Ng
    for o in out:
        assert np.array_equal(o["q"], np.rint(o["q"])) and np.array_equal(o["z1"], np.rint(o["z1"]))
        for k, v in o["grads"].items():
            assert AR.dyadic_ok(v, o["abs"][k], quantum), f"{k}: not exact in every order"
        assert f16_bits_ok(o["h1"]) and f16_bits_ok(o["dz2"]), \
            "an operand of the fp16 core keeps more than 11 bits below its tile maximum"
        assert float(np.float32((o["d"] ** 2).sum())) == (o["d"] ** 2).sum()
    assert float(np.float32(loss)) == loss
    return dict(pa=pa, pq=pq, batch=(s, a, s2, r, nd), Ng=Ng, out=out, loss=loss)


@pytest.mark.parametrize("N", RANK1_ROWS)
@pytest.mark.parametrize("SA", SA2, ids=lambda sa: f"S{sa[0]}A{sa[1]}")
def test_critic_rank1_integer_exact(SA, N, mfma, dev):
    from mobody_amd import ops
    S, A = SA
    c = int_critic_case(SA, N)
    grad, g, loss, (q_T, L) = run_critic(c["pa"], c["pq"], c["batch"], S, A, N, c["Ng"], mfma, dev)
    for m in range(2):
        for k, v in c["out"][m]["grads"].items():
            same_bits(g[m][k], v, f"S{S}A{A} N{N} {mfma} member {m} {k}")
    same_bits([loss], [c["loss"]], "q_loss")
    if mfma == "f32":           # the GEMM form of the same tiles: seed mode 0 (dz3 from memory), same activations, same masks
        x = torch.zeros(N, L.Kp1, device=dev)
        x[:, :S + A] = torch.from_numpy(np.concatenate(c["batch"][:2], 1)).to(dev)
        dz3 = torch.zeros(2, N, L.Np3, device=dev)
        dz3[:, :, :1] = torch.from_numpy(np.stack([o["dz3"] for o in c["out"]]).astype(np.float32)).to(dev)
        h1, h2 = (torch.from_numpy(np.stack([o[k] for o in c["out"]]).astype(np.float32)).to(dev) for k in ("h1", "h2"))
        gemm = nan(L.total_floats, dev)
        ops.mlp3_backward(q_T, S + A, 1, 2, dz3, x, h1, h2, gemm)
        torch.cuda.synchronize()
        assert bool((gemm == grad).all()), f"{int((gemm != grad).sum())} elements differ between the rank-1 and the GEMM form"


@functools.lru_cache(maxsize=None)
def real_critic_case(SA, N):
    S, A = SA
    seed = 1500 + N + S
    pa, pq, _ = gu.policy_params(seed, S, A)
    s, a, s2, r, nd = gu.gi.batch(seed + 5, 4 * N, S, A)
    keep = np.flatnonzero(FB.robust_rows(pa, pq, s, a))[:N]
    assert keep.size == N, "too few robust rows in the pool"
    s, a, s2, r, nd = (x[keep].copy() for x in (s, a, s2, r, nd))
    qn = np.random.default_rng(seed + 9).standard_normal((N, 1)).astype(np.float32)        # V(s') handed in (update_q_functions_1)
    Ng = 2 * N
    out, loss, terms = critic_ref(pq, pa, s, a, s2, r, nd, Ng, q_next=qn)
    return dict(pa=pa, pq=pq, batch=(s, a, s2, r, nd), qn=qn, Ng=Ng, out=out, loss=loss, terms=terms)


def real_critic_bounds(c, split):
    """edz3 = (2 / N_global) (E_q + E_y + u |d|) + 4 u |dz3|: the forward bound of q, y = r + nd gamma q_next (three roundings on
    its two terms), the difference, then 2 d (1 / N_global): the reciprocal, two products."""
    x = np.concatenate([c["batch"][0], c["batch"][1]], 1).astype(np.float64)
    Ey = 3 * U * (np.abs(c["terms"]["r"]) + np.abs(c["terms"]["ndq"]))
    gb, Eloss = [], 0.0
    for m, pre in enumerate(("network1.", "network2.")):
        lq, o = FB.net_weights(c["pq"], pre), c["out"][m]
        pad = np.maximum(lq[0][1], 0).max()
        Eq = FB.e2e_bound(x, lq, FB.C_E2E, split, pad)[1][:, 0]
        Ed = Eq + Ey + U * np.abs(o["d"])
        E = (2.0 / c["Ng"] * Ed + 4 * U * np.abs(o["dz3"][:, 0]))[:, None]
        (W1, b1), (W2, b2), _ = lq
        z1, e1 = FB.layer_bound(x, W1, b1, FB.C_E2E)
        _, e2 = FB.layer_bound(np.maximum(z1, 0), W2, b2, FB.C_E2E, split=split, pad=pad)
        gb.append(FB.grad_bounds(o["tape"], FB.C_E2E, split, pre, edz3=E, ex={2: e1, 4: e1 @ np.abs(W2) + e2}))
        Eloss = Eloss + ((2 * np.abs(o["d"]) * Ed + Ed ** 2).sum() + (len(x) + 5) * U * (o["d"] ** 2).sum()) / c["Ng"]
    return gb, Eloss


@pytest.mark.parametrize("N", (33, 65))
@pytest.mark.parametrize("SA", SA2, ids=lambda sa: f"S{sa[0]}A{sa[1]}")
def test_critic_rank1_vs_fp64(SA, N, mfma, dev):
    S, A = SA
    c = real_critic_case(SA, N)
    gb, Eloss = real_critic_bounds(c, mfma == "f16x2")
    _, g, loss, _ = run_critic(c["pa"], c["pq"], c["batch"], S, A, N, c["Ng"], mfma, dev, q_next=c["qn"])
    for m, pre in enumerate(("network1.", "network2.")):
        ratios = {k: AR.ratios(g[m][k], v, gb[m][pre + k]) for k, v in c["out"][m]["grads"].items()}
        print(f"S{S}A{A} N{N} {mfma} member {m}", {k: f"{v:.3g}" for k, v in ratios.items()})
        for k, v in c["out"][m]["grads"].items():
            FB.check(g[m][k], v, gb[m][pre + k], f"S{S}A{A} N{N} {mfma} member {m} {k}")
    FB.check([loss], [c["loss"]], [Eloss], "q_loss")
