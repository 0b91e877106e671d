"""GPU checks of BOSA's second stage: the wide nets' input gradient alone, the derivative of the policy VAE's estimator
with respect to the action (mobody_bosa_loglik_grad), the actor phase through critic_1 (mobody_bosa_actor_forward / _backward), and
the class with config['critic_actor'] -- critic_actor_train against the g28 fixtures of the real reference, train() across the stage
boundary, checkpoints and the CLI.

Tolerances.  dll_da: the project's gradient tolerance, rtol 1e-5 / atol 1e-5 x max |dll_da|; ll: bosa_ref.estimator_tolerance, and the
bits of mobody_bosa_loglik.  Actor gradient: bosa2_ref.grad_tolerance; d loss / d(pre-tanh) -- dpi with the tanh's derivative, read
from the train workspace -- per element at rtol 1e-5 / atol 1e-5 x its largest entry, its padding exactly 0; loss_out[0] at rtol 1e-5
with no atol, on critics whose q_0 has one sign (the loss is +-1) and on one with a quarter of the rows below zero; pi and the
statistics rtol 1e-5 (the signed sum: atol 1e-5 x the sum of magnitudes).  Class: masks exact, scalars rtol 1e-5 with atol 1e-5 x the magnitudes of their terms, parameters
params_close at their lr.  tests/test_bosa_actor_ref.py holds the precondition of the normalised ones: a float32 evaluation of the
fp64 restatement on these inputs stays within half of each.  The reference is computed once per case (tests/bosa_actor_cases.py).

Shapes.  The first cases of every part are the fixture variants' (hidden 8 or 72, at most 33 rows, N 33 and 257).  Each part also
runs where the product runs and at its kernels' edges, with the same checks and tolerances: the input gradient over
tests/test_hip_wide.py's BWD_CASES (hidden up to 1024, members 1 to 8, rows of exactly 16, 64 and 128, in / out of 1 and 256) in three
column ranges each; the estimator's gradient at BC.LLG_WIDE_CASES (hidden 750 x 256 rows, exact GEMM tiles, B = 1 / 255 / 256 / 257 /
513, n = 64, the smallest and the largest policy VAE, pen, ant, beta 0.05) and with a NaN / +Inf row, which must stay in its row; the
actor phase at BC.EDGE_CASES (N = 2, 32, 64, 256, 1024, 1025; (S, A) = (11, 3), (45, 24), (111, 8)) and both split precisions at
BC.SPLIT_CASES; the class over two calls at bs = 128 against the fp64 restatement."""
import json
import os

import numpy as np
import pytest
import torch

import bosa2_ref as B2
import bosa_actor_cases as BC
import bosa_ref as BR
import golden_util as gu
import wide_ref as WR
from test_hip_bosa import GUARD, NAN, Vae, guard_intact
from test_hip_bosa_class import buffers, config_tree, load_scaled, make, same_bits
from test_hip_iql import Net
from test_hip_train import close, params_close
from test_hip_wide import BWD_CASES as WIDE_BWD_CASES, IDS as WIDE_IDS, run_forward as run_wide_forward

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the input gradient alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim,hidden,out_dim,E,rows,cols,per_member", [(23, 72, 6, 1, 99, (17, 23), False), (23, 72, 6, 2, 33, (0, 23), True),
                                                                         (4, 8, 1, 1, 2, (0, 4), False)])
def test_input_grad_has_the_bits_of_the_full_backward(in_dim, hidden, out_dim, E, rows, cols, per_member, dev):
    from mobody_amd import _lib, ops, packing
    p = WR.params(31, in_dim, hidden, out_dim, E)
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    blob = packing.pack_wide(*(p[k] for k in WR.KEYS), dev)
    rng = np.random.default_rng(32)
    x = torch.from_numpy(rng.standard_normal(((E, rows, in_dim) if per_member else (rows, in_dim))).astype(np.float32)).to(dev)
    dz3 = torch.from_numpy(rng.standard_normal((E, rows, out_dim)).astype(np.float32)).to(dev)
    _, sx, h1, h2 = ops.wide_mlp3_forward(blob, L, [x], save=True)
    assert sx.shape[0] == (E if per_member else 1)
    _, want = ops.wide_mlp3_backward(blob, L, dz3, sx, h1, h2, dx_cols=cols)
    n = L.members * rows * (cols[1] - cols[0])
    got = ops.wide_mlp3_input_grad(blob, L, dz3, h1, h2, cols, x_shared=not per_member)
    torch.cuda.synchronize()
    assert got.numel() == n and bits_equal(got, want) and float(want.abs().max()) > 0
    ref = WR.backward(WR.f64(p), WR.bcast(x.cpu().numpy(), E), h1.cpu().numpy()[:, :, :hidden].astype(np.float64),
                      h2.cpu().numpy()[:, :, :hidden].astype(np.float64), dz3.cpu().numpy().astype(np.float64))["dx"][:, :, cols[0]:cols[1]]
    close(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


def column_ranges(in_dim):
    """The full range, the last column alone, and an interior range that starts and ends off a multiple of 16 (the K step of the wide
    GEMM) where in_dim has room for one; in_dim = 1 has the one range."""
    off16 = lambda c, step: c if c % 16 else c + step
    out = [(0, in_dim)] + ([(in_dim - 1, in_dim)] if in_dim > 1 else [])
    c0, c1 = off16(max(in_dim // 3, 1), 1), off16(in_dim - max(in_dim // 4, 1), -1)
    if 0 < c0 < c1 < in_dim:
        assert c0 % 16 and c1 % 16
        out.append((c0, c1))
    return out


@pytest.mark.parametrize("case", WIDE_BWD_CASES, ids=WIDE_IDS(WIDE_BWD_CASES))
def test_input_grad_has_the_bits_of_the_full_backward_at_the_domains_corners(case, dev):
    """tests/test_hip_wide.py's BWD_CASES -- its seven base cases, hidden up to 750, and wide_ref.CORNER_CASES: hidden 8 and 1024,
    members 1 to 8, rows of exactly 16, 64 and 128, in and out of 1 and 256 -- each over column_ranges: dx carries the full
    backward's bits and lies within rtol 1e-5 / atol 1e-5 x max of the fp64 backward (computed once per case)."""
    from mobody_amd import ops
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    p, L, blob, x, out, xs, h1, h2 = run_wide_forward(case, dev)
    dz3 = torch.from_numpy(np.random.default_rng(5).standard_normal((E, rows, out_dim)).astype(np.float32)).to(dev)
    ref = WR.backward(WR.f64(p), WR.bcast(xs.cpu().numpy()[:, :, :in_dim], E), h1.cpu().numpy()[:, :, :hidden].astype(np.float64),
                      h2.cpu().numpy()[:, :, :hidden].astype(np.float64), dz3.cpu().numpy().astype(np.float64))["dx"]
    ranges = column_ranges(in_dim)
    assert len(ranges) == (1 if in_dim == 1 else 3), (in_dim, ranges)
    for c0, c1 in ranges:
        _, want = ops.wide_mlp3_backward(blob, L, dz3, xs, h1, h2, dx_cols=(c0, c1))
        got = ops.wide_mlp3_input_grad(blob, L, dz3, h1, h2, (c0, c1), x_shared=per_member is None)
        torch.cuda.synchronize()
        assert got.shape == (E, rows, c1 - c0) and bits_equal(got, want) and float(want.abs().max()) > 0, (c0, c1)
        r64 = ref[:, :, c0:c1]
        tol = 1e-5 * np.abs(r64) + 1e-5 * np.abs(r64).max()
        worst = float((np.abs(got.cpu().numpy() - r64) / tol).max())
        WORST["input_grad"] = max(WORST.get("input_grad", 0.0), worst)
        print("input_grad h%d rows %d E %d %dx%d cols [%d, %d): worst error / tolerance %.4f (so far %.4f)" %
              (hidden, rows, E, in_dim, out_dim, c0, c1, worst, WORST["input_grad"]))
        close(got, r64, rtol=1e-5, atol=1e-5 * np.abs(r64).max())


# ---- 2. the estimator's gradient ---------------------------------------------------------------------------------------------------
class Llg:
    """The policy VAE of a case on the device and one mobody_bosa_loglik_grad call with guarded buffers."""

    def __init__(self, c, dev, enc=None):
        from mobody_amd import ops
        n, B, ma, beta = c[1], c[2], c[3], (c[4] if len(c) > 4 else BC.BETA)
        S, A, H, enc0, dec, s, a, eps = BC.llg_case(*c)
        self.v = Vae("policy", (S, A, H, 1, B), dev, seed=BC.VAE_SEED, beta=beta, max_action=ma, num_samples=n)
        if enc is not None:
            from mobody_amd import packing
            self.v.blob[:self.v.n_enc] = packing.pack_wide(*(enc[k] for k in WR.KEYS), dev).reshape(-1)
        words = ops.bosa_loglik_grad_workspace(self.v.block(), dev).numel()
        self.buf = torch.full((words + GUARD,), NAN, device=dev)
        self.ws, self.B, self.A, self.n, self.dev = self.buf[:words], B, A, n, dev
        self.s, self.a, self.eps = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (s, a, eps))

    def run(self, eps="given", **ff):
        from mobody_amd import ops
        B, A, n = self.B, self.A, self.n
        ll, w = torch.full((1, B), NAN, device=self.dev), torch.full((1, n, B), NAN, device=self.dev)
        dbuf = torch.full((B * A + 1,), NAN, device=self.dev)
        e = self.eps if isinstance(eps, str) else eps
        ops.bosa_loglik_grad(self.v.block(state=self.s, action=self.a, eps=e, ll=ll, w_out=w, workspace=self.ws, **ff), dbuf[:-1])
        torch.cuda.synchronize()
        assert guard_intact(self.buf) and bool(torch.isnan(dbuf[-1])), "mobody_bosa_loglik_grad wrote behind a buffer"
        return dbuf[:-1].reshape(B, A), ll, w

    def forward_only(self):
        from mobody_amd import ops
        ll, w = torch.full((1, self.B), NAN, device=self.dev), torch.full((1, self.n, self.B), NAN, device=self.dev)
        ops.bosa_loglik(self.v.block(state=self.s, action=self.a, eps=self.eps, ll=ll, w_out=w, workspace=self.v.ws))
        torch.cuda.synchronize()
        return ll, w


@pytest.mark.parametrize("c", BC.LLG_CASES, ids=BC.llg_id)
def test_loglik_grad_vs_fp64(c, dev):
    check_llg(c, dev)


@pytest.mark.parametrize("c", BC.LLG_WIDE_CASES, ids=BC.llg_id)
def test_loglik_grad_vs_fp64_at_the_product_shape_and_the_kernels_edges(c, dev):
    """The same checks at BC.LLG_WIDE_CASES: hidden 750 with 256 rows (n B = 256 and 2560, exact 64-row tiles of the wide GEMM) and 513
    rows (a third workgroup of the row-wise kernels); B = 1, 255, 256, 257 (the first and last thread of a workgroup of
    k_bosa_llg_seed); n B = 128; n = 64 at A = 1 and at walker shapes; the smallest layout; the largest policy VAE (4 A = 256 encoder
    outputs, 256 decoder inputs) at hidden 8 and 1024; pen and ant at hidden 750; and beta 0.05, whose softmax is sharply peaked
    (|w| up to 360, 38 nats within a row) and whose direct term is ten times larger.  beta 0.01 is not run: at hidden 750 a float32
    evaluation of the restatement itself is 2.1 times over the gradient tolerance, which is then out of fp32's reach."""
    check_llg(c, dev)


def check_llg(c, dev):
    d64, ll64, ex = BC.llg_reference(*c)
    k = Llg(c, dev)
    d, ll, w = k.run()
    ll0, w0 = k.forward_only()
    assert bits_equal(ll, ll0) and bits_equal(w, w0), "ll / w_out differ from mobody_bosa_loglik's"
    tol_d, tol_ll = BC.llg_tolerances(d64, ll64, ex["w"])
    rd = float((np.abs(d.cpu().numpy() - d64) / tol_d).max())
    rl = float((np.abs(ll.cpu().numpy()[0] - ll64) / tol_ll).max())
    WORST["dll_da"], WORST["ll"] = max(WORST.get("dll_da", 0.0), rd), max(WORST.get("ll", 0.0), rl)
    print("%s: dll_da worst error / tolerance %.4f, ll %.4f (so far %.4f, %.4f)" % (BC.llg_id(c), rd, rl, WORST["dll_da"], WORST["ll"]))
    assert rd <= 1.0 and rl <= 1.0
    S, A, H = BC.llg_shape(c[0])
    p = p_of(k, S, A, H)
    # p_k = exp(w_k - logsumexp(w)): w_k and the logsumexp are each within estimator_tolerance's 1e-5 x max_s |w_s| of the row, so to
    # first order p_k is within p_k x twice that; p_k <= 1, and a factor 2 covers the second order and the exp / divide roundings
    assert (np.abs(p - ex["p"]) <= 4e-5 * np.abs(ex["w"]).max(0)[None] + 1e-6).all()
    # n <= 10 terms of at most 1, each rounded once: 2e-6; for n = 64 the same count of roundings, (n + 10) 2^-24
    np.testing.assert_allclose(p.sum(0), 1.0, rtol=0, atol=2e-6 if c[1] <= 10 else (c[1] + 10) * 2.0 ** -24)
    if c[1] == 1:                                  # one sample: p is exactly 1 on the device too
        assert (p == 1.0).all() and (ex["p"] == 1.0).all()


def p_of(k, S, A, H):
    """The device's p_k [n, B]: the second slot of the pairs pq [n B][2], the last piece of mobody_bosa_workspace's part."""
    off = BC.pq_offset(S, A, H, k.B, k.n)
    return k.ws[off:off + 2 * k.n * k.B].reshape(k.n, k.B, 2)[:, :, 1].cpu().numpy()


denc_offset = BC.denc_offset                    # tests/test_bosa_actor_ref.py ties it to the library's totals


def test_loglik_grad_at_the_clamp_edges(dev):
    """As test_reparam_kernel_at_the_clamp_edges: the log_std head's W3 columns are zero and its biases planted at -4, 15, just
    outside each and inside, so the pre-clamp values are those floats exactly.  Outside columns give exactly 0 through that head,
    the ends pass."""
    f32 = np.float32
    edges = np.array([f32(-4 - 1e-3), f32(-4 + 1e-3), f32(-4), f32(15 - 1e-3), f32(15 + 1e-3), f32(15), f32(-30), f32(0.3), f32(-2.5), f32(40),
                      f32(-4), f32(-3.0)], f32)
    passes = np.array([0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1], bool)
    c = ("small", 3, 33, 1.0)
    S, A, H, enc, dec, s, a, eps = BC.llg_case(*c)
    Lz = 2 * A
    assert len(edges) == Lz and ((edges >= -4) & (edges <= 15)).tolist() == passes.tolist()
    enc = {k: v.copy() for k, v in enc.items()}
    enc["W3"][:, :, Lz:] = 0
    enc["b3"][:, Lz:] = edges
    # std is e^15 (or nearly) on four columns: their noise is zero, so that z stays where the decoder is not saturated
    eps = eps.copy()
    eps[:, :, edges > 10] = 0
    k = Llg(c, dev, enc=enc)
    k.eps = torch.from_numpy(eps).to(dev)
    d, ll, _ = k.run()
    d64, ll64, ex = B2.loglik_grad_action(enc, dec, s, a, eps, BC.BETA, 1.0)
    assert (ex["pre"] == edges.astype(np.float64)).all()
    denc = k.ws[denc_offset(S, A, H, 33, 3):][:33 * 2 * Lz].reshape(33, 2 * Lz).cpu().numpy()
    head = denc[:, Lz:]
    assert (head[:, ~passes] == 0).all() and (head[:, passes] != 0).all()
    scale = np.abs(ex["denc"]).max()
    np.testing.assert_allclose(denc, ex["denc"], rtol=1e-5, atol=1e-5 * scale)
    tol_d, tol_ll = BC.llg_tolerances(d64, ll64, ex["w"])
    assert (np.abs(d.cpu().numpy() - d64) <= tol_d).all() and (np.abs(ll.cpu().numpy()[0] - ll64) <= tol_ll).all()


@pytest.mark.parametrize("where", ("state", "action"))
@pytest.mark.parametrize("value", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_loglik_grad_keeps_a_non_finite_row_to_itself(where, value, dev):
    """One row of the state (or of the action) is NaN or +Inf: the call returns, the guard words are intact, and every OTHER row's
    dll_da, ll and w_out carry the bits of the unplanted run -- every kernel on the path is row-wise or a GEMM whose output row reads
    one input row.  What the planted row itself holds is not asserted (DESIGN 5u leaves three differences from torch on non-finite
    values open)."""
    k = Llg(("small", 3, 33, 1.0), dev)
    clean = [t.clone() for t in k.run()]
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    row = 7
    (k.s if where == "state" else k.a)[row] = value
    d, ll, w = k.run()                              # asserts the guard words
    keep = torch.arange(k.B, device=dev) != row
    assert bits_equal(d[keep], clean[0][keep]), "a non-finite row reached another row's dll_da"
    assert bits_equal(ll[:, keep], clean[1][:, keep]) and bits_equal(w[:, :, keep], clean[2][:, :, keep])


def test_loglik_grad_repeats_its_bits_and_draws_the_stream_itself(dev):
    from mobody_amd import _lib, ops
    c = ("small", 3, 33, 1.0)
    k = Llg(c, dev)
    one, two = k.run(), k.run()
    assert all(bits_equal(x, y) for x, y in zip(one, two))
    seed, call = 77, 5
    B, n, Lz = 33, 3, 12
    drawn = ops.rng_normal(seed, _lib.BOSA_STREAMS["policy_ll"], call, B * n * Lz, dev).reshape(B, n, Lz)
    implicit, explicit = k.run(eps=None, seed=seed, call=call), k.run(eps=drawn)
    assert all(bits_equal(x, y) for x, y in zip(implicit, explicit)) and not bits_equal(implicit[0], one[0])


# ---- 3. the actor phase ------------------------------------------------------------------------------------------------------------
dz3a_offset = BC.dz3a_offset                    # likewise, against mobody_train_workspace


class ActorPhase:
    def __init__(self, N, dev, mode="f32", ma=1.0, shift=0.0, qcut=0.0, SA=BC.ACTOR_SA):
        from mobody_amd import _lib, ops
        S, A = SA
        pa, pq, _, _, s, _ = BC.actor_case(N, ma, shift, qcut, SA)
        self.a = Net({"network." + k: v for k, v in pa.items()}, S, A, 1, dev, mode)
        self.q = Net(pq, S + A, 1, 2, dev, mode)
        self.gbuf = torch.full((self.a.blob.numel() + 1,), NAN, device=dev)
        self.a.grad = self.gbuf[:-1]
        self.dims = ops.train_dims(S, A, N, N)
        self.hyp = _lib.MobodyHyper(0.99, 0.005, ma, 1.0, 0.0, 0, 1, ops.prec_id(mode))
        self.ws = ops.train_workspace(self.dims, dev)
        self.stats, self.loss = torch.full((3,), NAN, device=dev), torch.full((3,), NAN, device=dev)
        self.pibuf = torch.full((N * A + 1,), NAN, device=dev)
        self.s, self.N, self.S, self.A, self.dev, self.mode = torch.from_numpy(s).to(dev), N, S, A, dev, mode

    def forward(self):
        from mobody_amd import ops
        ops.bosa_actor_forward(self.dims, self.hyp, self.a.blob, self.q.blob, self.s, self.stats[:2], self.pibuf[:-1], self.ws,
                               actor_blob_T=self.a.blob_T, q_blob_T=self.q.blob_T)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.pibuf[-1])) and bool(torch.isnan(self.stats[2]))
        return self.pibuf[:-1].reshape(self.N, self.A)

    def backward(self, extra, **opt):
        from mobody_amd import ops
        kw = opt or dict(grad_actor=self.a.grad)
        ops.bosa_actor_backward(self.dims, self.hyp, self.a.blob, self.a.blob_T, self.q.blob, self.q.blob_T, self.s, self.stats[:2], extra,
                                self.loss[:2], self.ws, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.gbuf[-1])) and bool(torch.isnan(self.loss[2]))
        return self.loss[:2].cpu().numpy()

    def seed(self):
        """d loss / d(pre-tanh) as the backward left it: (its A real columns [N, A], its padding columns)."""
        off, Np3 = dz3a_offset(self.S, self.A, self.N)
        d = self.ws[off:off + self.N * Np3].reshape(self.N, Np3).cpu().numpy()
        return d[:, :self.A], d[:, self.A:]


def check_actor(N, dev, mode, ma, shift, lamda, qcut=0.0, SA=BC.ACTOR_SA):
    logs, g64, ex = BC.actor_reference(N, ma, shift, lamda, qcut=qcut, SA=SA)
    # what the class hands over: -(lamda / N) dll_da, recorded from the fp64 restatement and rounded to float32
    extra = torch.from_numpy(BC.actor_extra(N, ma, shift, lamda, qcut, SA)).to(dev)
    k = ActorPhase(N, dev, mode, ma, shift, qcut, SA)
    pi = k.forward().cpu().numpy()
    stats = k.stats[:2].cpu().numpy().astype(np.float64)
    sum_abs, sum_q = np.abs(ex["q"]).sum(), ex["q"].sum()
    close(pi, ex["pi"], rtol=1e-5, atol=1e-5 * ma)
    close(stats[0], sum_abs, rtol=1e-5, atol=0)
    close(stats[1], sum_q, rtol=1e-5, atol=1e-5 * sum_abs)
    loss = k.backward(extra)
    head = -ex["norm_q"] * ex["q"].mean()
    print("actor N=%d mode=%s qcut=%g: loss_out[0] %.8g / %.8g, relative error / 1e-5 %.4f" % (N, mode, qcut, loss[0], head, abs(loss[0] - head) / abs(head) / 1e-5))
    close(float(loss[0]), head, rtol=1e-5, atol=0)
    assert loss[1] == 0
    # dpi per element, as the seed of the actor's backward: (dq/da + dpi_extra) max_action (1 - (pi / max_action)^2); padding exactly 0
    d64 = BC.pre_tanh_seed(ex, ma)
    got_d, pad = k.seed()
    rs = float((np.abs(got_d - d64) / BC.seed_tolerance(d64)).max())
    print("actor N=%d (S, A)=%s mode=%s ma=%g shift=%g lamda=%g qcut=%g: d(pre-tanh) per element, worst error / tolerance %.4f" %
          (N, SA, mode, ma, shift, lamda, qcut, rs))
    assert rs <= 1.0 and pad.shape[1] > 0 and (pad == 0).all() and np.abs(d64).max() > 0
    want = B2.to_state_dict(g64, ("network.",))
    got = k.a.unpack(k.a.grad)
    scale = max(float(np.abs(v).max()) for v in want.values())
    worst = max(float((np.abs(got[name] - v) / (1e-5 * np.abs(v) + 1e-5 * scale)).max()) for name, v in want.items())
    print("actor N=%d (S, A)=%s mode=%s ma=%g shift=%g lamda=%g: gradient worst error / tolerance %.4f" % (N, SA, mode, ma, shift, lamda, worst))
    assert worst <= 1.0 and scale > 0
    return k, extra


@pytest.mark.parametrize("N", BC.ACTOR_ROWS)
def test_actor_phase_vs_fp64(N, dev):
    check_actor(N, dev, "f32", 1.0, 0.0, BC.ACTOR_LAMDA)
    check_actor(N, dev, "f32", 1.0, 0.0, 0.0)                    # dpi_extra = 0: the Q term alone
    check_actor(N, dev, "f32", 1.0, 100.0, BC.ACTOR_LAMDA)       # critic_2 below critic_1 on every row: Q is member 0, not the minimum
    check_actor(N, dev, "f32", 1.0, 0.0, BC.ACTOR_LAMDA, qcut=0.25)   # a quarter of the rows with q_0 < 0: the loss is not +-1
    check_actor(N, dev, "f32", 1.0, 0.0, 0.0, qcut=0.25)


def test_actor_phase_with_a_wider_action_range(dev):
    check_actor(33, dev, "f32", 2.0, 0.0, BC.ACTOR_LAMDA)


@pytest.mark.parametrize("c", BC.EDGE_CASES, ids=BC.edge_id)
def test_actor_phase_vs_fp64_at_row_edges_and_other_widths(c, dev):
    """BC.EDGE_CASES: at (17, 6) the smallest N, one and two exact 32-row tiles, the product's 256, and 1024 / 1025 -- the 1024-thread
    stride of k_bosa_actor_stats takes its second trip at row 1025; at N = 65 a narrow net, pen's A = 24 and ant's S = 111.  At 256
    and 1025 rows also with a quarter of the rows below zero, so that the loss is not +-1."""
    N, SA = c
    check_actor(N, dev, "f32", 1.0, 0.0, BC.ACTOR_LAMDA, SA=SA)
    if N in BC.QCUT_ROWS and SA == BC.ACTOR_SA:
        check_actor(N, dev, "f32", 1.0, 0.0, BC.ACTOR_LAMDA, qcut=0.25)


@pytest.mark.parametrize("c", BC.SPLIT_CASES, ids=BC.edge_id)
@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_actor_phase_split_precisions_at_the_product_rows_and_pen(mode, c, dev):
    """The fp32-grade split modes at the exact-fp32 bounds, as test_actor_phase_precisions holds them at 257 rows."""
    check_actor(c[0], dev, mode, 1.0, 0.0, BC.ACTOR_LAMDA, SA=c[1])


def test_actor_phase_fused_form_is_the_gradient_form_plus_adam(dev):
    N, lr = 257, 3e-4
    _, extra = check_actor(N, dev, "f32", 1.0, 0.0, BC.ACTOR_LAMDA)
    two = ActorPhase(N, dev)
    one = ActorPhase(N, dev)
    for t in (1, 2):
        two.forward(), one.forward()
        la = two.backward(extra)
        two.a.adam(t, lr, "f32")
        lb = one.backward(extra, m=one.a.am, v=one.a.av, t=t, lr=lr)
        torch.cuda.synchronize()
        assert np.array_equal(la.view(np.int32), lb.view(np.int32))
        for x, y in ((two.a.blob, one.a.blob), (two.a.am, one.a.am), (two.a.av, one.a.av), (two.a.blob_T, one.a.blob_T)):
            assert bits_equal(x, y)
    assert not bits_equal(one.a.blob, ActorPhase(N, dev).a.blob)


@pytest.mark.parametrize("mode", ["default", "f16x2", "bf16x3", "bf16x2", "bf16"])
def test_actor_phase_precisions(mode, dev):
    """The fp32-grade modes (and the build's default) at the exact-fp32 bounds, as every `mfma`-parametrised suite holds them; the
    two lower modes are refused by name."""
    from mobody_amd import _lib, ops
    mode = ops.default_mfma() if mode == "default" else mode
    if mode in ("bf16x2", "bf16"):
        k = ActorPhase(33, dev, mode)
        with pytest.raises(_lib.MobodyError, match=r"precision \d: must be one of 0 \(f32\), 3 \(bf16x3\), 4 \(f16x2\)"):
            k.forward()
        return
    check_actor(257, dev, mode, 1.0, 0.0, BC.ACTOR_LAMDA)


# ---- 4. the class ------------------------------------------------------------------------------------------------------------------
T = lambda p: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()}


def nets_state(pol):
    """Everything a stage-2 call reads or writes, by name.  Of a target's T blob only the W2 planes follow the Polyak update (nothing
    else of it is read by a forward), so the targets enter with their parameter blobs alone."""
    out = {"vae_policy": pol.vae_policy.blob, "vae_dyna": pol.vae_dyna.blob, "scalars": pol._s2}
    for name, n in (("actor", pol.actor), ("critic", pol.critic), ("actor_target", pol.actor_target), ("critic_target", pol.critic_target)):
        out[name] = n.blob
        if not name.endswith("target"):
            out[name + ".T"] = n.blob_T
    for name, opt in (("actor_optimizer", pol.actor_optimizer), ("critic_optimizer", pol.critic_optimizer)):
        out[name + ".m"], out[name + ".v"] = opt.m, opt.v
    return {k: v.clone() for k, v in out.items()}


def differing(a, b, skip=()):
    return [k for k in a if k not in skip and not bits_equal(a[k], b[k])]


@pytest.mark.parametrize("tag", ("small", "tiny"))
def test_critic_actor_train_vs_reference_fixture(tag, dev):
    from mobody_amd.algo.call_algo import call_algo
    g, cfg, vaes, actor_sd, q_sd, mixed = BC.g28_setup(tag)
    S, A, H, E, bs = BR.VARIANTS[tag]
    pol = call_algo("bosa", dict(cfg, critic_actor=1), 3, dev)
    for vae, nets in ((pol.vae_policy, vaes[0]), (pol.vae_dyna, vaes[1])):
        vae.load_state_dict(T(BR.state_dict(*nets, vae.kind)))
    for n in (pol.actor, pol.actor_target):
        n.load_state_dict(T(actor_sd))
    for n in (pol.critic, pol.critic_target):
        n.load_state_dict(T(q_sd))
    call = [0]
    kinds = {"target": "target", "dynamics_ll": "dynamics", "policy_ll": "policy"}
    pol.noise_fn = lambda kind, shape: np.asarray(g["c%d_noise_%s" % (call[0], kinds[kind])], np.float32).reshape(shape)
    targets = lambda: [pol.actor_target.blob.clone(), pol.critic_target.blob.clone()]
    for call[0] in (1, 2, 3, 4):
        before = targets()
        pol.critic_actor_train(mixed)
        torch.cuda.synchronize()
        actor_call = call[0] % 2 == 0
        assert pol.total_it == int(g["c%d_total_it" % call[0]]) == call[0]
        assert pol.critic_optimizer.t == call[0] and pol.actor_optimizer.t == call[0] // 2
        assert np.array_equal(pol._keep2[2].cpu().numpy(), g["c%d_mask" % call[0]])
        log = pol.stage2_log()
        want = {k: float(g["c%d_log::%s" % (call[0], k)]) for k in B2.STAGE2_SCALARS[:8 if actor_call else 4]}
        terms = BC.scalar_terms(want, cfg)
        for k, v in want.items():
            print("%s call %d %s: %.7g / %.7g" % (tag, call[0], k, log[k], v))
            close(log[k], v, rtol=1e-5, atol=1e-5 * terms[k])
        assert same_bits(before, targets()) != actor_call, "the targets move on actor calls, and only then"
    sds = {"actor": pol.actor.state_dict(), "actor_target": pol.actor_target.state_dict(), "critic_1": pol.critic_1.state_dict(),
           "critic_2": pol.critic_2.state_dict(), "critic_1_target": pol.critic_1_target.state_dict(), "critic_2_target": pol.critic_2_target.state_dict()}
    for name, sd in sds.items():
        lr = cfg["actor_lr" if name.startswith("actor") else "critic_lr"]
        assert len(sd) == 6
        for k, v in sd.items():
            params_close(gu.sub(v.cpu().numpy()), g["c4_p::%s::%s" % (name, k.replace("network.", "net."))], lr)


def test_critic_actor_train_at_the_product_batch_vs_the_restatement(dev):
    """bs = 128 (256 mixed rows), walker shapes, VAEs 72 wide, E = 2, two calls, the second an actor call (BC.batch_setup).  The
    expectation is the fp64 RESTATEMENT (tests/bosa2_ref.py composed by BC.stage2_calls), not the real reference: nets from
    gu.gi.mlp_params / BR.vae_params, noise from a seeded NumPy generator through noise_fn.  g28 above stays the tie to the reference;
    this holds the class at the batch the product runs, with the same assertions."""
    from mobody_amd.algo.call_algo import call_algo
    cfg, vaes, actor_sd, q_sd, mixed, _ = BC.batch_setup()
    per_call, st = BC.batch_reference()
    S, A, H, E, bs = BC.BATCH_SHAPE
    pol = call_algo("bosa", dict(cfg, critic_actor=1), 3, dev)
    for vae, nets in ((pol.vae_policy, vaes[0]), (pol.vae_dyna, vaes[1])):
        vae.load_state_dict(T(BR.state_dict(*nets, vae.kind)))
    for n in (pol.actor, pol.actor_target):
        n.load_state_dict(T(actor_sd))
    for n in (pol.critic, pol.critic_target):
        n.load_state_dict(T(q_sd))
    call = [0]
    pol.noise_fn = lambda kind, shape: BC.batch_noise(call[0], cfg)[kind].reshape(shape)
    targets = lambda: [pol.actor_target.blob.clone(), pol.critic_target.blob.clone()]
    for call[0], want, mask in per_call:
        before = targets()
        pol.critic_actor_train(mixed)
        torch.cuda.synchronize()
        actor_call = call[0] % 2 == 0
        assert pol.total_it == call[0] and pol.critic_optimizer.t == call[0] and pol.actor_optimizer.t == call[0] // 2
        assert np.array_equal(pol._keep2[2].cpu().numpy().reshape(-1), mask.astype(np.float32)) and len(mask) == 2 * bs
        log = pol.stage2_log()
        names = B2.STAGE2_SCALARS[:8 if actor_call else 4]
        assert list(log) == list(names)
        terms = BC.scalar_terms(want, cfg)
        for k in names:
            print("batch call %d %s: %.7g / %.7g, error / tolerance %.4f" % (call[0], k, log[k], want[k], abs(log[k] - want[k]) / (1e-5 * abs(want[k]) + 1e-5 * terms[k] + 1e-300)))
            close(log[k], want[k], rtol=1e-5, atol=1e-5 * terms[k])
        assert same_bits(before, targets()) != actor_call, "the targets move on actor calls, and only then"
    assert call[0] == 2
    ref = {"actor": B2.to_state_dict(st["actor"], ("",)), "actor_target": B2.to_state_dict(st["actor_target"], ("",))}
    for j in (1, 2):
        for name, key in (("critic_%d" % j, "critic"), ("critic_%d_target" % j, "critic_target")):
            ref[name] = {k[len("network%d." % j):]: v for k, v in B2.to_state_dict(st[key]).items() if k.startswith("network%d." % j)}
    sds = {"actor": pol.actor.state_dict(), "actor_target": pol.actor_target.state_dict(), "critic_1": pol.critic_1.state_dict(),
           "critic_2": pol.critic_2.state_dict(), "critic_1_target": pol.critic_1_target.state_dict(), "critic_2_target": pol.critic_2_target.state_dict()}
    for name, sd in sds.items():
        lr = cfg["actor_lr" if name.startswith("actor") else "critic_lr"]
        assert len(sd) == 6 and sorted(k.replace("net.", "network.") for k in sd) == sorted(ref[name]), (name, sorted(sd), sorted(ref[name]))
        for k, v in sd.items():
            params_close(v.cpu().numpy(), ref[name][k.replace("net.", "network.")], lr)


def run_train(dev, graph, calls, **over):
    pol = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3, graph=graph, **over)
    load_scaled(pol)
    src, tar = buffers(dev, rng="device", seed=9)
    seq = []
    for _ in range(calls):
        pol.train(src, tar, 8, None, None)
        seq.append((pol.total_it, pol.critic_optimizer.t, pol.actor_optimizer.t))
    torch.cuda.synchronize()
    return pol, src, tar, seq


def test_train_crosses_the_stage_boundary_and_runs_stage_two_eagerly(dev):
    """vae_iteration = 4: two VAE calls (total_it 2, 4), then stage-2 calls counting once each; the actor steps at even total_it.
    graph = 1 replays the VAE stage and still runs stage 2 eagerly, with the bits of graph = 0."""
    (e, es, et, seq_e), (g, gs, gt, seq_g) = run_train(dev, 0, 6), run_train(dev, 1, 6)
    assert seq_e == seq_g == [(2, 0, 0), (4, 0, 0), (5, 1, 0), (6, 2, 1), (7, 3, 1), (8, 4, 2)]
    assert e.vae_policy_optimizer.t == e.vae_dyna_optimizer.t == 2 and g._graph is None and e.max_train_steps() == float("inf")
    assert differing(nets_state(e), nets_state(g)) == [], "stage 2 after a replayed VAE stage differs from the eager run"
    assert (e._noise_calls, es._draws, et._draws) == (g._noise_calls, gs._draws, gt._draws)
    log = e.stage2_log()
    assert list(log) == list(B2.STAGE2_SCALARS) and all(np.isfinite(v) for v in log.values()) and log["lamda_policy"] == 0.25
    assert "critic_loss" in e.log_line() and len(e.losses()) == 3
    fresh = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3)
    assert not same_bits([fresh.actor.blob, fresh.critic.blob], [e.actor.blob, e.critic.blob])
    assert not same_bits([e.actor_target.blob], [e.actor.blob])


def test_train_draws_the_source_first_and_logs_the_stage_scalars(dev, monkeypatch):
    pol = make(dev, vae_iteration=0, critic_actor=1)
    load_scaled(pol)
    src, tar = buffers(dev)
    order, seen, normal = [], [], []
    randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *shape, **kw: (normal.append(tuple(shape)), randn(*shape, **kw))[1])
    for name, rb in (("src", src), ("tar", tar)):
        rb.draw_indices = (lambda n, rb=rb, name=name, f=rb.draw_indices: (order.append(name), f(n))[1])

    class W:
        def add_scalar(self, k, v, step):
            seen.append((k, v, step))
    pol.total_it = 4998
    pol.train(src, tar, 8, W(), None)
    assert pol.total_it == 4999 and not seen and pol.actor_optimizer.t == 0
    pol.train(src, tar, 8, W(), None)
    assert pol.total_it == 5000 and pol.actor_optimizer.t == 1 and order == ["src", "tar"] * 2
    # torch's generator in the reference's order: target noise, the dynamics estimator, and on the actor call the policy estimator
    N, n, E = 16, 4, 2
    S, A = BC.ACTOR_S, BC.ACTOR_A
    assert normal == [(N, A), (n, E, N, 2 * S), (N, A), (n, E, N, 2 * S), (N, n, 2 * A)]
    assert [k for k, _, _ in seen] == ["train/" + k for k in B2.STAGE2_SCALARS] and {s for _, _, s in seen} == {5000}
    assert all(np.isfinite(v) for _, v, _ in seen)
    before = nets_state(pol)
    pol.train(src, tar, 65, W(), None)                          # a short buffer: total_it counts once and nothing else happens
    assert pol.total_it == 5001 and differing(before, nets_state(pol)) == [] and len(seen) == 8


def test_without_the_key_the_boundary_refusal_is_what_it_was(dev):
    pol = make(dev, vae_iteration=0)
    src, tar = buffers(dev)
    assert pol.max_train_steps() == 0 and not pol.critic_actor and not hasattr(pol, "critic")
    with pytest.raises(NotImplementedError, match="critic / actor stage is not built"):
        pol.train(src, tar, 8, None, None)
    assert pol.total_it == 0
    from test_bosa_ref import bosa_config
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline import bosa
    for key in bosa.STAGE2_KEYS:                    # the constructor, after its other checks and before anything is built
        built = []
        with pytest.raises(NotImplementedError, match=r"BOSA is built from a BOSA config only: config lacks \['%s'\]" % key):
            orig = bosa._WideVae.__init__
            try:
                bosa._WideVae.__init__ = lambda self, *a, **k: built.append(a)
                call_algo("bosa", {k: v for k, v in bosa_config(critic_actor=1).items() if k != key}, 3, dev)
            finally:
                bosa._WideVae.__init__ = orig
        assert not built
    call_algo("bosa", {k: v for k, v in bosa_config().items() if k not in bosa.STAGE2_KEYS}, 3, dev)     # unkeyed: none of them is needed


def test_checkpoints_resume_bit_for_bit(dev, tmp_path):
    from mobody_amd.algo.offline_offline.bosa import STAGE2_FILES, TARGET_FILES
    g, gs, gt, _ = run_train(dev, 0, 6)
    prefix = str(tmp_path / "model")
    g.save(prefix)
    vae_files = ["_vae_dynamics", "_vae_dynamics_optimizer", "_vae_policy", "_vae_policy_optimizer"]
    assert sorted(os.listdir(tmp_path)) == sorted("model" + f for f in vae_files + list(STAGE2_FILES) + list(TARGET_FILES)) and len(os.listdir(tmp_path)) == 13
    assert list(torch.load(prefix + "_critic_2", weights_only=True)) == ["net.%d.%s" % (i, w) for i in (0, 2, 4) for w in ("weight", "bias")]
    assert list(torch.load(prefix + "_actor", weights_only=True)) == ["net.%d.%s" % (i, w) for i in (0, 2, 4) for w in ("weight", "bias")]
    sd = torch.load(prefix + "__critic_2_optimizer", weights_only=True)
    assert sorted(sd["state"]) == list(range(6)) and float(sd["state"][0]["step"]) == 4 and sd["param_groups"][0]["lr"] == 3e-4
    fresh = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3)
    fresh.load(prefix)
    assert differing(nets_state(fresh), nets_state(g), skip=("scalars",)) == []
    assert (fresh.critic_optimizer.t, fresh.actor_optimizer.t) == (4, 2)
    fresh.total_it, fresh._noise_calls = g.total_it, g._noise_calls
    fs, ft = buffers(dev, rng="device", seed=9)
    fs._draws, ft._draws = gs._draws, gt._draws
    for _ in range(2):
        fresh.train(fs, ft, 8, None, None)
        g.train(gs, gt, 8, None, None)
    torch.cuda.synchronize()
    assert fresh.total_it == 10 and differing(nets_state(fresh), nets_state(g)) == []
    # the reference's ten files alone: the targets are copies of the online nets
    g.save(prefix)
    for f in TARGET_FILES:
        os.remove(prefix + f)
    ten = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3)
    ten.load(prefix)
    assert same_bits([ten.actor_target.blob, ten.critic_target.blob, ten.actor_target.blob_T, ten.critic_target.blob_T],
                     [g.actor.blob, g.critic.blob, ten.actor.blob_T, ten.critic.blob_T])
    assert not same_bits([g.actor_target.blob], [g.actor.blob])


def test_cli_runs_past_the_vae_stage_with_the_key(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.bosa import BOSA, vae_steps
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: pytest.fail("BOSA builds no dynamics"))
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path, vae_iteration=5, batch_size=16, critic_actor=1))
    out_dir = tmp_path / "out"
    argv = ["--policy", "BOSA", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", "1",
            "--rng", "device", "--src_rows", "300", "--tar_rows", "200", "--save-model", "--eval_freq", "3", "--log_every", "2",
            "--dir", str(out_dir), "--params", json.dumps(dict(graph=1))]
    n = vae_steps(5)
    pol = tm.main(argv + ["--max_step", str(n + 4)])
    assert n == 2 and isinstance(pol, BOSA) and pol.total_it == 2 * n + 4 and pol.critic_optimizer.t == 4 and pol.actor_optimizer.t == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3 and "VAE_Policy/vae_loss" in lines[0] and all("critic_loss" in ln and "actor_loss" in ln for ln in lines[1:])
    files = sorted({f for _, _, fs in os.walk(out_dir) for f in fs if f.startswith("model_")})
    assert len(files) == 13 and "model__critic_2_optimizer" in files and "model_critic_1_target" in files
    # without the key the early refusal is what it was
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path, vae_iteration=5, batch_size=16))
    with pytest.raises(SystemExit, match="the largest max_step is 2"):
        tm.main(argv + ["--max_step", str(n + 1)])
