"""GPU checks of BOSA's VAE stage (csrc/bosa.hip) against the fp64 restatement tests/bosa_ref.py.

Tolerances.  VAE step: losses rtol 1e-5; gradients rtol 1e-5 / atol 1e-5 x the tensor's largest entry; parameters over three fused
steps params_close at the VAE's lr.  The reparameterisation kernel alone, per element (u = 2^-24): std = expf(clamped) is within two
units in the last place (4 u), so z = mean + std eps is within 8 u (|mean| + |std eps|); a seed is a sum of two products of at most
four such factors: 16 u x the sum of the terms' magnitudes; a blocked gradient is exactly 0.  The estimator: ll rtol 1e-5 with atol
1e-5 x max_s |w_s| of the row; min over members exact given ll; the mask threshold sits in the middle of the widest gap between
neighbouring fp64 min-ll values around their median, and that gap must exceed ten times the tolerance there.

Every workspace mobody_bosa_workspace sizes is followed by NaN sentinel floats whose bits are checked after each call, and is itself
NaN-filled, so a read before the first write shows.  bosa_ref.LL_BOUNDARY_CASES / VAE_BOUNDARY_SHAPE cross the 256-row and
256-partial-sum boundaries of the row-wise kernels (tests/test_bosa_ref.py shows that they would catch a fault there).  A NaN
likelihood of one member makes the row's min_ll NaN and its mask 0, as torch.min and the comparison do in the reference.
"""
import numpy as np
import pytest
import torch

import bosa_ref as BR
import wide_ref as WR
from test_hip_train import params_close

pytestmark = pytest.mark.gpu
U = WR.U
NAN = float("nan")
GUARD, NAN_BITS = 64, 0x7FC00000

# name -> (S, A, hidden, members, batch rows): the fixture variants' shapes, and the reference's real width
SHAPES = {"small": (17, 6, 72, 2, 16), "odd": (17, 6, 72, 5, 66), "tiny": (3, 1, 8, 1, 4), "pen": (45, 24, 72, 2, 8),
          "real": (17, 6, 750, 5, 16)}
KINDS = ("policy", "dynamics")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


batch = BR.batch


def guarded_workspace(blk, dev):
    """(workspace, the whole buffer): mobody_bosa_workspace floats, NaN-filled, and GUARD NaN sentinel floats behind them."""
    from mobody_amd import ops
    n = ops.bosa_workspace(blk, dev).numel()
    buf = torch.full((n + GUARD,), NAN, device=dev)
    return buf[:n], buf


def guard_intact(buf):
    return bool((buf[-GUARD:].view(torch.int32) == NAN_BITS).all())


class Vae:
    """One VAE on the device: blob = encoder | decoder, gradient with a sentinel float behind it, Adam moments, workspace."""

    def __init__(self, kind, shape, dev, seed=21, beta=0.5, max_action=1.0, num_samples=0, **gen):
        from mobody_amd import ops, packing
        self.kind, self.dev, self.beta, self.ma = kind, dev, beta, max_action
        self.S, self.A, self.H, E, self.B = shape
        self.E = 1 if kind == "policy" else E
        self.enc, self.dec = BR.vae_params(seed, kind, self.S, self.A, self.H, self.E, **gen)
        self.blob = torch.cat([packing.pack_wide(*(p[k] for k in WR.KEYS), dev) for p in (self.enc, self.dec)])
        self.n_enc = packing.pack_wide(*(self.enc[k] for k in WR.KEYS), "cpu").numel()
        self.gbuf = torch.full((self.blob.numel() + 1,), NAN, device=dev)
        self.grad, self.m, self.v = self.gbuf[:-1], torch.zeros_like(self.blob), torch.zeros_like(self.blob)
        self.loss = torch.full((3,), NAN, device=dev)
        self.Lz = BR.dims(kind, self.S, self.A)[1]
        self.ns = num_samples
        self.ws, self.wsbuf = guarded_workspace(self.block(), dev)
        self.keep = []

    def block(self, **ff):
        from mobody_amd import ops
        return ops.bosa_block(self.kind, self.S, self.A, self.H, self.E, self.B, self.beta, self.ma, self.ns, blob=self.blob, **ff)

    def dev_batch(self, b):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(self.dev) for x in b]
        self.keep = t
        return dict(state=t[0], action=t[1], next_state=t[2])

    def step(self, b, eps, t=None, lr=0.0, **ff):
        from mobody_amd import ops
        opt = dict(m=self.m, v=self.v, t=t, lr=lr) if t is not None else {}
        e = torch.from_numpy(eps).to(self.dev) if eps is not None else None
        ops.bosa_vae(self.block(grad=self.grad, loss_out=self.loss, workspace=self.ws, eps=e, **self.dev_batch(b), **opt, **ff))
        torch.cuda.synchronize()
        assert torch.isnan(self.gbuf[-1])
        assert guard_intact(self.wsbuf), "mobody_bosa_vae wrote behind its workspace"
        return self.loss.cpu().numpy()

    def grads(self):
        from mobody_amd import packing
        ein, Lz, din, dout = BR.dims(self.kind, self.S, self.A)
        g = self.grad.cpu()
        return (dict(zip(WR.KEYS, (t.numpy() for t in packing.unpack_wide(g[:self.n_enc], ein, self.H, 2 * Lz, self.E)))),
                dict(zip(WR.KEYS, (t.numpy() for t in packing.unpack_wide(g[self.n_enc:], din, self.H, dout, self.E)))))

    def params(self):
        from mobody_amd import packing
        ein, Lz, din, dout = BR.dims(self.kind, self.S, self.A)
        p = self.blob.cpu()
        return (dict(zip(WR.KEYS, (t.numpy() for t in packing.unpack_wide(p[:self.n_enc], ein, self.H, 2 * Lz, self.E)))),
                dict(zip(WR.KEYS, (t.numpy() for t in packing.unpack_wide(p[self.n_enc:], din, self.H, dout, self.E)))))


def check_grads(got, want, tag):
    for net, g, w in zip(("enc", "dec"), got, want):
        for k in WR.KEYS:
            scale = np.abs(w[k]).max()
            print("%s %s.%s: worst error / tolerance %.3f" % (tag, net, k, (np.abs(g[k] - w[k]) / (1e-5 * scale + 1e-5 * np.abs(w[k]) + 1e-300)).max()))
            np.testing.assert_allclose(g[k], w[k], rtol=1e-5, atol=1e-5 * scale, err_msg="%s %s.%s" % (tag, net, k))


# ---- the row-wise kernel alone ------------------------------------------------------------------------------------------------
def test_reparam_kernel_at_the_clamp_edges(dev):
    from mobody_amd import ops
    f32 = np.float32
    edges = [f32(-4 - 1e-3), f32(-4 + 1e-3), f32(-4), f32(15 - 1e-3), f32(15 + 1e-3), f32(15), f32(-30), f32(0.3), f32(-2.5), f32(40)]
    assert edges[0] < -4 < edges[1] and edges[3] < 15 < edges[4]
    Lz, n = len(edges), 7
    rng = np.random.default_rng(0)
    mean = rng.standard_normal((n, Lz)).astype(f32) * f32(3)
    eps = rng.standard_normal((n, Lz)).astype(f32)
    eps[0], mean[1] = np.abs(eps[0]), -np.abs(mean[1])                              # mixed signs everywhere else
    pre = np.tile(np.array(edges, f32), (n, 1))
    dz = rng.standard_normal((n, Lz)).astype(f32)
    enc = np.concatenate([mean, pre], axis=1)
    beta = 0.5
    td = lambda x: torch.from_numpy(x).to(dev)
    z, kl, denc = ops.bosa_reparam(td(enc), td(eps), beta, dz=td(dz))
    z0, kl0, none = ops.bosa_reparam(td(enc), td(eps), beta)
    torch.cuda.synchronize()
    assert none is None and torch.equal(z, z0) and torch.equal(kl, kl0)
    zw, klw, dw = BR.reparam(enc, eps, beta, dz)
    std = np.exp(np.clip(pre.astype(np.float64), -4, 15))
    z, denc = z.cpu().numpy(), denc.cpu().numpy()
    assert (np.abs(z - zw) <= 8 * U * (np.abs(mean) + np.abs(std * eps))).all()
    np.testing.assert_allclose(kl.item(), klw, rtol=1e-5)
    N = n * Lz
    assert (np.abs(denc[:, :Lz] - dw[:, :Lz]) <= 16 * U * (np.abs(dz) + beta * np.abs(mean) / N)).all()
    blocked = np.array([e < -4 or e > 15 for e in edges])
    assert blocked.tolist() == [True, False, False, False, True, False, True, False, False, True]
    assert not denc[:, Lz:][:, blocked].view(np.int32).any(), "a value outside [-4, 15] passed gradient"
    open_ = ~blocked
    assert (denc[:, Lz:][:, open_] != 0).all() and (dw[:, Lz:][:, open_] != 0).all()      # -4 and 15 themselves pass
    bound = 16 * U * (np.abs(dz * eps * std) + beta * (std ** 2 + 1) / N)
    assert (np.abs(denc[:, Lz:] - dw[:, Lz:]) <= bound).all()


# ---- the VAE step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_vae_step_vs_fp64(dev, kind, name):
    """Losses and every gradient of one step; then three fused steps against the fp64 trajectory; explicit noise."""
    vae_step_vs_fp64(dev, kind, name, SHAPES[name], 1.0 if name != "pen" else 1.5)


def test_vae_step_vs_fp64_past_256_partial_sums(dev):
    """The dynamics VAE at 5 x 300 rows of the pen shape: 528 partial sums of the KL term and 264 of the reconstruction, so both of
    k_bosa_finish's 256-strided loops take a second trip, and every row-wise kernel runs hundreds of workgroups."""
    S, A, H, E, B = BR.VAE_BOUNDARY_SHAPE
    assert -(-E * B * 2 * S // 256) == 528 and -(-E * B * S // 256) == 264
    vae_step_vs_fp64(dev, "dynamics", "boundary", BR.VAE_BOUNDARY_SHAPE, 1.0, seed=BR.VAE_BOUNDARY_SEED)


def vae_step_vs_fp64(dev, kind, name, shape, ma, seed=21):
    S, A, H, E, B = shape
    v = Vae(kind, shape, dev, seed=seed, beta=0.5, max_action=ma)
    lr, rng = 1e-3, np.random.default_rng(4)
    enc64, dec64 = WR.f64(v.enc), WR.f64(v.dec)
    m64 = [{k: 0.0 for k in WR.KEYS} for _ in range(2)]
    v64 = [{k: 0.0 for k in WR.KEYS} for _ in range(2)]
    for t in (1, 2, 3):
        b = batch(100 + t, S, A, B)
        b = (b[0], (ma * b[1]).astype(np.float32), b[2])
        eps = rng.standard_normal((v.E, B, v.Lz)).astype(np.float32)
        losses, (genc, gdec), ex = BR.vae_step(enc64, dec64, kind, *b, eps, 0.5, ma)
        if t == 1:
            inside = (ex["pre"] >= -4) & (ex["pre"] <= 15)
            assert inside.any() and (ex["pre"] < -4).any(), "the weights do not reach both clamp branches"
            before = v.blob.clone()
            got = v.step(b, eps)                                                  # gradient form: nothing moves
            np.testing.assert_allclose(got, losses, rtol=1e-5)
            check_grads(v.grads(), (genc, gdec), "%s/%s" % (kind, name))
            assert torch.equal(before, v.blob) and not v.m.any() and not v.v.any()
        got = v.step(b, eps, t=t, lr=lr)
        np.testing.assert_allclose(got, losses, rtol=1e-5)
        for p, g, mm, vv in ((enc64, genc, m64[0], v64[0]), (dec64, gdec, m64[1], v64[1])):
            for k in WR.KEYS:
                p[k], mm[k], vv[k] = WR.adam(p[k], g[k], mm[k], vv[k], t, lr)
        for net, p_got, p_want in zip(("enc", "dec"), v.params(), (enc64, dec64)):
            for k in WR.KEYS:
                params_close(p_got[k], p_want[k], lr)
    from mobody_amd import packing
    ein, Lz, din, dout = BR.dims(kind, S, A)
    pad = torch.cat([packing.wide_padding_mask(ein, H, 2 * Lz, v.E, dev), packing.wide_padding_mask(din, H, dout, v.E, dev)])
    for tns in (v.blob, v.grad, v.m, v.v):
        assert not tns[pad].view(torch.int32).any(), "padding moved"


@pytest.mark.parametrize("kind", KINDS)
def test_vae_step_is_bit_identical_and_device_noise_matches_the_generator(dev, kind):
    from mobody_amd import _lib, ops
    shape = SHAPES["odd"]
    S, A, H, E, B = shape
    b = batch(7, S, A, B)
    a, c = Vae(kind, shape, dev), Vae(kind, shape, dev)
    seed, call = 1234, 5
    call_dev = torch.tensor([3], dtype=torch.int64, device=dev)
    la = a.step(b, None, seed=seed, call=call, call_dev=call_dev)
    lb = a.step(b, None, seed=seed, call=call, call_dev=call_dev)
    assert np.array_equal(la.view(np.int32), lb.view(np.int32))
    g1 = a.grad.clone()
    a.step(b, None, seed=seed, call=call, call_dev=call_dev)
    assert torch.equal(g1.view(torch.int32), a.grad.view(torch.int32))
    # the same step with the noise read back from the generator's stream at call + call_dev[0]
    eps = ops.rng_normal(seed, _lib.BOSA_STREAMS[kind], call + 3, a.E * B * a.Lz, dev).cpu().numpy().reshape(a.E, B, a.Lz)
    lc = c.step(b, eps)
    assert np.array_equal(la.view(np.int32), lc.view(np.int32)) and torch.equal(g1.view(torch.int32), c.grad.view(torch.int32))
    # the device step count: t_dev = 2 is the host's t = 2
    t_dev = torch.tensor([2], dtype=torch.int64, device=dev)
    a.step(b, eps, t=2, lr=1e-3)
    c.step(b, eps, t=0, lr=1e-3, t_dev=t_dev)
    for x, y in ((a.blob, c.blob), (a.m, c.m), (a.v, c.v)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- the estimator ------------------------------------------------------------------------------------------------------------
def run_ll(v, b, eps, n, log_eps=0.0, far_row=None):
    from mobody_amd import ops
    v.ns = n
    v.ws, v.wsbuf = guarded_workspace(v.block(), v.dev)
    new = lambda *s: torch.full(s, NAN, device=v.dev)
    out = dict(ll=new(v.E, v.B), w_out=new(v.E, n, v.B))
    if v.kind == "dynamics":
        out.update(min_ll=new(v.B), mask=new(v.B), mask_mean=new(1))
    e = torch.from_numpy(eps).to(v.dev) if eps is not None else None
    ops.bosa_loglik(v.block(workspace=v.ws, eps=e, log_eps=float(log_eps), **v.dev_batch(b), **out))
    torch.cuda.synchronize()
    assert guard_intact(v.wsbuf), "mobody_bosa_loglik wrote behind its workspace"
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,n", [("small", 1), ("small", 4), ("odd", 4), ("tiny", 64), ("pen", 4), ("real", 1), ("odd", 64)] +
                         [(k, c[1]) for k, c in BR.LL_BOUNDARY_CASES.items()])
def test_estimator_vs_fp64(dev, kind, name, n):
    shape = SHAPES[name] if name in SHAPES else BR.LL_BOUNDARY_CASES[name][0]
    S, A, H, E, B = shape
    v = Vae(kind, shape, dev, beta=0.5, max_action=1.0)
    # `far`: one row whose w all lie below -1e4, the target far from any decoding
    s, a, s2, eps, far = BR.estimator_case(kind, S, A, v.E, B, n)
    ll64, w64 = BR.loglik(v.enc, v.dec, kind, s, a, s2, eps, 0.5, 1.0)
    got = run_ll(v, (s, a, s2), eps, n)                     # every output pre-filled with NaN
    assert (w64[:, :, far] < -1e4).all() and np.isfinite(got["ll"]).all()
    for k, t in got.items():
        assert np.isfinite(t).all(), "%s: %d entries left unwritten or not finite" % (k, (~np.isfinite(t)).sum())
    tol = BR.estimator_tolerance(ll64, w64)
    print("ll: worst error / tolerance %.3f" % (np.abs(got["ll"] - ll64) / tol).max())
    assert (np.abs(got["ll"] - ll64) <= tol).all()
    assert (np.abs(got["w_out"] - w64) <= 1e-5 * np.abs(w64) + 1e-5 * np.abs(w64).max(1, keepdims=True)).all()
    if kind == "policy":
        return
    assert np.array_equal(got["min_ll"], got["ll"].min(0)), "min over members is not exact"
    # threshold in the widest gap between neighbouring fp64 minima around the median
    thr, gap, row_tol = BR.mask_threshold(ll64, tol)            # row_tol: of the two rows on either side of the gap
    assert gap > 10 * row_tol, "no usable gap for the mask threshold"
    got = run_ll(v, (s, a, s2), eps, n, log_eps=thr)
    want = (ll64.min(0) > thr).astype(np.float32)
    assert 0 < want.sum() < B and np.array_equal(got["mask"], want)
    assert np.array_equal(got["min_ll"], got["ll"].min(0)) and np.isfinite(got["mask_mean"]).all()
    assert got["mask_mean"][0] == np.float32(want.sum() / np.float32(B))


@pytest.mark.parametrize("members", [2, 1])
def test_nan_member_poisons_min_ll_and_masks_the_row(dev, members):
    """torch.min propagates NaN and NaN > log(eps) is False (bosa.py:585-590), so a row on which one member's likelihood is NaN
    has min_ll = NaN and mask = 0 in the reference; fminf would drop the NaN and let the row through on the other members (with one
    member: min_ll = +Inf, mask = 1).  NaN noise of one latent column makes that member's ll NaN on three rows; every other
    entry keeps the bits of the clean run.  Against the kernel before the flag in k_bosa_ll_reduce this test failed (min_ll
    finite or +Inf and mask 1 on the planted rows, mask_mean 1)."""
    S, A, H, _, B = SHAPES["small"]
    n, m = 4, members - 1                                    # the planted member: 1 of 2, or the only one
    v = Vae("dynamics", (S, A, H, members, B), dev, beta=0.5, max_action=1.0)
    b = batch(9, S, A, B)
    clean = np.random.default_rng(1).standard_normal((n, members, B, v.Lz)).astype(np.float32)
    rows = [0, 5, B - 1]
    bad = np.zeros(B, bool)
    bad[rows] = True
    eps = clean.copy()
    eps[:, m, rows, 3] = np.nan
    log_eps = -1e30                                          # every finite row passes
    ref = run_ll(v, b, clean, n, log_eps=log_eps)
    got = run_ll(v, b, eps, n, log_eps=log_eps)
    assert np.isfinite(ref["ll"]).all() and (ref["mask"] == 1).all() and ref["mask_mean"][0] == 1
    # what the restatement's semantics give on the planted rows (NumPy's min propagates NaN as torch's does)
    with np.errstate(invalid="ignore"):
        ll64 = BR.loglik(v.enc, v.dec, "dynamics", *b, eps, 0.5, 1.0)[0]
        assert np.isnan(ll64[m, bad]).all() and np.isnan(ll64.min(0)[bad]).all() and not (ll64.min(0)[bad] > log_eps).any()
    assert np.isnan(got["ll"][m, bad]).all(), got["ll"][m, bad]
    assert np.isnan(got["min_ll"][bad]).all(), got["min_ll"][bad]
    assert (got["mask"][bad] == 0).all(), got["mask"][bad]
    # everything else: the clean run's bits
    touched = np.zeros((members, B), bool)
    touched[m, bad] = True
    i32 = lambda x: np.ascontiguousarray(x).view(np.int32)
    assert np.array_equal(i32(got["ll"][~touched]), i32(ref["ll"][~touched]))
    assert np.array_equal(i32(got["min_ll"][~bad]), i32(ref["min_ll"][~bad])) and np.array_equal(i32(got["mask"][~bad]), i32(ref["mask"][~bad]))
    assert (got["mask"][~bad] == 1).all() and got["mask_mean"][0] == np.float32(B - 3) / np.float32(B)


def test_estimator_device_noise_and_refusals(dev):
    from mobody_amd import _lib, ops
    shape = SHAPES["small"]
    S, A, H, E, B = shape
    b = batch(3, S, A, B)
    for kind in KINDS:
        v = Vae(kind, shape, dev)
        n = 4
        v.ns = n
        drawn = run_ll(v, b, None, n)
        flat = ops.rng_normal(0, _lib.BOSA_STREAMS[kind + "_ll"], 0, v.E * B * n * v.Lz, dev).cpu().numpy()
        eps = flat.reshape((B, n, v.Lz) if kind == "policy" else (n, v.E, B, v.Lz))
        given = run_ll(v, b, eps, n)
        assert np.array_equal(drawn["ll"].view(np.int32), given["ll"].view(np.int32))
        for bad in (0, 65):
            v.ns = bad
            with pytest.raises(_lib.MobodyError, match="num_samples|bad block"):
                run_ll(v, b, None, bad)
        v.ns = n
        with pytest.raises(_lib.MobodyError, match="exact fp32"):
            ops.bosa_loglik(v.block(precision=4, workspace=v.ws, ll=torch.empty(v.E, B, device=dev), **v.dev_batch(b)))
        with pytest.raises(_lib.MobodyError, match="exact fp32"):
            ops.bosa_vae(v.block(precision=1, workspace=v.ws, grad=v.grad, loss_out=v.loss, **v.dev_batch(b)))


# ---- against the fixtures of the real reference (tests/golden/make_golden_bosa.py) ----------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tag", list(BR.VARIANTS))
def test_vae_step_and_estimator_vs_reference_fixture(dev, kind, tag):
    from test_bosa_ref import check_fixture_grads, load_fixture, sub
    g, nets, mixed, _ = load_fixture(tag)
    S, A, H, E, bs = BR.VARIANTS[tag]
    lr = float(g["lr"])
    seed = int(g["seed"]) + (50 if kind == "dynamics" else 0)
    v = Vae(kind, (S, A, H, E, 2 * bs), dev, seed=seed, beta=0.5, log_std_bias=float(g["log_std_bias"]), log_std_scale=float(g["log_std_scale"]))
    for n in (1, 4):                                              # the estimators, on the initial weights
        got = run_ll(v, mixed, g["ll%d_%s_eps" % (n, kind)], n)
        ll64, w64 = BR.loglik(v.enc, v.dec, kind, *mixed, g["ll%d_%s_eps" % (n, kind)], 0.5)
        tol = 1e-5 * np.abs(ll64) + 1e-5 * np.abs(w64).max(1)
        assert (np.abs(got["ll"] - g["ll%d_%s" % (n, kind)]) <= tol).all() and (np.abs(got["ll"] - ll64) <= tol).all()
    for call in (1, 2, 3):
        eps = g["t%d_%s_eps" % (call, kind)]
        if call == 1:
            np.testing.assert_allclose(v.step(mixed, eps), g["t1_%s_loss" % kind], rtol=1e-5)      # gradient form
            check_fixture_grads(g, 1, kind, v.grads())
        np.testing.assert_allclose(v.step(mixed, eps, t=call, lr=lr), g["t%d_%s_loss" % (call, kind)], rtol=1e-5)
        check_fixture_grads(g, call, kind, v.grads())
        for name, got in BR.state_dict(*v.params(), kind).items():
            params_close(sub(got), g["t%d_%s_p::%s" % (call, kind, name)], lr)
