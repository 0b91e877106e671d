"""CPU checks of the fp64 restatement tests/bosa_ref.py itself (finite differences, the estimator's algebra), of the shapes the GPU
tests use (both clamp branches are reached), and of the BOSA entry points' declarations and refusals (no GPU work is launched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bosa_ref as BR
import wide_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000
SHAPES = {"small": (17, 6, 72, 2, 16), "odd": (17, 6, 72, 5, 66), "tiny": (3, 1, 8, 1, 4), "pen": (45, 24, 72, 2, 8)}


def _batch(seed, S, A, B):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(B, S), np.tanh(f(B, A)), f(B, S)


@pytest.mark.parametrize("kind", ("policy", "dynamics"))
def test_vae_step_gradients_match_finite_differences(kind):
    S, A, H, E, B = 3, 2, 8, 2, 5
    enc, dec = (WR.f64(p) for p in BR.vae_params(5, kind, S, A, H, E, log_std_bias=-3.5))
    E = enc["W1"].shape[0]
    s, a, s2 = _batch(1, S, A, B)
    Lz = BR.dims(kind, S, A)[1]
    eps = np.random.default_rng(2).standard_normal((E, B, Lz))
    beta, ma = 0.7, 1.3
    loss = lambda e, d: BR.vae_step(e, d, kind, s, a, s2, eps, beta, ma)[0][2]
    (rec, kl, tot), (genc, gdec), ex = BR.vae_step(enc, dec, kind, s, a, s2, eps, beta, ma)
    assert tot == rec + beta * kl and (ex["pre"] < -4).any() and (ex["pre"] > -4).any()
    rng, h = np.random.default_rng(3), 1e-6
    for which, g in ((0, genc), (1, gdec)):
        for k in WR.KEYS:
            for idx in [tuple(rng.integers(0, n) for n in g[k].shape) for _ in range(5)]:
                nets_hi, nets_lo = [{kk: v.copy() for kk, v in p.items()} for p in (enc, dec)], [{kk: v.copy() for kk, v in p.items()} for p in (enc, dec)]
                nets_hi[which][k][idx] += h
                nets_lo[which][k][idx] -= h
                fd = (loss(*nets_hi) - loss(*nets_lo)) / (2 * h)
                assert abs(fd - g[k][idx]) < 2e-6 * max(1.0, abs(g[k][idx])), (which, k, idx, fd, g[k][idx])


def test_reparam_matches_vae_step_and_blocks_outside_the_clamp():
    enc = np.array([[0.5, -1.0, -4.0, 15.0], [0.2, 0.3, -4.001, 15.001]])
    eps, dz = np.array([[1.0, -2.0], [0.5, 0.25]]), np.array([[0.1, 0.2], [0.3, 0.4]])
    z, kl, d = BR.reparam(enc, eps, 0.5, dz)
    assert z[0, 0] == 0.5 + np.exp(-4.0) and z[0, 1] == -1.0 - 2.0 * np.exp(15.0)
    assert (d[0, 2:] != 0).all() and (d[1, 2:] == 0).all()                        # -4 and 15 pass, beyond them nothing does
    std = np.exp(np.clip(enc[:, 2:], -4, 15))
    assert np.isclose(kl, -0.5 * (1 + 2 * np.clip(enc[:, 2:], -4, 15) - enc[:, :2] ** 2 - std ** 2).mean())


@pytest.mark.parametrize("kind", ("policy", "dynamics"))
@pytest.mark.parametrize("name", list(SHAPES))
def test_gpu_test_shapes_reach_both_clamp_branches(kind, name):
    S, A, H, E, B = SHAPES[name]
    enc, dec = BR.vae_params(21, kind, S, A, H, E)
    b = _batch(101, S, A, B)
    pre = BR.encode(enc, kind, *b)[1]
    assert (pre < -4).any() and ((pre >= -4) & (pre <= 15)).any()
    # no value within fp32 rounding of a clamp end, where the kernel's gate and the restatement's could differ
    assert (np.abs(pre + 4) > 1e-5).all() and (np.abs(pre - 15) > 1e-5).all()


@pytest.mark.parametrize("kind", ("policy", "dynamics"))
def test_estimator_algebra(kind):
    """n = 1: ll = w.  Repeating one noise draw n times leaves ll unchanged (logsumexp of n equal terms - log n)."""
    S, A, H, E, B = SHAPES["small"]
    enc, dec = BR.vae_params(21, kind, S, A, H, E)
    E = enc["W1"].shape[0]
    s, a, s2 = _batch(9, S, A, B)
    Lz = BR.dims(kind, S, A)[1]
    rng = np.random.default_rng(0)
    one = rng.standard_normal((B, 1, Lz) if kind == "policy" else (1, E, B, Lz))
    ll1, w1 = BR.loglik(enc, dec, kind, s, a, s2, one, 0.5)
    assert ll1.shape == (E, B) and np.allclose(ll1, w1[:, 0])
    rep = np.repeat(one, 4, axis=1 if kind == "policy" else 0)
    ll4, w4 = BR.loglik(enc, dec, kind, s, a, s2, rep, 0.5)
    assert w4.shape == (E, 4, B) and np.allclose(ll4, ll1, rtol=1e-12)
    # against the definition, one row
    mean, pre, std, _, _, _ = BR.encode(enc, kind, s, a, s2)
    z = mean[0, 2] + std[0, 2] * (one[2, 0] if kind == "policy" else one[0, 0, 2])
    xd = np.concatenate([s[2], z] if kind == "policy" else [s[2], a[2], z])[None, None]
    d0 = {k: np.asarray(v, np.float64)[:1] for k, v in dec.items()}
    u = WR.forward(d0, xd, "tanh" if kind == "policy" else "raw")[0][0, 0]
    x = (a if kind == "policy" else s2)[2]
    ln = lambda v, m, sd: (-0.5 * ((v - m) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2 * np.pi)).sum()
    assert np.isclose(w1[0, 0, 2], ln(x, u, np.sqrt(0.125)) + ln(z, 0.0, 1.0) - ln(z, mean[0, 2], std[0, 2]), rtol=1e-12)


# ---- the shapes that cross workgroup boundaries (tests/test_hip_bosa.py): what the GPU cases can and would catch -------------------
@pytest.mark.parametrize("name", list(BR.LL_BOUNDARY_CASES))
def test_mask_threshold_has_a_usable_gap_at_the_boundary_shapes(name):
    """The GPU test's precondition, from the restatement alone: next to the median of the fp64 minima there is a gap of more than
    ten tolerances, and the threshold in its middle splits the rows -- so a change of seeds cannot turn the mask check vacuous."""
    (S, A, H, E, B), n = BR.LL_BOUNDARY_CASES[name]
    assert B > 256 and B % 256 != 0
    enc, dec = BR.vae_params(21, "dynamics", S, A, H, E)
    s, a, s2, eps, far = BR.estimator_case("dynamics", S, A, E, B, n)
    ll64, w64 = BR.loglik(enc, dec, "dynamics", s, a, s2, eps, 0.5, 1.0)
    assert (w64[:, :, far] < -1e4).all() and np.isfinite(ll64).all()
    thr, gap, row_tol = BR.mask_threshold(ll64, BR.estimator_tolerance(ll64, w64))
    print("%s: gap %.3f / ten tolerances %.4f" % (name, gap, 10 * row_tol))
    assert gap > 10 * row_tol
    want = ll64.min(0) > thr
    assert 0 < want.sum() < B and not want[far]
    if B > 257:                                                                   # rows of the later workgroups on both sides
        assert want[256:].any() and not want[256:].all()


def test_unwritten_rows_past_one_workgroup_fail_the_finiteness_check():
    """An estimator that leaves rows 256.. of its NaN-prefilled outputs alone (one workgroup's worth written) is caught."""
    (S, A, H, E, B), n = BR.LL_BOUNDARY_CASES["odd-b300"]
    enc, dec = BR.vae_params(21, "dynamics", S, A, H, E)
    s, a, s2, eps, far = BR.estimator_case("dynamics", S, A, E, B, n)
    ll64 = BR.loglik(enc, dec, "dynamics", s, a, s2, eps, 0.5, 1.0)[0]
    got = np.full((E, B), np.nan, np.float32)
    got[:, :256] = ll64[:, :256]
    assert np.isfinite(got[:, :256]).all() and not np.isfinite(got).all()
    mask = np.full(B, np.nan, np.float32)                                         # ... and a mask mean over 256 rows only is not B's
    mask[:256] = 1.0
    assert mask[:256].sum() / B != 1.0 and not np.isfinite(mask).all()


def test_a_loss_from_the_first_256_partial_sums_misses_the_tolerance():
    """k_bosa_finish adds the per-workgroup partial sums (256 elements each) in 256-strided loops.  At the boundary shape the KL
    term has 528 partial sums and the reconstruction 264: a loss from the first 256 alone is off by far more than rtol 1e-5."""
    S, A, H, E, B = BR.VAE_BOUNDARY_SHAPE
    enc, dec = (WR.f64(p) for p in BR.vae_params(BR.VAE_BOUNDARY_SEED, "dynamics", S, A, H, E))
    s, a, s2 = BR.batch(101, S, A, B)
    eps = np.random.default_rng(4).standard_normal((E, B, 2 * S)).astype(np.float32)
    (rec, kl, tot), _, ex = BR.vae_step(enc, dec, "dynamics", s, a, s2, eps, 0.5, 1.0)
    kl_terms = (1.0 + np.log(ex["std"] ** 2) - ex["mean"] ** 2 - ex["std"] ** 2).reshape(-1)           # element (e B + b) Lz + l
    rec_terms = ((ex["u"] - np.asarray(s2, np.float64)[None]) ** 2).reshape(-1)                          # element (e B + b) D + d
    partial = lambda t: np.add.reduceat(t, np.arange(0, t.size, 256))
    pk, pr = partial(kl_terms), partial(rec_terms)
    assert (pk.size, pr.size) == (528, 264) and kl_terms.size == 135000 and rec_terms.size == 67500
    assert np.isclose(-0.5 * pk.sum() / kl_terms.size, kl, rtol=1e-12) and np.isclose(pr.sum() / rec_terms.size, rec, rtol=1e-12)
    kl_cut, rec_cut = -0.5 * pk[:256].sum() / kl_terms.size, pr[:256].sum() / rec_terms.size
    for cut, full in ((kl_cut, kl), (rec_cut, rec), (rec_cut + 0.5 * kl, tot), (rec + 0.5 * kl_cut, tot)):
        assert abs(cut - full) > 100 * 1e-5 * abs(full)
    # both clamp branches at this shape, in comparable shares, and nothing within fp32 rounding of a clamp end
    pre = ex["pre"]
    inside, below = ((pre >= -4) & (pre <= 15)).mean(), (pre < -4).mean()
    assert inside > 0.25 and below > 0.25 and (np.abs(pre + 4) > 1e-5).all() and (np.abs(pre - 15) > 1e-5).all()


def test_a_nan_member_poisons_the_minimum_and_masks_the_row():
    """The reference's rule (torch.min propagates NaN, NaN > log(eps) is False; NumPy's min and comparison do the same): a row on
    which one member's likelihood is NaN has min_ll = NaN and mask = 0, whatever the other members give."""
    S, A, H, E, B = SHAPES["small"]
    enc, dec = BR.vae_params(21, "dynamics", S, A, H, E)
    s, a, s2 = BR.batch(9, S, A, B)
    eps = np.random.default_rng(1).standard_normal((4, E, B, 2 * S)).astype(np.float32)
    eps[:, 1, [0, 5, B - 1], 3] = np.nan
    with np.errstate(invalid="ignore"):
        ll = BR.loglik(enc, dec, "dynamics", s, a, s2, eps, 0.5, 1.0)[0]
        lo = ll.min(0)
        mask = lo > -1e30
    bad = np.zeros(B, bool)
    bad[[0, 5, B - 1]] = True
    assert np.isnan(ll[1, bad]).all() and np.isfinite(ll[0]).all() and np.isfinite(ll[1, ~bad]).all()
    assert np.isnan(lo[bad]).all() and not mask[bad].any() and mask[~bad].all() and mask.mean() == (B - 3) / B


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_bosa_symbols_declared_bound_and_exported(lib):
    from mobody_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    for e in ("mobody_bosa_reparam", "mobody_bosa_vae", "mobody_bosa_loglik"):
        assert re.search(r"%s\s+bosa\.py:\d+" % e, hdr), e                       # each entry cites the reference lines it replaces
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for e in ("mobody_bosa_vae", "mobody_bosa_loglik"):
        assert re.search(r"\bint %s\(const MobodyBosaVae\* a, void\* stream\);" % e, hdr)
        res, args = _lib.PROTOTYPES[e]
        assert res is C.c_int and args[0] is C.POINTER(_lib.MobodyBosaVae) and args[1] is _lib.vp and hasattr(lib, e)
    decl = re.search(r"\bstruct MobodyBosaVae \{(.*?)\};", hdr, flags=re.S).group(1)
    names = [n.strip(" *") for stmt in decl.split(";") if stmt.strip() for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]
    assert names == [f for f, _ in _lib.MobodyBosaVae._fields_]
    assert C.sizeof(_lib.MobodyBosaVae) == _lib.BLOCK_BYTES[_lib.MobodyBosaVae]
    for k, v in _lib.BOSA_STREAMS.items():
        assert re.search(r"MOBODY_BOSA_STREAM_%s = %d\b" % (k.upper(), v), hdr), k
    assert min(_lib.BOSA_STREAMS.values()) > 5                                     # streams 1-5 are taken
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7
    for f in ("bosa_block", "bosa_workspace", "bosa_reparam", "bosa_vae", "bosa_loglik"):
        assert callable(getattr(ops, f)), f


def _refused(lib, entry, blk, *words):
    assert getattr(lib, entry)(C.byref(blk), None) == -1, entry
    msg = lib.mobody_last_error().decode()
    assert msg.startswith((entry + ":", "mobody_wide_layout:")), msg
    for w in words:
        assert w in msg, (w, msg)


def test_bosa_refusals_come_before_any_runtime_call(lib):
    from mobody_amd import _lib
    ok = dict(kind=1, S=17, A=6, hidden=72, members=2, B=8, beta=0.5, max_action=1.0, blob=PTR, state=PTR, action=PTR, next_state=PTR,
              workspace=PTR)
    vae = dict(grad=PTR, loss_out=PTR, **ok)
    for entry in ("mobody_bosa_vae", "mobody_bosa_loglik"):
        cls = _lib.MobodyBosaVae
        _refused(lib, entry, cls(struct_bytes=C.sizeof(cls) - 1), "struct_bytes")
        _refused(lib, entry, _lib.block(cls, **{**vae, "kind": 2}), "kind 2")
        _refused(lib, entry, _lib.block(cls, **{**vae, "kind": 0}), "the policy VAE has one member")
        _refused(lib, entry, _lib.block(cls, **{**vae, "hidden": 1025}), "hidden 1025")
        _refused(lib, entry, _lib.block(cls, **{**vae, "S": 65}), "out_dim 260")
        _refused(lib, entry, _lib.block(cls, **{**vae, "members": 9}), "members 9")
        _refused(lib, entry, _lib.block(cls, precision=4, **vae), "precision 4", "exact fp32")
        _refused(lib, entry, _lib.block(cls, **{**vae, "B": 0}), "B 0")
        _refused(lib, entry, _lib.block(cls, **{**vae, "beta": 0.0}), "beta 0")
    _refused(lib, "mobody_bosa_vae", _lib.block(_lib.MobodyBosaVae, m=PTR, **vae), "one of m, v without the other")
    _refused(lib, "mobody_bosa_vae", _lib.block(_lib.MobodyBosaVae, m=PTR, v=PTR, **vae), "step t must be >= 1")
    _refused(lib, "mobody_bosa_vae", _lib.block(_lib.MobodyBosaVae, **{**vae, "grad": None}), "null pointer")
    ll = dict(ll=PTR, **ok)
    for n in (0, 65, -1):
        _refused(lib, "mobody_bosa_loglik", _lib.block(_lib.MobodyBosaVae, num_samples=n, **ll), "num_samples %d outside [1, 64]" % n)
    _refused(lib, "mobody_bosa_loglik", _lib.block(_lib.MobodyBosaVae, num_samples=4, grad=PTR, **ll), "forward only")
    _refused(lib, "mobody_bosa_loglik", _lib.block(_lib.MobodyBosaVae, num_samples=4, mask_mean=PTR, **ll), "mask_mean needs mask")
    _refused(lib, "mobody_bosa_loglik", _lib.block(_lib.MobodyBosaVae, num_samples=4, **{**ok}), "null pointer")
    blk = _lib.block(_lib.MobodyBosaVae, num_samples=4, **ok)
    w4 = lib.mobody_bosa_workspace(C.byref(blk))
    blk.num_samples = 8
    assert 0 < w4 < lib.mobody_bosa_workspace(C.byref(blk))
    blk.num_samples = 65
    assert lib.mobody_bosa_workspace(C.byref(blk)) == -1


# ---- the class: registry, constructor order, the counting (no GPU) -------------------------------------------------------------
def bosa_config(**over):
    """The reference's config/mujoco/bosa/walker2d.yaml keys at a small width."""
    c = dict(vae_policy_lr=1e-3, vae_policy_hidden_dim=72, vae_policy_beta=0.5, vae_dyna_lr=1e-3, vae_dyna_ensemble=2, vae_dyna_hidden_dim=72,
             vae_dyna_beta=0.5, vae_iteration=7, lamda_policy=0.25, lamda_dyna=1.0, epsilon_policy_exp=0.01, epsilon_dyna_exp=0.01,
             conservation_coef=0.1, num_samples=4, noise_clip=0.5, expl_noise=0.1, update_interval=2, actor_lr=3e-4, critic_lr=3e-4, gamma=0.99,
             tau=0.005, policy_noise=0.2, policy_freq=2, batch_size=8, state_dim=17, action_dim=6, max_action=1.0)
    c.update(over)
    return c


def test_vae_steps_and_the_total_it_sequence():
    from mobody_amd.algo.offline_offline.bosa import vae_steps
    assert [vae_steps(v) for v in (0, 1, 2, 3, 7, 8, 100000, -5)] == [0, 0, 1, 1, 3, 4, 50000, 0]
    for V in range(0, 12):                      # the reference's counting, replayed: calls until total_it + 1 < V fails
        total_it, calls = 0, 0
        while True:
            total_it += 1
            if not total_it < V:
                break
            total_it += 1
            calls += 1
            assert total_it == 2 * calls
        assert calls == vae_steps(V), V


def test_registry_and_constructor_order():
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline import bosa
    from mobody_amd.engine import default_config
    assert len(bosa._KEYS) == 17
    for k in bosa._KEYS:                                                  # every missing key is named
        c = bosa_config()
        del c[k]
        with pytest.raises(NotImplementedError, match=r"config lacks \['%s'\]" % k):
            call_algo("bosa", c, 3, "cpu")
    with pytest.raises(NotImplementedError, match="BOSA config only"):     # another algorithm's config
        call_algo("BOSA", default_config(17, 6), 3, "cpu")
    c = bosa_config(vae_policy_hidden_dim=2000)
    del c["num_samples"]
    with pytest.raises(NotImplementedError, match="num_samples"):          # missing comes before range
        call_algo("bosa", c, 3, "cpu")
    for key, bad in (("vae_policy_hidden_dim", 7), ("vae_dyna_hidden_dim", 1025), ("vae_dyna_ensemble", 0), ("vae_dyna_ensemble", 9),
                     ("num_samples", 0), ("num_samples", 65), ("vae_policy_beta", 0.0), ("vae_dyna_beta", -1.0), ("epsilon_policy_exp", 0.0),
                     ("epsilon_dyna_exp", 0.0), ("vae_iteration", -1)):
        with pytest.raises(ValueError, match=key):                         # range comes before device
            call_algo("bosa", bosa_config(**{key: bad}), 3, "cpu")
    with pytest.raises(RuntimeError, match="needs a GPU device"):          # a full config on 'cpu'
        call_algo("bosa", bosa_config(), 3, "cpu")


def test_two_rank_world_is_refused_before_the_device_check(monkeypatch):
    import torch
    from mobody_amd.algo.call_algo import call_algo
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="data-parallel BOSA is not built"):
        call_algo("bosa", bosa_config(), 3, "cpu")
    with pytest.raises(ValueError, match="num_samples"):                   # ... and after the range check
        call_algo("bosa", bosa_config(num_samples=99), 3, "cpu")


# ---- the restatement against the fixtures of the real reference (tests/golden/make_golden_bosa.py) ------------------------------
def sub(x):
    f = np.asarray(x).reshape(-1)
    return f[::13].copy() if f.size > 4096 else f.copy()


def load_fixture(tag):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g27_bosa_%s.npz" % tag))
    S, A, H, E, bs = (int(g[k]) for k in ("S", "A", "hidden", "E", "bs"))
    assert (S, A, H, E, bs) == BR.VARIANTS[tag]
    setting = (float(g["log_std_bias"]), float(g["log_std_scale"]))
    nets = {"policy": BR.vae_params(int(g["seed"]), "policy", S, A, H, 1, *setting),
            "dynamics": BR.vae_params(int(g["seed"]) + 50, "dynamics", S, A, H, E, *setting)}
    import gen_inputs as gi
    for k in nets:
        assert gi.checksum(BR.state_dict(*nets[k], k)) == float(g["wsum_" + k]), k
    rows_src, rows_tar = gi.batch(501, 64, S, A), gi.batch(502, 64, S, A)
    mixed = tuple(np.concatenate([t[:bs], s[:bs]]) for s, t in zip(rows_src, rows_tar))[:3]
    return g, nets, mixed, (rows_src, rows_tar)


def check_fixture_grads(g, call, kind, grads, rtol=1e-5):
    """Thinned gradient entries at rtol / atol x the tensor's largest entry, and the fp64 [sum, sum of squares] of the whole tensor."""
    sd = BR.state_dict(*grads, kind)
    for name, got in sd.items():
        want, scale = g["t%d_%s_g::%s" % (call, kind, name)], np.abs(got).max()
        np.testing.assert_allclose(sub(got), want, rtol=rtol, atol=rtol * scale, err_msg=name)
        s1, s2 = g["t%d_%s_gsum::%s" % (call, kind, name)]
        assert abs(got.astype(np.float64).sum() - s1) <= 4 * rtol * scale * np.sqrt(got.size) + rtol * abs(s1), name
        np.testing.assert_allclose((got.astype(np.float64) ** 2).sum(), s2, rtol=4 * rtol, err_msg=name)


@pytest.mark.parametrize("tag", list(BR.VARIANTS))
def test_restatement_vs_reference_fixture(tag):
    g, nets, mixed, _ = load_fixture(tag)
    lr = float(g["lr"])
    assert float(g["restate_grad"]) <= 1.0 and float(g["restate_param"]) <= 0.05 and float(g["restate_ll"]) <= 1.0 and float(g["clamp_margin"]) > 1e-3
    for kind in ("policy", "dynamics"):
        for n in (1, 4):
            ll64, w64 = BR.loglik(*nets[kind], kind, *mixed, g["ll%d_%s_eps" % (n, kind)], 0.5)
            tol = 1e-5 * np.abs(ll64) + 1e-5 * np.abs(w64).max(1)
            assert (np.abs(g["ll%d_%s" % (n, kind)] - ll64) <= tol).all(), (kind, n)
        p = [WR.f64(nets[kind][0]), WR.f64(nets[kind][1])]
        m = [{q: 0.0 for q in WR.KEYS} for _ in range(2)]
        v = [{q: 0.0 for q in WR.KEYS} for _ in range(2)]
        for call in (1, 2, 3):
            losses, grads, ex = BR.vae_step(*p, kind, *mixed, g["t%d_%s_eps" % (call, kind)], 0.5, 1.0)
            np.testing.assert_allclose(losses, g["t%d_%s_loss" % (call, kind)], rtol=1e-5)
            assert (ex["pre"] < -4).any() and ((ex["pre"] >= -4) & (ex["pre"] <= 15)).any()
            check_fixture_grads(g, call, kind, grads)
            for net in (0, 1):
                for q in WR.KEYS:
                    p[net][q], m[net][q], v[net][q] = WR.adam(p[net][q], grads[net][q], m[net][q], v[net][q], call, lr)
            for name, got in BR.state_dict(*p, kind).items():
                assert np.abs(sub(got) - g["t%d_%s_p::%s" % (call, kind, name)]).max() <= 0.05 * lr, (call, name)


def test_total_it_sequence_of_the_reference():
    from mobody_amd.algo.offline_offline.bosa import vae_steps
    for tag in BR.VARIANTS:
        g = np.load(os.path.join(ROOT, "tests", "golden", "g27_bosa_%s.npz" % tag))
        assert g["total_it_seq"].tolist() == [2, 4, 6, 7] and bool(g["moved_on"])       # vae_iteration = 7: call 4 left the VAE stage
    assert vae_steps(7) == 3


def test_reference_checkpoint_round_trips_through_packing():
    """The reference's own state_dicts at the tiny shape: keys, shapes and values survive pack -> unpack."""
    import torch
    from mobody_amd import packing
    S, A, H, E, _ = BR.VARIANTS["tiny"]
    d = os.path.join(ROOT, "tests", "golden", "ckpt_bosa_ref")
    sp = torch.load(os.path.join(d, "model_vae_policy"), map_location="cpu", weights_only=True)
    sdyn = torch.load(os.path.join(d, "model_vae_dynamics"), map_location="cpu", weights_only=True)
    assert list(sp) == [k + s for k in BR.NET_KEYS for s in (".weight", ".bias")]
    assert list(sdyn) == [k + s for k in BR.NET_KEYS for s in (".W", ".b")]
    assert sp["mean.weight"].shape == (2 * A, H) and sdyn["log_std.W"].shape == (E, H, 2 * S) and sdyn["decoder.4.b"].shape == (E, 1, S)
    back = packing.unpack_bosa_vae_policy(*packing.pack_bosa_vae_policy(sp, "cpu"), S, A, H)
    assert list(back) == list(sp) and all(torch.equal(back[k], sp[k]) for k in sp)
    back = packing.unpack_bosa_vae_dynamics(*packing.pack_bosa_vae_dynamics(sdyn, "cpu"), S, A, H, E)
    assert list(back) == list(sdyn) and all(torch.equal(back[k], sdyn[k]) for k in sdyn)
    # EnsembleFC's initialisation (bosa.py:188-196): fmod(randn, 2) weights, zero biases
    assert float(sdyn["encoder_shared.0.W"].abs().max()) < 2.0 and not sdyn["mean.b"].any()
