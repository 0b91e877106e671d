"""CPU checks of tests/bosa2_ref.py, the fp64 restatement of BOSA's critic / actor stage: the estimator's gradient with
respect to the action, the critic's and the actor's gradients against central finite differences of their losses; a float32
evaluation of the critic step within half of the GPU test's tolerance (the project's precondition for a normalised tolerance); the
composed stage-2 call against the g28 fixtures of the real reference; the
new entry point's declaration and refusals (nothing is launched: the refusals come first); the ABI stays 7; the class's config
check is what it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bosa2_ref as B2
import bosa_ref as BR
import wide_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000


@pytest.mark.parametrize("n", (1, 4))
@pytest.mark.parametrize("tag", ("tiny", "small"))
@pytest.mark.parametrize("ma", (1.0, 2.0))
def test_loglik_grad_action_matches_finite_differences(tag, n, ma):
    """Every entry of dll_da on the fixture variant's mixed batch, eps fixed.  Bound: the central difference at h = 1e-6 carries
    rounding 2^-52 |ll| / h < 3e-10 |ll| and truncation h^2 |ll'''| / 6; 1e-8 |ll| + 1e-6 x the largest entry covers both with
    room, and is 1e-3 of the smallest of the pieces (direct term, encoder path) asserted below."""
    S, A, H, _, bs = BR.VARIANTS[tag]
    B = 2 * bs
    enc, dec = (WR.f64(p) for p in BR.vae_params(22, "policy", S, A, H))   # a seed at which 4 tiny rows reach both branches
    s, a, _ = BR.batch(4, S, A, B)
    a = ma * a.astype(np.float64)
    eps = np.random.default_rng(n).standard_normal((B, n, 2 * A))
    beta = 0.5
    d, ll, ex = B2.loglik_grad_action(enc, dec, s, a, eps, beta, ma)
    ref = BR.loglik(enc, dec, "policy", s, a, None, eps, beta, ma)[0][0]
    np.testing.assert_allclose(ll, ref, rtol=1e-13)
    pre = ex["pre"]
    assert min(np.abs(pre + 4).min(), np.abs(pre - 15).min()) > 1e-4, "a pre-clamp log_std sits on a clamp edge: no derivative there"
    assert (pre < -4).any() and (pre > -4).any(), "one clamp branch is not reached"
    h, scale = 1e-6, np.abs(d).max()
    for j in range(A):
        hi, lo = a.copy(), a.copy()
        hi[:, j] += h
        lo[:, j] -= h
        fd = (BR.loglik(enc, dec, "policy", s, hi, None, eps, beta, ma)[0][0] - BR.loglik(enc, dec, "policy", s, lo, None, eps, beta, ma)[0][0]) / (2 * h)
        assert (np.abs(fd - d[:, j]) <= 1e-8 * np.abs(ll) + 1e-6 * scale).all(), (j, np.abs(fd - d[:, j]).max(), scale)
    if n == 1:
        assert (ex["p"] == 1.0).all()
    assert np.abs(ex["direct"]).max() > 1e-3 * scale and np.abs(ex["dxa"]).max() > 1e-3 * scale


def _small_nets(S=3, A=2, H=8):
    q, qt = WR.f64(WR.params(1, S + A, H, 1, 2)), WR.f64(WR.params(2, S + A, H, 1, 2))
    actor, actor_t = WR.f64(WR.params(3, S, H, A, 1)), WR.f64(WR.params(4, S, H, A, 1))
    return q, qt, actor, actor_t


def _fd_check(loss, p, g, rng, h=1e-6, picks=6):
    for k in WR.KEYS:
        for idx in [tuple(rng.integers(0, n) for n in g[k].shape) for _ in range(picks)]:
            hi, lo = {kk: v.copy() for kk, v in p.items()}, {kk: v.copy() for kk, v in p.items()}
            hi[k][idx] += h
            lo[k][idx] -= h
            fd = (loss(hi) - loss(lo)) / (2 * h)
            assert abs(fd - g[k][idx]) < 2e-8 * max(1.0, abs(g[k][idx])) + 1e-9, (k, idx, fd, g[k][idx])


@pytest.mark.parametrize("ma", (1.0, 1.5))
def test_critic_step_gradients_match_finite_differences(ma):
    S, A, bs = 3, 2, 6
    N = 2 * bs
    q, qt, _, actor_t = _small_nets(S, A)
    rng = np.random.default_rng(7)
    s, a, s2 = BR.batch(5, S, A, N)
    r, nd = rng.standard_normal((N, 1)), (rng.random((N, 1)) < 0.8).astype(np.float64)
    noise = np.clip(0.2 * rng.standard_normal((N, A)), -0.5, 0.5)
    mask = (rng.random(N) < 0.5).astype(np.float64)
    y, a2 = B2.critic_targets(qt, actor_t, s2, r, nd, noise, 0.99, ma)
    assert (np.abs(a2) <= ma).all() and y.shape == (N,)
    logs, seed, g = B2.critic_step(q, s, a, y, mask, 0.1)
    assert np.isclose(logs["critic_loss"], logs["critic_td_loss"] + 0.1 * logs["critic_cons_loss"], rtol=1e-14)
    assert 0 < mask.sum() < N and (seed[:, :N // 2][:, mask[:N // 2] == 0] == 0).all()      # a masked target row: no gradient at all
    assert (seed[:, N // 2:][:, mask[N // 2:] == 0] == 0.1 / bs).all()                       # a masked source row: c alone
    _fd_check(lambda p: B2.critic_step(p, s, a, y, mask, 0.1)[0]["critic_loss"], q, g, rng)


@pytest.mark.parametrize("n", (1, 4))
def test_actor_step_gradients_match_finite_differences(n):
    S, A, N, ma, beta, lam = 3, 2, 8, 1.5, 0.5, 0.1
    q, _, actor, _ = _small_nets(S, A)
    enc, dec = (WR.f64(p) for p in BR.vae_params(22, "policy", S, A, 8))
    s = BR.batch(6, S, A, N)[0]
    eps = np.random.default_rng(n).standard_normal((N, n, 2 * A))
    logs, g, ex = B2.actor_step(actor, q, enc, dec, s, eps, beta, lam, ma)
    norm_q = ex["norm_q"]                                                        # detached (:617): held fixed under the differences

    def loss(p):
        pi = WR.forward(p, s, "tanh", ma)[0][0]
        qv = WR.forward({k: v[:1] for k, v in q.items()}, np.concatenate([s, pi], 1))[0][0, :, 0]
        ll = BR.loglik(enc, dec, "policy", s, pi, None, eps, beta, ma)[0][0]
        return -norm_q * qv.mean() + lam * (-ll).mean()
    assert np.isclose(loss(actor), logs["actor_loss"], rtol=1e-13) and logs["neg_log_beta_max"] >= logs["neg_log_beta_mean"]
    _fd_check(loss, actor, g, np.random.default_rng(8))


def test_polyak():
    _, qt, _, _ = _small_nets()
    q = {k: v + 1.0 for k, v in qt.items()}
    out = B2.polyak(qt, q, 0.005)
    assert all(np.allclose(out[k], qt[k] + 0.005, rtol=0, atol=1e-15) for k in qt) and B2.polyak(qt, q, 0.0)["W1"].tolist() == qt["W1"].tolist()


@pytest.mark.parametrize("N", B2.MODE9_ROWS)
@pytest.mark.parametrize("w_zero", (False, True))
def test_mode9_cases_float32_evaluation_within_half_the_gpu_tolerance(N, w_zero):
    """tests/test_hip_bosa_stage2.py checks the kernel's gradients at rtol 1e-5 / atol 1e-5 x the largest entry and the losses at
    rtol 1e-5: a float32 evaluation of the restatement on the same inputs stays within half of both."""
    import golden_util as gu
    import iql_ref as IR
    S, A = B2.MODE9_S, B2.MODE9_A
    q = B2.twin_from_state_dict(IR.iql_params(S, A, 431, 16.0)[1])
    rows, q_next, w, c = B2.mode9_case(N, gu.gi.batch(501, max(N, 64), S, A))
    if w_zero:
        w = np.zeros_like(w)
    s, a, _, r, nd = rows
    out = {}
    for dt in (np.float64, np.float32):
        y = np.asarray(r, dt).reshape(-1) + np.asarray(nd, dt).reshape(-1) * dt(0.99) * np.asarray(q_next, dt)
        out[dt] = B2.critic_step(q, s, a, y, 2 * w, B2.MODE9_COEF, dtype=dt, c=c)
    (l64, seed64, g64), (l32, _, g32) = out[np.float64], out[np.float32]
    assert np.allclose(seed64[:, w == 0], c[w == 0].astype(np.float64), rtol=1e-7, atol=0)          # a masked row's seed is c alone: the case's c
    tol = B2.grad_tolerance(g64)
    worst = max((np.abs(g32[k] - g64[k]) / tol[k]).max() for k in WR.KEYS)
    print("N=%d w_zero=%s: float32 gradients, worst error / tolerance %.4f" % (N, w_zero, worst))
    assert worst <= 0.5
    for k in ("critic_loss", "critic_cons_loss"):
        assert abs(l32[k] - l64[k]) <= 0.5e-5 * abs(l64[k]), (k, l32[k], l64[k])


@pytest.mark.parametrize("tag", ("small", "tiny"))
def test_restatement_follows_the_reference_fixture(tag):
    """g28 (tests/golden/make_golden_bosa2.py): four stage-2 train() calls of the real reference on the CPU, the actor stepping at
    calls 2 and 4.  The composed restatement gives the reference's masks exactly, its logged scalars at rtol 1e-5, its parameters
    within 0.05 lr (g27's bound; the generator measured 0.006 and 0.0008 lr), and leaves the targets alone at calls 1 and 3."""
    import golden_util as gu
    g = gu.load("g28_bosa2_" + tag)
    S, A, H, E, bs = BR.VARIANTS[tag]
    assert (int(g["S"]), int(g["A"]), int(g["hidden"]), int(g["E"]), int(g["bs"])) == (S, A, H, E, bs)
    seed, setting = int(g["seed"]), (float(g["log_std_bias"]), float(g["log_std_scale"]))
    cfg = BR.bosa_cfg(S, A, H, E, vae_iteration=0, epsilon_dyna_exp=float(g["epsilon_dyna_exp"]))
    vae_pol, vae_dyn = BR.vae_params(seed, "policy", S, A, H, 1, *setting), BR.vae_params(seed + 50, "dynamics", S, A, H, E, *setting)
    actor_sd = gu.gi.mlp_params(seed + 1, S, A)
    q_sd = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(seed + 1 + j, S + A, 1).items()}
    assert np.isclose(gu.gi.checksum(actor_sd), float(g["wsum_actor"]), rtol=1e-12) and np.isclose(gu.gi.checksum(q_sd), float(g["wsum_critic"]), rtol=1e-12)
    src, tar = gu.gi.batch(501, 64, S, A), gu.gi.batch(502, 64, S, A)
    mixed = [np.concatenate([t_[:bs], s_[:bs]]) for s_, t_ in zip(src, tar)]
    mixed[4] = g["not_done"]
    assert np.array_equal(mixed[4], 1.0 - np.concatenate([tar[4][:bs], src[4][:bs]]))
    # the fixture's own margins (asserted by the generator, pinned here)
    assert ((g["mask_ratio"] >= 0.25) & (g["mask_ratio"] <= 0.75)).all() and float(g["mask_margin"]) > 10 and float(g["clamp_margin"]) > 1e-3
    st = B2.stage2_init(actor_sd, q_sd)
    nets = {"actor": ("actor", ""), "actor_target": ("actor_target", ""), "critic_1": ("critic", "network1."), "critic_2": ("critic", "network2."),
            "critic_1_target": ("critic_target", "network1."), "critic_2_target": ("critic_target", "network2.")}
    before = None
    for call in (1, 2, 3, 4):
        noise = {k: g["c%d_noise_%s" % (call, k)] for k in ("target", "dynamics", "policy") if "c%d_noise_%s" % (call, k) in g}
        assert ("policy" in noise) == (call % 2 == 0)
        logs = B2.stage2_call(st, vae_pol, vae_dyn, mixed, noise, cfg)
        assert st["total_it"] == int(g["c%d_total_it" % call]) == call
        assert np.array_equal(logs["mask"].astype(np.float32), g["c%d_mask" % call]) and 0 < logs["mask"].sum() < 2 * bs
        names = B2.STAGE2_SCALARS[:4] + (B2.STAGE2_SCALARS[4:] if call % 2 == 0 else ())
        assert {k.split("::")[1] for k in g if k.startswith("c%d_log::" % call)} == set(names)
        for k in names:
            np.testing.assert_allclose(float(logs[k]), float(g["c%d_log::%s" % (call, k)]), rtol=1e-5, err_msg="call %d %s" % (call, k))
        worst = 0.0
        for ref_name, (net, pre) in nets.items():
            sd = B2.to_state_dict(st[net], ("network1.", "network2.") if pre else ("",))
            lr = cfg["actor_lr" if net.startswith("actor") else "critic_lr"]
            for k, v in sd.items():
                if k.startswith(pre + "network."):
                    want = g["c%d_p::%s::%s" % (call, ref_name, k[len(pre):].replace("network.", "net."))]
                    worst = max(worst, float(np.abs(gu.sub(v) - want).max() / lr))
        print("%s call %d: parameters within %.4f lr" % (tag, call, worst))
        assert worst <= 0.05
        targets = {k: {q: v.copy() for q, v in st[k].items()} for k in ("actor_target", "critic_target")}
        if call % 2 == 1 and before is not None:
            assert all(np.array_equal(targets[k][q], before[k][q]) for k in targets for q in targets[k]), "a target moved without an actor step"
        before = targets


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_abi_stays_7_and_the_header_documents_the_new_entry(lib):
    from mobody_amd import _lib
    assert lib.mobody_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    assert "#define MOBODY_ABI_VERSION 7" in hdr
    comments = " ".join(re.findall(r"/\*.*?\*/", hdr, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    name = "mobody_bosa_critic"
    assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name)
    assert re.search(r"\b%s\b" % name, comments) and "seed mode 9" in comments
    # additions only: the block it takes is mobody_critic's, at its size
    assert C.sizeof(_lib.MobodyCritic) == _lib.BLOCK_BYTES[_lib.MobodyCritic]
    src = open(os.path.join(ROOT, "mobody-model-based-off-dynamics-offline-reinforcement-learning_amd", "csrc", "train.h")).read()
    assert "static_assert(sizeof(ConsSeed) <= sizeof(ActorRowArgs)" in src


def _refused(lib, blk, extra, *words):
    assert lib.mobody_bosa_critic(C.byref(blk), *extra, None) == -1
    msg = lib.mobody_last_error().decode()
    assert msg.startswith("mobody_bosa_critic:"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_bosa_critic_refusals_come_before_any_launch(lib):
    from mobody_amd import _lib
    d, h = _lib.MobodyTrainDims(17, 6, 64, 64, 64, 64), _lib.MobodyHyper(0.99, 0.005, 1.0, 2.5, 0.1, 1, 1, 0)
    ok = dict(d=d, h=h, grad_q=PTR, q_next=PTR)
    blk = lambda **over: _lib.block(_lib.MobodyCritic, **{**ok, **over})
    rows = (PTR, PTR, 0.1, 32)
    _refused(lib, _lib.MobodyCritic(struct_bytes=8), rows, "struct_bytes")
    _refused(lib, blk(grad_q=None), rows, "exactly one of grad_q")
    _refused(lib, blk(m=PTR, v=PTR), rows, "exactly one of grad_q")
    _refused(lib, blk(phase=1), rows, "phase, gather and policy_forward")
    _refused(lib, blk(policy_forward=1), rows, "phase, gather and policy_forward")
    _refused(lib, blk(q_next=None), rows, "q_next is NULL")
    _refused(lib, blk(), (None, PTR, 0.1, 32), "row_weight / row_const is NULL")
    _refused(lib, blk(), (PTR, None, 0.1, 32), "row_weight / row_const is NULL")
    _refused(lib, blk(), (PTR, PTR, 0.1, 0), "cons_rows_global 0")
    _refused(lib, blk(), rows, "null pointer")                       # every argument of its own is in order: refused further on


def test_bosa_config_check_is_unchanged():
    """No key was added to the class's required set; a config without `critic_actor` passes the check, one that lacks a BOSA key is
    refused with the key named (the class itself needs a GPU: tests/test_hip_bosa_class.py holds its refusals)."""
    from mobody_amd.algo.offline_offline import bosa
    assert "critic_actor" not in bosa._KEYS
    cfg = BR.bosa_cfg(17, 6, 72, 2)
    bosa._check_config(cfg)
    with pytest.raises(NotImplementedError, match=r"config lacks \['conservation_coef'\]"):
        bosa._check_config({k: v for k, v in cfg.items() if k != "conservation_coef"})
