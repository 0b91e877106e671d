"""CPU checks for BOSA's actor phase and stage-2 step: the new entries' declarations, that every refusal of theirs comes
before any runtime call (nothing is launched here) with its field named, the gradient workspace against its closed form, the keyed
constructor's missing-key refusals, and the precondition of the GPU tests' normalised tolerances -- a float32 evaluation of the fp64
restatement on the GPU tests' exact inputs stays within half of them: at the fixture variants' shapes and at every wide, edge and
product-batch case of tests/bosa_actor_cases.py and bosa2_ref.MODE9_EDGE_CASES.  The offsets through which the GPU tests read p_k, the
encoder's seed and the actor's seed out of the two workspaces are partial sums of closed forms that are held against the library's
totals here, at the old shape and at new ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bosa2_ref as B2
import bosa_actor_cases as BC
import bosa_ref as BR
import wide_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000
NEW = ("mobody_wide_mlp3_input_grad", "mobody_bosa_loglik_grad_workspace", "mobody_bosa_loglik_grad", "mobody_bosa_actor_forward",
       "mobody_bosa_actor_backward")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_abi_stays_7_and_the_header_documents_the_new_entries(lib):
    from mobody_amd import _lib, ops
    assert lib.mobody_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    assert "#define MOBODY_ABI_VERSION 7" in hdr
    blocks = re.findall(r"/\*.*?\*/", hdr, flags=re.S)
    comments = " ".join(blocks)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert re.search(r"\b%s\b" % name, comments), name
    for name in ("mobody_bosa_loglik_grad", "mobody_bosa_actor_forward", "mobody_bosa_actor_backward"):
        assert any(name in b and re.search(r"bosa\.py:\d+", b) for b in blocks), name     # cites the reference lines it replaces
    P, vp = C.POINTER, _lib.vp
    assert _lib.PROTOTYPES["mobody_wide_mlp3_input_grad"] == (C.c_int, [P(_lib.MobodyWideBwd), vp])
    assert _lib.PROTOTYPES["mobody_bosa_loglik_grad_workspace"] == (C.c_int64, [P(_lib.MobodyBosaVae)])
    assert _lib.PROTOTYPES["mobody_bosa_loglik_grad"] == (C.c_int, [P(_lib.MobodyBosaVae), vp, vp])
    assert _lib.PROTOTYPES["mobody_bosa_actor_forward"] == _lib.PROTOTYPES["mobody_bosa_actor_backward"] == (C.c_int, [P(_lib.MobodyActor), vp, vp])
    # additions only: the blocks keep their sizes, the new stream id is in the header
    for cls in (_lib.MobodyActor, _lib.MobodyBosaVae, _lib.MobodyWideBwd):
        assert C.sizeof(cls) == _lib.BLOCK_BYTES[cls]
    assert _lib.BOSA_STREAMS["target_noise"] == 10 and "MOBODY_BOSA_STREAM_TARGET_NOISE = 10" in code
    for f in ("wide_mlp3_input_grad", "bosa_loglik_grad_workspace", "bosa_loglik_grad", "bosa_actor_forward", "bosa_actor_backward"):
        assert callable(getattr(ops, f)), f


def _refused(call, entry, *words):
    from mobody_amd import _lib
    assert call() == -1, entry
    msg = _lib.load().mobody_last_error().decode()
    assert msg.startswith((entry + ":", "mobody_wide_layout:")), msg
    for w in words:
        assert w in msg, (w, msg)


def test_input_grad_refusals_come_before_any_runtime_call(lib):
    from mobody_amd import _lib
    entry = "mobody_wide_mlp3_input_grad"
    L = _lib.wide_layout(23, 72, 6, 1)
    ok = dict(layout=L, blob=PTR, dz3=PTR, h1=PTR, h2=PTR, x_shared=1, rows=99, dx=PTR, dx_col0=17, dx_col1=23, workspace=PTR)
    run = lambda **over: (lambda: lib.mobody_wide_mlp3_input_grad(C.byref(_lib.block(_lib.MobodyWideBwd, **{**ok, **over})), None))
    _refused(lambda: lib.mobody_wide_mlp3_input_grad(C.byref(_lib.MobodyWideBwd(struct_bytes=8)), None), entry, "struct_bytes")
    _refused(run(grad=PTR), entry, "grad must be NULL")
    _refused(run(dx=None), entry, "dx is NULL")
    _refused(run(precision=4), entry, "precision 4", "exact fp32")
    _refused(run(rows=0), entry, "rows 0 outside [1, 2^21]")
    _refused(run(rows=(1 << 21) + 1), entry, "outside [1, 2^21]")
    _refused(run(dz3=None), entry, "null pointer")
    _refused(run(workspace=None), entry, "null pointer")
    _refused(run(x_shared=2), entry, "x_shared 2")
    _refused(run(dx_col1=24), entry, "dx columns [17, 24) outside [0, 23)")
    bad = _lib.wide_layout(23, 72, 6, 1)
    bad.Hp = 64
    _refused(run(layout=bad), entry, "the layout is not mobody_wide_layout's")


def test_loglik_grad_refusals_come_before_any_runtime_call(lib):
    from mobody_amd import _lib
    entry = "mobody_bosa_loglik_grad"
    ok = dict(kind=0, S=17, A=6, hidden=72, members=1, B=8, beta=0.5, max_action=1.0, num_samples=4, blob=PTR, state=PTR, action=PTR, ll=PTR,
              workspace=PTR)
    run = lambda dll=PTR, **over: (lambda: lib.mobody_bosa_loglik_grad(C.byref(_lib.block(_lib.MobodyBosaVae, **{**ok, **over})), dll, None))
    cls = _lib.MobodyBosaVae
    _refused(lambda: lib.mobody_bosa_loglik_grad(C.byref(cls(struct_bytes=C.sizeof(cls) - 1)), PTR, None), entry, "struct_bytes")
    _refused(run(kind=1, members=2, next_state=PTR), entry, "kind 1", "policy VAE")
    _refused(run(kind=2), entry, "kind 2")
    _refused(run(members=2), entry, "the policy VAE has one member")
    _refused(run(hidden=1025), entry, "hidden 1025")
    _refused(run(A=65), entry, "out_dim 260")
    _refused(run(precision=4), entry, "precision 4", "exact fp32")
    _refused(run(B=0), entry, "B 0")
    _refused(run(beta=0.0), entry, "beta 0")
    for n in (0, 65, -1):
        _refused(run(num_samples=n), entry, "num_samples %d outside [1, 64]" % n)
    _refused(run(grad=PTR), entry, "grad, m, v must be NULL")
    _refused(run(state=None), entry, "null pointer")
    _refused(run(ll=None), entry, "null pointer")
    _refused(run(dll=None), entry, "dll_da is NULL")
    _refused(run(mask_mean=PTR), entry, "mask_mean needs mask")
    _refused(run(B=1 << 20, num_samples=3), entry, "num_samples * B = 3145728 > 2^21")
    blk = lambda **over: C.byref(_lib.block(cls, **{**ok, **over}))
    assert lib.mobody_bosa_loglik_grad_workspace(blk(kind=1, members=2)) == -1
    assert lib.mobody_bosa_loglik_grad_workspace(blk(num_samples=0)) == -1 and lib.mobody_bosa_loglik_grad_workspace(blk(num_samples=65)) == -1
    assert lib.mobody_bosa_loglik_grad_workspace(blk(B=0)) == -1 and lib.mobody_bosa_loglik_grad_workspace(None) == -1


@pytest.mark.parametrize("n", (1, 3, 10))
def test_loglik_grad_workspace_closed_form(lib, n):
    """mobody_bosa_workspace keeps its value and comes first; behind it the seed [n B][A], dz [n B][Lz], the decoder's backward scratch
    2 [n B][Hp] and the two [B][A] pieces, each rounded up to four floats."""
    from mobody_amd import _lib
    S, A, H, B = 17, 6, 72, 33
    blk = _lib.block(_lib.MobodyBosaVae, kind=0, S=S, A=A, hidden=H, members=1, B=B, beta=0.5, max_action=1.0, num_samples=n)
    r4 = lambda v: (v + 3) & ~3
    Hp, Lz, nB = 96, 2 * A, n * B
    enc, dec = _lib.wide_layout(S + A, H, 2 * Lz, 1), _lib.wide_layout(S + Lz, H, A, 1)
    assert (enc.Hp, dec.Hp, enc.Kp1, dec.Kp1) == (Hp, Hp, 32, 32)
    base = (r4(B * enc.Kp1) + 2 * r4(B * Hp) + r4(B * 2 * Lz) + r4(nB * Lz) + r4(nB * dec.Kp1) + 2 * r4(nB * Hp) + r4(nB * A) + r4(B * A) + r4(B * Lz) +
            r4(B * 2 * Lz) + r4(2 * B * Hp) + r4(-(-B * Lz // 256)) + r4(-(-B * A // 256)) + r4(2 * nB))
    assert lib.mobody_bosa_workspace(C.byref(blk)) == base
    assert lib.mobody_bosa_loglik_grad_workspace(C.byref(blk)) == base + r4(nB * A) + r4(nB * Lz) + r4(2 * nB * Hp) + 2 * r4(B * A)


@pytest.mark.parametrize("shape,B,n", [((17, 6, 72), 33, 3), ((45, 24, 750), 64, 4), ((128, 64, 1024), 17, 2), ((3, 1, 8), 4, 64), ((1, 1, 8), 33, 3)])
def test_workspace_offsets_the_gpu_tests_read_through_add_up_to_the_library_totals(lib, shape, B, n):
    """The GPU tests read p_k (pq's second slot) and the encoder's seed out of the estimator's workspace at offsets that depend on
    (S, A, H, B, n) through the layouts' Kp1 and Hp: tests/bosa_actor_cases.py's closed form, of which those offsets are partial
    sums, gives the library's totals at the old shape and at new ones (pen at the product's width, the largest policy VAE, n = 64,
    the smallest layout)."""
    from mobody_amd import _lib
    S, A, H = shape
    blk = _lib.block(_lib.MobodyBosaVae, kind=0, S=S, A=A, hidden=H, members=1, B=B, beta=0.5, max_action=1.0, num_samples=n)
    base, grad = BC.bosa_workspace_floats(S, A, H, B, n)
    assert lib.mobody_bosa_workspace(C.byref(blk)) == base and lib.mobody_bosa_loglik_grad_workspace(C.byref(blk)) == grad
    assert 0 < BC.denc_offset(S, A, H, B, n) < BC.pq_offset(S, A, H, B, n) == base - ((2 * n * B + 3) & ~3)


@pytest.mark.parametrize("S,A,N", [(17, 6, 33), (17, 6, 2), (17, 6, 256), (17, 6, 1025), (11, 3, 65), (45, 24, 65), (111, 8, 65)])
def test_train_workspace_offset_of_the_actor_seed_adds_up_to_the_library_total(lib, S, A, N):
    """dz3a_offset depends on (S, A, N) through the layouts' Kp1 / Np3 and the 32-row tiles: the closed form it is a partial sum of
    gives mobody_train_workspace at the old shape and at the new row edges and widths."""
    from mobody_amd import _lib
    d = _lib.MobodyTrainDims(S, A, N, N, N, N)
    assert lib.mobody_train_workspace(C.byref(d)) == BC.train_workspace_floats(S, A, N)
    off, Np3 = BC.dz3a_offset(S, A, N)
    assert Np3 > A and off % 4 == 0                 # every case has padding columns, which the GPU test holds at exactly 0


@pytest.mark.parametrize("entry", ("mobody_bosa_actor_forward", "mobody_bosa_actor_backward"))
def test_actor_refusals_come_before_any_runtime_call(lib, entry):
    from mobody_amd import _lib
    d, h = _lib.MobodyTrainDims(17, 6, 64, 64, 64, 64), _lib.MobodyHyper(0.99, 0.005, 1.0, 1.0, 0.0, 0, 1, 0)
    ok = dict(d=d, h=h, actor_blob=PTR, actor_blob_T=PTR, q_blob=PTR, q_blob_T=PTR, state=PTR, stats=PTR, workspace=PTR, grad_actor=PTR, loss_out=PTR)
    fn = getattr(lib, entry)
    run = lambda extra=PTR, **over: (lambda: fn(C.byref(_lib.block(_lib.MobodyActor, **{**ok, **over})), extra, None))
    _refused(lambda: fn(C.byref(_lib.MobodyActor(struct_bytes=8)), PTR, None), entry, "struct_bytes")
    _refused(run(d=_lib.MobodyTrainDims(17, 6, 0, 0, 0, 0)), entry, "need 1 <= N")
    _refused(run(d=_lib.MobodyTrainDims(17, 6, (1 << 21) + 1, 0, (1 << 21) + 1, 0)), entry, "d.N 2097153 > 2^21")
    _refused(run(v_true=PTR), entry, "v_true given")
    _refused(run(policy_ready=1), entry, "policy_ready 1")
    for prec, name in ((1, "bf16"), (2, "bf16x2")):
        _refused(run(h=_lib.MobodyHyper(0.99, 0.005, 1.0, 1.0, 0.0, 0, 1, prec)), entry, "precision %d" % prec, "0 (f32), 3 (bf16x3), 4 (f16x2)")
    _refused(run(h=_lib.MobodyHyper(0.99, 0.005, 1.0, 1.0, 0.0, 0, 1, 4), actor_blob_T=None), entry, "split-precision modes need the T blobs")
    _refused(run(state=None), entry, "null pointer")
    if entry.endswith("forward"):
        _refused(run(extra=None), entry, "pi_out is NULL")
    else:
        _refused(run(extra=None), entry, "dpi_extra is NULL")
        _refused(run(grad_actor=None), entry, "exactly one of grad_actor")
        _refused(run(m=PTR, v=PTR), entry, "exactly one of grad_actor")
        _refused(run(grad_actor=None, m=PTR, v=PTR), entry, "step t must be >= 1")
        _refused(run(loss_out=None), entry, "null pointer")


def test_keyed_config_names_the_missing_keys():
    """The pieces of the constructor's stage-2 refusal: the key set, and the wording it gets from refuse_missing_keys.  The class
    refuses a non-GPU device first, so the constructor's own path -- all four keys, before anything is built -- is held by
    tests/test_hip_bosa_actor.py::test_without_the_key_the_boundary_refusal_is_what_it_was."""
    from mobody_amd.algo.offline_offline import bosa
    from mobody_amd.algo.offline_offline.mobody import refuse_missing_keys
    assert bosa.STAGE2_KEYS == ("gamma", "tau", "actor_lr", "critic_lr") and "critic_actor" not in bosa._KEYS
    assert bosa.STAGE2_LOG_KEYS == B2.STAGE2_SCALARS
    cfg = BR.bosa_cfg(17, 6, 72, 2, critic_actor=1)
    bosa._check_config(cfg)
    for k in bosa.STAGE2_KEYS:
        short = {q: v for q, v in cfg.items() if q != k}
        with pytest.raises(NotImplementedError, match=r"BOSA is built from a BOSA config only: config lacks \['%s'\]" % k):
            refuse_missing_keys("BOSA", [q for q in bosa.STAGE2_KEYS if q not in short], "config/*/bosa/*.yaml values")
    assert len(bosa.STAGE2_FILES + bosa.TARGET_FILES) == 9 and "__critic_2_optimizer" in bosa.STAGE2_FILES


# ---- the preconditions of the GPU tests' tolerances --------------------------------------------------------------------------------
def test_float32_estimator_gradient_within_half_the_gpu_tolerance():
    """All of tests/test_hip_bosa_actor.py's gradient cases: no pre-clamp log_std sits within 1e-4 of a clamp edge (a float32 gate
    could differ there), and the float32 evaluation of the restatement stays within half of both tolerances."""
    worst_d = worst_ll = 0.0
    for c in BC.LLG_CASES:
        _, _, _, enc, dec, s, a, eps = BC.llg_case(*c)
        d64, ll64, ex = BC.llg_reference(*c)
        d32, ll32, _ = B2.loglik_grad_action(enc, dec, s, a, eps, BC.BETA, c[3], dtype=np.float32)
        assert min(np.abs(ex["pre"] + 4).min(), np.abs(ex["pre"] - 15).min()) > 1e-4, c
        tol_d, tol_ll = BC.llg_tolerances(d64, ll64, ex["w"])
        rd, rl = (np.abs(d32 - d64) / tol_d).max(), (np.abs(ll32 - ll64) / tol_ll).max()
        worst_d, worst_ll = max(worst_d, rd), max(worst_ll, rl)
        if c[1] == 1:
            assert (ex["p"] == 1.0).all()
        assert np.abs(ex["direct"]).max() > 1e-3 * np.abs(d64).max() and np.abs(ex["dxa"]).max() > 1e-3 * np.abs(d64).max(), c
    print("float32 dll_da: worst error / tolerance %.4f; ll: %.4f" % (worst_d, worst_ll))
    assert worst_d <= 0.5 and worst_ll <= 0.5


def test_float32_estimator_gradient_within_half_the_gpu_tolerance_at_the_wide_cases():
    """The same at tests/bosa_actor_cases.py's LLG_WIDE_CASES (the product's shape, exact tiles, workgroup edges, the largest n, the
    corners of the policy VAE's layout, beta 0.05).  At B up to 513 some pre-clamp log_std comes nearer to -4 than 1e-4 (1.8e-5 at
    (17, 6, 72), B 256), so the gate's margin is held against the float32 evaluation's own error of that value instead: no
    pre-clamp log_std lies within eight times the largest |pre32 - pre64| of the case of a clamp edge, and both evaluations pass the
    same columns.  The peaked cases are what their name says: against the same inputs at beta 0.5 the weights of a row spread
    further, the largest |w| is more than four times and the direct term more than nine times as large."""
    worst_d = worst_ll = 0.0
    for c in BC.LLG_WIDE_CASES:
        shape, n, B, ma, beta = c
        _, _, _, enc, dec, s, a, eps = BC.llg_case(*c)
        d64, ll64, ex = BC.llg_reference(*c)
        d32, ll32, ex32 = B2.loglik_grad_action(enc, dec, s, a, eps, beta, ma, dtype=np.float32)
        margin = min(np.abs(ex["pre"] + 4).min(), np.abs(ex["pre"] - 15).min())
        pre_err = np.abs(ex32["pre"] - ex["pre"]).max()
        passes = lambda pre: (pre >= -4) & (pre <= 15)
        assert margin > 8 * pre_err and np.array_equal(passes(ex["pre"]), passes(ex32["pre"])), (c, margin, pre_err)
        tol_d, tol_ll = BC.llg_tolerances(d64, ll64, ex["w"])
        rd, rl = (np.abs(d32 - d64) / tol_d).max(), (np.abs(ll32 - ll64) / tol_ll).max()
        print("%s: float32 dll_da error / tolerance %.4f, ll %.4f; clamp margin %.2e (float32 error of pre %.1e)" % (BC.llg_id(c), rd, rl, margin, pre_err))
        worst_d, worst_ll = max(worst_d, rd), max(worst_ll, rl)
        if n == 1:
            assert (ex["p"] == 1.0).all()
        assert np.abs(ex["direct"]).max() > 1e-3 * np.abs(d64).max() and np.abs(ex["dxa"]).max() > 1e-3 * np.abs(d64).max(), c
        if beta == BC.PEAKED_BETA:
            base = BC.llg_reference(shape, n, B, ma)[2]
            spread = lambda w: (w.max(0) - w.min(0)).max()
            assert spread(ex["w"]) > spread(base["w"]) and np.abs(ex["w"]).max() > 4 * np.abs(base["w"]).max()
            assert np.abs(ex["direct"]).max() > 9 * np.abs(base["direct"]).max()
    print("float32 dll_da: worst error / tolerance %.4f; ll: %.4f" % (worst_d, worst_ll))
    assert worst_d <= 0.5 and worst_ll <= 0.5


def _float32_actor_ratios(N, SA, qcut):
    """(d(pre-tanh), gradient, pi, loss head) of a float32 evaluation of the actor step, each as error / tolerance."""
    logs64, g64, ex64 = BC.actor_reference(N, 1.0, 0.0, qcut=qcut, SA=SA)
    logs32, g32, ex32 = BC.actor_reference(N, 1.0, 0.0, dtype=np.float32, qcut=qcut, SA=SA)
    d64, d32 = BC.pre_tanh_seed(ex64, 1.0), BC.pre_tanh_seed(ex32, 1.0, np.float32)
    tol = B2.grad_tolerance(g64)
    head = -ex64["norm_q"] * ex64["q"].mean()
    if qcut:
        assert 0.2 < (ex64["q"] < 0).mean() < 0.3 and abs(head) < 0.9
    return ((np.abs(d32 - d64) / BC.seed_tolerance(d64)).max(), max((np.abs(g32[k] - g64[k]) / tol[k]).max() for k in WR.KEYS),
            (np.abs(ex32["pi"] - ex64["pi"]) / (1e-5 + 1e-5 * np.abs(ex64["pi"]))).max(),
            abs(float(-ex32["norm_q"] * ex32["q"].mean()) - head) / (1e-5 * abs(head)))


@pytest.mark.parametrize("c", BC.EDGE_CASES, ids=BC.edge_id)
def test_float32_actor_step_within_half_the_gpu_tolerance_at_the_edges(c):
    """tests/bosa_actor_cases.py's EDGE_CASES, with the qcut = 0.25 variant where the GPU test runs it."""
    N, SA = c
    for qcut in ((0.0, 0.25) if N in BC.QCUT_ROWS and SA == BC.ACTOR_SA else (0.0,)):
        ratios = _float32_actor_ratios(N, SA, qcut)
        print("%s qcut=%g: float32 d(pre-tanh) error / tolerance %.4f, gradient %.4f, pi %.4f, loss head %.4f" % ((BC.edge_id(c), qcut) + ratios))
        assert max(ratios) <= 0.5


@pytest.mark.parametrize("c", B2.MODE9_EDGE_CASES, ids=BC.edge_id)
@pytest.mark.parametrize("w_zero", (False, True))
def test_float32_mode9_within_half_the_gpu_tolerance_at_the_edges(c, w_zero):
    """As tests/test_bosa2_ref.py::test_mode9_cases_float32_evaluation_within_half_the_gpu_tolerance, at the edge cases that
    tests/test_hip_bosa_stage2.py runs: gradients against grad_tolerance, the two losses against rtol 1e-5."""
    N, SA = c
    assert B2.MODE9_EDGE_CASES == BC.EDGE_CASES
    q = B2.twin_from_state_dict(B2.mode9_params(SA))
    rows, q_next, w, c9 = B2.mode9_case(N, SA=SA)
    assert 0 < (w != 0).sum() < N
    if w_zero:
        w = np.zeros_like(w)
    s, a, _, r, nd = rows
    out = {}
    for dt in (np.float64, np.float32):
        y = np.asarray(r, dt).reshape(-1) + np.asarray(nd, dt).reshape(-1) * dt(0.99) * np.asarray(q_next, dt)
        out[dt] = B2.critic_step(q, s, a, y, 2 * w, B2.MODE9_COEF, dtype=dt, c=c9)
    (l64, _, g64), (l32, _, g32) = out[np.float64], out[np.float32]
    tol = B2.grad_tolerance(g64)
    worst = max((np.abs(g32[k] - g64[k]) / tol[k]).max() for k in WR.KEYS)
    scalars = max(abs(l32[k] - l64[k]) / (1e-5 * abs(l64[k])) for k in ("critic_loss", "critic_cons_loss"))
    print("%s w_zero=%s: float32 gradients, worst error / tolerance %.4f; losses / rtol 1e-5 %.4f" % (BC.edge_id(c), w_zero, worst, scalars))
    assert worst <= 0.5 and scalars <= 0.5


def test_float32_stage2_scalars_within_half_the_gpu_tolerance_at_the_product_batch():
    """BC.BATCH_SHAPE, two calls: the mask threshold sits in a gap of more than ten estimator tolerances (the GPU test asserts the
    masks exactly), both masks keep rows on either side, and the float32 scalars stay within half of the class test's bound."""
    cfg, _, _, _, mixed, (gap, tol) = BC.batch_setup()
    assert len(mixed[0]) == 256 and gap > 10 * tol and np.exp(-700) < cfg["epsilon_dyna_exp"] < 1
    worst = {}
    for call, l32, l64, st in BC.stage2_calls("batch", np.float32):
        assert 0.25 <= st["mask"].mean() <= 0.75
        terms = BC.scalar_terms(l64, cfg)
        for k in B2.STAGE2_SCALARS[:8 if call % 2 == 0 else 4]:
            worst[k] = max(worst.get(k, 0.0), abs(l32[k] - l64[k]) / (1e-5 * abs(l64[k]) + 1e-5 * terms[k] + 1e-300))
    assert call == 2 and st["ta"] == 1 and st["tq"] == 2
    print("batch", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("N", BC.ACTOR_ROWS)
@pytest.mark.parametrize("shift,qcut", ((0.0, 0.0), (100.0, 0.0), (0.0, 0.25)))
def test_float32_actor_step_within_half_the_gpu_tolerance(N, shift, qcut):
    logs64, g64, ex64 = BC.actor_reference(N, 1.0, shift, qcut=qcut)
    logs32, g32, ex32 = BC.actor_reference(N, 1.0, shift, dtype=np.float32, qcut=qcut)
    d64, d32 = BC.pre_tanh_seed(ex64, 1.0), BC.pre_tanh_seed(ex32, 1.0, np.float32)
    seed_r = (np.abs(d32 - d64) / BC.seed_tolerance(d64)).max()
    print("N=%d shift=%g qcut=%g: float32 d(pre-tanh) per element, worst error / tolerance %.4f" % (N, shift, qcut, seed_r))
    assert seed_r <= 0.5
    if qcut:
        assert 0.2 < (ex64["q"] < 0).mean() < 0.3 and abs(-ex64["norm_q"] * ex64["q"].mean()) < 0.9
    tol = B2.grad_tolerance(g64)
    worst = max((np.abs(g32[k] - g64[k]) / tol[k]).max() for k in WR.KEYS)
    pi_r = (np.abs(ex32["pi"] - ex64["pi"]) / (1e-5 + 1e-5 * np.abs(ex64["pi"]))).max()
    head = -ex64["norm_q"] * ex64["q"].mean()
    print("N=%d shift=%g: float32 actor gradient, worst error / tolerance %.4f; pi %.4f" % (N, shift, worst, pi_r))
    assert worst <= 0.5 and pi_r <= 0.5
    assert abs(float(-ex32["norm_q"] * ex32["q"].mean()) - head) <= 0.5e-5 * abs(head)
    if shift:                                   # member 1 lies below member 0 on every row: a min-Q implementation would differ
        pa, pq, *_ = BC.actor_case(N, 1.0, shift)
        q = B2._fwd(WR.f64(B2.twin_from_state_dict(pq)), np.broadcast_to(np.concatenate([BC.actor_case(N)[4], ex64["pi"]], 1), (2, N, 23)))[0][:, :, 0]
        assert (q[1] < q[0] - 50).all()


@pytest.mark.parametrize("tag", ("small", "tiny"))
def test_float32_stage2_scalars_within_half_the_gpu_tolerance(tag):
    """The class test holds each logged scalar at rtol 1e-5 with atol 1e-5 x the sum of the magnitudes of its terms: a float32
    evaluation on the same state stays within half; the fp64 composition is the fixture's."""
    g, cfg, *_ = BC.g28_setup(tag)
    worst = {}
    for call, l32, l64, _ in BC.stage2_calls(tag, np.float32):
        terms = BC.scalar_terms(l64, cfg)
        for k in B2.STAGE2_SCALARS[:8 if call % 2 == 0 else 4]:
            np.testing.assert_allclose(l64[k], float(g["c%d_log::%s" % (call, k)]), rtol=1e-5, err_msg="call %d %s" % (call, k))
            ratio = abs(l32[k] - l64[k]) / (1e-5 * abs(l64[k]) + 1e-5 * terms[k] + 1e-300)
            worst[k] = max(worst.get(k, 0.0), ratio)
    print(tag, {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst
