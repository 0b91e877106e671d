"""Inputs, fp64 references and tolerances shared by tests/test_bosa_actor_ref.py (CPU) and tests/test_hip_bosa_actor.py (GPU): the cases
of the estimator's gradient (mobody_bosa_loglik_grad), of BOSA's actor phase (mobody_bosa_actor_forward / _backward) and of the
class's stage-2 call against the g28 fixtures.  Every reference is computed once and cached.

Beside the fixture variants' mild shapes (LLG_CASES, ACTOR_ROWS, g28) it holds the shapes the product runs and the kernels' edges:
LLG_WIDE_CASES (explicit (S, A, H), rows, samples, beta), EDGE_CASES / QCUT_ROWS / SPLIT_CASES for the actor phase and mode 9, and
one class call at the product's batch whose expectation is the fp64 restatement alone (batch_setup, stage2_calls("batch")).  The
builders take the shape as an argument; the seeds, generators and call order are those of the first cases, whose inputs keep their
bits.  The closed forms of both workspaces live here too, so that the CPU suite can tie the offsets the GPU tests read through to the
library's totals."""
import functools

import numpy as np

import bosa2_ref as B2
import bosa_ref as BR
import golden_util as gu
import wide_ref as WR

BETA = 0.5
VAE_SEED = 22                       # tests/test_bosa2_ref.py's: both clamp branches are reached on the fixture variants' rows
# (variant, num_samples, rows, max_action): rows = 2 bs of the variant and 33, so that n B is 99 and 330 and never a multiple of 64
LLG_CASES = [(tag, n, B, ma) for tag in ("tiny", "small", "pen") for n in (1, 3, 10) for B in (2 * BR.VARIANTS[tag][4], 33) for ma in (1.0, 2.0)]


# Explicit shapes, ((S, A, H), num_samples, rows, max_action, beta): the product's width and batch (VAEs 750 wide, 256 mixed rows), row
# counts that are exact 64-row tiles of the wide GEMM (n B = 128, 256, 2560), the first and last row of a 256-thread workgroup of the
# row-wise kernels and their third workgroup, the largest num_samples, the smallest and the largest policy VAE the layouts take
# (4 A = 256 encoder outputs, S + 2 A = 256 decoder inputs) at the smallest and the largest hidden width, pen and ant at the product's
# width, and a sharply peaked softmax (beta 0.05: |w| reaches 360, the spread within a row 38 nats, the direct term is ten times
# larger).  beta 0.01 is left out: at H 750 a float32 evaluation of the restatement itself is 2.1 times over the gradient tolerance.
WALKER, WALKER_WIDE = (17, 6, 72), (17, 6, 750)
LLG_WIDE_CASES = ([(WALKER_WIDE, n, 256, 1.0, BETA) for n in (1, 10)] + [(WALKER_WIDE, 3, 513, 1.0, BETA)] +
                  [(WALKER, 3, B, 1.0, BETA) for B in (1, 255, 256, 257)] +
                  [(WALKER, 2, 64, 1.0, BETA), ((3, 1, 8), 64, 4, 1.0, BETA), (WALKER, 64, 33, 1.0, BETA), ((1, 1, 8), 3, 33, 1.0, BETA),
                   ((128, 64, 8), 3, 33, 1.0, BETA), ((128, 64, 1024), 2, 17, 1.0, BETA), ((45, 24, 750), 4, 64, 1.0, BETA),
                   ((111, 8, 750), 3, 65, 1.0, BETA), (WALKER_WIDE, 10, 256, 1.0, 0.05), (WALKER, 10, 257, 1.0, 0.05)])
PEAKED_BETA = 0.05


def llg_id(c):
    if isinstance(c[0], str):
        return "%s-n%d-B%d-ma%g" % c
    return "s%da%dh%d-n%d-B%d-ma%g-beta%g" % (c[0] + c[1:])


def llg_shape(shape):
    """(S, A, H) of a BR.VARIANTS tag or of an explicit (S, A, H)."""
    return BR.VARIANTS[shape][:3] if isinstance(shape, str) else tuple(shape)


@functools.lru_cache(maxsize=None)
def llg_case(shape, n, B, ma, beta=BETA):
    """(S, A, H, enc, dec, s, a, eps) in fp32; a is the point of evaluation, inside (-ma, ma).  shape: a BR.VARIANTS tag or (S, A, H);
    the inputs do not depend on beta."""
    S, A, H = llg_shape(shape)
    enc, dec = BR.vae_params(VAE_SEED, "policy", S, A, H)
    s, a, _ = BR.batch(4, S, A, B)
    eps = np.random.default_rng(n).standard_normal((B, n, 2 * A)).astype(np.float32)
    return S, A, H, enc, dec, s, (np.float32(ma) * a).astype(np.float32), eps


@functools.lru_cache(maxsize=None)
def llg_reference(shape, n, B, ma, beta=BETA):
    """(dll_da [B, A], ll [B], extras) of tests/bosa2_ref.loglik_grad_action in fp64."""
    _, _, _, enc, dec, s, a, eps = llg_case(shape, n, B, ma)
    return B2.loglik_grad_action(enc, dec, s, a, eps, beta, ma)


def llg_tolerances(d64, ll64, w64):
    """(dll_da: the project's gradient tolerance rtol 1e-5 / atol 1e-5 x max |dll_da|, ll: BR.estimator_tolerance); w64 [n, B]."""
    return 1e-5 * np.abs(d64) + 1e-5 * np.abs(d64).max(), BR.estimator_tolerance(ll64[None], w64[None])[0]


# ---- the actor phase: walker shapes, one row past one and past eight 32-row tiles -----------------------------------------------------
ACTOR_S, ACTOR_A, ACTOR_H, ACTOR_ROWS, ACTOR_N_SAMPLES, ACTOR_LAMDA = 17, 6, 72, (33, 257), 3, 0.25
ACTOR_SA = (ACTOR_S, ACTOR_A)
# The row edges at walker shapes -- the smallest N, one and two exact 32-row tiles, the product's 256, and 1024 / 1025: k_bosa_actor_stats
# strides by 1024 threads, its second trip starts at row 1025 -- and other widths at N = 65: a narrow net, pen (A = 24) and ant (S = 111).
# Mode 9 (tests/test_hip_bosa_stage2.py) runs at the same ones.
EDGE_ROWS = (2, 32, 64, 256, 1024, 1025)
EDGE_WIDTHS, EDGE_WIDTH_ROWS = ((11, 3), (45, 24), (111, 8)), 65
EDGE_CASES = [(N, ACTOR_SA) for N in EDGE_ROWS] + [(EDGE_WIDTH_ROWS, SA) for SA in EDGE_WIDTHS]
QCUT_ROWS = (256, 1025)                 # the qcut = 0.25 variant, so that the loss is not +-1
SPLIT_CASES = [(256, ACTOR_SA), (EDGE_WIDTH_ROWS, (45, 24))]     # the split precisions (f16x2, bf16x3) of both


def edge_id(c):
    return "N%d-s%da%d" % (c[0], c[1][0], c[1][1])


@functools.lru_cache(maxsize=None)
def actor_case(N, ma=1.0, shift=0.0, qcut=0.0, SA=ACTOR_SA):
    """(actor state dict, twin-Q state dict, enc, dec, s [N, S], eps [N, n, Lz]).  shift: subtracted from critic_2's output bias, so that
    member 1 lies below member 0 on every row and a min-Q implementation differs.  qcut in (0, 1): critic_1's output bias is moved so
    that this fraction of the rows has q_0 < 0 -- without it every q_0 of these nets has one sign and -mean(q) / mean|q| is +-1.
    SA: (state_dim, action_dim)."""
    S, A = SA
    pa = gu.gi.mlp_params(611, S, A)
    pq = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(611 + j, S + A, 1).items()}
    pq["network2.network.4.bias"] = pq["network2.network.4.bias"] - np.float32(shift)
    if qcut:
        pq["network1.network.4.bias"] = pq["network1.network.4.bias"] - np.float32(np.quantile(actor_reference(N, ma, shift, SA=SA)[2]["q"], qcut))
    enc, dec = BR.vae_params(VAE_SEED, "policy", S, A, ACTOR_H)
    s = gu.gi.batch(612, max(N, 64), S, A)[0][:N]
    eps = np.random.default_rng(N).standard_normal((N, ACTOR_N_SAMPLES, 2 * A)).astype(np.float32)
    return pa, pq, enc, dec, s, eps


@functools.lru_cache(maxsize=None)
def actor_reference(N, ma=1.0, shift=0.0, lamda=ACTOR_LAMDA, dtype=np.float64, qcut=0.0, SA=ACTOR_SA):
    """(logs, actor gradient as a parameter dict, extras) of tests/bosa2_ref.actor_step."""
    pa, pq, enc, dec, s, eps = actor_case(N, ma, shift, qcut, SA)
    return B2.actor_step(B2.twin_from_state_dict(pa, ("",)), B2.twin_from_state_dict(pq), enc, dec, s, eps, BETA, lamda, ma, dtype=dtype)


@functools.lru_cache(maxsize=None)
def actor_extra(N, ma=1.0, shift=0.0, lamda=ACTOR_LAMDA, qcut=0.0, SA=ACTOR_SA):
    """What the class hands the actor's backward: -(lamda / N) dll_da at pi, from the fp64 restatement, rounded to float32."""
    _, _, enc, dec, s, eps = actor_case(N, ma, shift, qcut, SA)
    pi = actor_reference(N, ma, shift, lamda, qcut=qcut, SA=SA)[2]["pi"]
    return (-(lamda / N) * B2.loglik_grad_action(enc, dec, s, pi, eps, BETA, ma)[0]).astype(np.float32)


# ---- where the GPU tests read intermediate values out of the workspaces ----------------------------------------------------------------
# Both workspaces hand out pieces rounded up to four floats.  tests/test_bosa_actor_ref.py ties these offsets to the library's own
# totals (mobody_bosa_workspace, mobody_train_workspace) on the CPU, at the shapes where the GPU tests read through them.
def _r4(v):
    return (v + 3) & ~3


def denc_offset(S, A, H, B, n):
    """Float offset of the encoder's seed [B][2 Lz] in the workspace: the pieces mobody_bosa_workspace hands out in front of it."""
    from mobody_amd import _lib
    Lz, nB = 2 * A, n * B
    enc, dec = _lib.wide_layout(S + A, H, 2 * Lz, 1), _lib.wide_layout(S + Lz, H, A, 1)
    return (_r4(B * enc.Kp1) + 2 * _r4(B * enc.Hp) + _r4(B * 2 * Lz) + _r4(nB * Lz) + _r4(nB * dec.Kp1) + 2 * _r4(nB * dec.Hp) + _r4(nB * A) +
            _r4(B * A) + _r4(B * Lz))


def pq_offset(S, A, H, B, n):
    """Float offset of the pairs pq [n B][2], the last piece of mobody_bosa_workspace's part: behind the encoder's seed, its backward
    scratch 2 [B][Hp] and the two per-workgroup partial-sum pieces."""
    from mobody_amd import _lib
    Lz = 2 * A
    Hp = _lib.wide_layout(S + A, H, 2 * Lz, 1).Hp
    return denc_offset(S, A, H, B, n) + _r4(B * 2 * Lz) + _r4(2 * B * Hp) + _r4(-(-B * Lz // 256)) + _r4(-(-B * A // 256))


def bosa_workspace_floats(S, A, H, B, n):
    """(mobody_bosa_workspace, mobody_bosa_loglik_grad_workspace) of the policy VAE in closed form: pq is the last piece of the first;
    behind it the seed [n B][A], dz [n B][Lz], the decoder's backward scratch 2 [n B][Hp] and two [B][A] pieces."""
    from mobody_amd import _lib
    Lz, nB = 2 * A, n * B
    base = pq_offset(S, A, H, B, n) + _r4(2 * nB)
    return base, base + _r4(nB * A) + _r4(nB * Lz) + _r4(2 * nB * _lib.wide_layout(S + Lz, H, A, 1).Hp) + 2 * _r4(B * A)


def dz3a_offset(S, A, N):
    """(float offset of the actor's seed dz3a [N][Np3] in the train workspace (N = Nt), Np3): the pieces mobody_train_workspace hands
    out in front of it (csrc/train.hip's carve)."""
    from mobody_amd import _lib
    Lq, La = _lib.mlp_layout(S + A, 1, 2), _lib.mlp_layout(S, A, 1)
    H, N32 = 256, (N + 31) & ~31
    mw = -(-N // 32) * H
    off = 2 * _r4(N * A) + 3 * _r4(2 * N) + _r4(N * Lq.Kp1) + _r4(2 * N32 * H) + _r4(2 * N * H) + _r4(N * La.Kp1) + _r4(N32 * H) + _r4(N * H)
    off += 2 * _r4(2 * mw) + 2 * _r4(mw) + _r4(2 * (N32 // 32)) + _r4(N32 // 32) + _r4(2 * (N32 // 32))
    return off + _r4(2 * N * Lq.Np3) + _r4(2 * N32 * H) + _r4(2 * N * H), La.Np3


def train_workspace_floats(S, A, N):
    """mobody_train_workspace (N = Nt) in closed form: dz3a and what carve hands out behind it -- dxa, the row weights, the loss
    partials, the bias partials per 32-row tile, the split-K slabs (tests/aux_ref.wgrad_nsplit), the bias corrections, the tickets
    and mode 9's pairs."""
    import aux_ref as R
    from mobody_amd import _lib
    Lq, La = _lib.mlp_layout(S + A, 1, 2), _lib.mlp_layout(S, A, 1)
    off, Np3 = dz3a_offset(S, A, N)
    H, tiles = 256, -(-N // 32)
    per_q, per_a = 2 * H + Lq.Np3, 2 * H + La.Np3
    slabs = max(_r4(Lq.total_floats) * R.wgrad_nsplit(N, 2), _r4(La.total_floats) * R.wgrad_nsplit(N, 1))
    return (off + _r4(N * Np3) + _r4(2 * N * A) + _r4(N) + _r4(2 * tiles) + _r4(tiles * max(2 * per_q, per_a)) + _r4(slabs) + 4 + _r4(tiles) +
            _r4(4 * tiles))


def pre_tanh_seed(ex, ma, dtype=np.float64):
    """d loss / d(pre-tanh) [N, A] per element, what the actor's backward is seeded with: dpi * max_action (1 - (pi / max_action)^2)."""
    ma = dtype(ma)
    return ex["dpi"] * ma * (1 - (ex["pi"] / ma) ** 2)


def seed_tolerance(d64):
    """Per element: rtol 1e-5 / atol 1e-5 x the largest entry."""
    return 1e-5 * np.abs(d64) + 1e-5 * np.abs(d64).max()


# ---- a stage-2 call of the class against g28 ---------------------------------------------------------------------------------------
def g28_setup(tag):
    """(g, cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed rows) as tests/test_bosa2_ref.py builds them."""
    g = gu.load("g28_bosa2_" + tag)
    S, A, H, E, bs = BR.VARIANTS[tag]
    seed, setting = int(g["seed"]), (float(g["log_std_bias"]), float(g["log_std_scale"]))
    cfg = BR.bosa_cfg(S, A, H, E, vae_iteration=0, epsilon_dyna_exp=float(g["epsilon_dyna_exp"]))
    vaes = BR.vae_params(seed, "policy", S, A, H, 1, *setting), BR.vae_params(seed + 50, "dynamics", S, A, H, E, *setting)
    actor_sd = gu.gi.mlp_params(seed + 1, S, A)
    q_sd = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(seed + 1 + j, S + A, 1).items()}
    src, tar = gu.gi.batch(501, 64, S, A), gu.gi.batch(502, 64, S, A)
    mixed = [np.concatenate([t_[:bs], s_[:bs]]) for s_, t_ in zip(src, tar)]
    mixed[4] = g["not_done"]
    return g, cfg, vaes, actor_sd, q_sd, mixed


def g28_noise(g, call):
    return {k: g["c%d_noise_%s" % (call, k)] for k in ("target", "dynamics", "policy") if "c%d_noise_%s" % (call, k) in g}


def scalar_terms(logs, cfg):
    """The sum of the magnitudes of the terms each logged scalar adds (its atol is 1e-5 x this), from the scalars themselves: a mean's
    magnitude stands in for the mean of magnitudes, which can only make the bound tighter."""
    coef, lam = cfg["conservation_coef"], cfg["lamda_policy"]
    t = dict(critic_mask_ratio=0.0, critic_cons_loss=abs(logs["critic_cons_loss"]))
    t["critic_loss"] = t["critic_td_loss"] = abs(logs["critic_td_loss"]) + coef * abs(logs["critic_cons_loss"])
    if "actor_loss" in logs:
        t.update(neg_log_beta_mean=abs(logs["neg_log_beta_mean"]), neg_log_beta_max=abs(logs["neg_log_beta_max"]), lamda_policy=0.0,
                 actor_loss=abs(logs["actor_loss"] - lam * logs["neg_log_beta_mean"]) + lam * abs(logs["neg_log_beta_mean"]))
    return t


# The product's batch (bs = 128: 256 mixed rows) at walker shapes, hidden 72, E = 2, two calls (the second an actor call).  Nothing of it
# comes from the real reference: the nets are gu.gi.mlp_params' / BR.vae_params', the noise a seeded NumPy generator's, and the
# expectation is the fp64 restatement alone.  g28 stays the tie to the reference.
BATCH_SHAPE, BATCH_SEED, BATCH_CALLS = (17, 6, 72, 2, 128), 952, (1, 2)


def batch_noise(call, cfg=None):
    """Raw normal draws of one call at BATCH_SHAPE by the class's kinds (target [N, A], dynamics_ll [n, E, N, 2 S], policy_ll
    [N, n, 2 A]), each from a generator seeded with (BATCH_SEED, call, kind index)."""
    S, A, _, E, bs = BATCH_SHAPE
    N, n = 2 * bs, (cfg or BR.bosa_cfg(*BATCH_SHAPE[:4]))["num_samples"]
    shapes = {"target": (N, A), "dynamics_ll": (n, E, N, 2 * S), "policy_ll": (N, n, 2 * A)}
    return {k: np.random.default_rng((BATCH_SEED, call, i)).standard_normal(shape).astype(np.float32) for i, (k, shape) in enumerate(shapes.items())}


@functools.lru_cache(maxsize=None)
def batch_setup():
    """(cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed rows, (gap, tolerance) of the mask threshold) at BATCH_SHAPE.  epsilon_dyna_exp is
    BR.mask_threshold's over both calls' pooled fp64 minima (the masks depend on the VAEs, the rows and the noise alone, not on the
    nets being trained), as tests/golden/make_golden_bosa2.py sets g28's."""
    S, A, H, E, bs = BATCH_SHAPE
    vaes = BR.vae_params(BATCH_SEED, "policy", S, A, H, 1), BR.vae_params(BATCH_SEED + 50, "dynamics", S, A, H, E)
    actor_sd = gu.gi.mlp_params(BATCH_SEED + 1, S, A)
    q_sd = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gu.gi.mlp_params(BATCH_SEED + 1 + j, S + A, 1).items()}
    src, tar = gu.gi.batch(501, bs, S, A), gu.gi.batch(502, bs, S, A)
    mixed = [np.concatenate([t_, s_]) for s_, t_ in zip(src, tar)]
    cfg = BR.bosa_cfg(S, A, H, E, vae_iteration=0)
    s, a, s2 = mixed[:3]
    lls = [BR.loglik(*vaes[1], "dynamics", s, a, s2, batch_noise(call, cfg)["dynamics_ll"], cfg["vae_dyna_beta"]) for call in BATCH_CALLS]
    ll = np.concatenate([x[0] for x in lls], 1)
    tol = np.concatenate([BR.estimator_tolerance(*x) for x in lls], 1)
    thr, gap, t = BR.mask_threshold(ll, tol)
    cfg["epsilon_dyna_exp"] = float(np.exp(thr))
    return cfg, vaes, actor_sd, q_sd, mixed, (gap, t)


def stage2_calls(tag, dtype=np.float64):
    """The four g28 calls composed from tests/bosa2_ref.py's pieces as stage2_call composes them; the state advances in fp64 and each
    call's scalars are evaluated in `dtype` on it.  Yields (call, logs in dtype, logs in fp64, state).  tag "batch": the two calls of
    BATCH_SHAPE in place of a fixture's."""
    if tag == "batch":
        cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed, _ = batch_setup()
        kinds = {"target": "target", "dynamics": "dynamics_ll", "policy": "policy_ll"}
        calls, noise_of = BATCH_CALLS, lambda call: {k: batch_noise(call, cfg)[v] for k, v in kinds.items()}
    else:
        g, cfg, (vae_pol, vae_dyn), actor_sd, q_sd, mixed = g28_setup(tag)
        calls, noise_of = (1, 2, 3, 4), lambda call: g28_noise(g, call)
    s, a, s2, r, nd = mixed
    st = B2.stage2_init(actor_sd, q_sd)
    ma = cfg["max_action"]
    for call in calls:
        noise = noise_of(call)
        st["total_it"] += 1
        tn = np.clip(np.asarray(noise["target"], np.float64) * cfg["expl_noise"], -cfg["noise_clip"], cfg["noise_clip"])
        mask, _ = B2.dyna_mask(*vae_dyn, s, a, s2, noise["dynamics"], cfg["vae_dyna_beta"], cfg["epsilon_dyna_exp"])
        st["mask"] = mask
        out = {}
        for dt in (dtype, np.float64):
            y, _ = B2.critic_targets(st["critic_target"], st["actor_target"], s2, r, nd, tn, cfg["gamma"], ma, dtype=dt)
            logs, _, gq = B2.critic_step(st["critic"], s, a, y, mask, cfg["conservation_coef"], dtype=dt)
            out[dt] = dict(logs, critic_mask_ratio=mask.mean())
        st["tq"] += 1
        for k in WR.KEYS:
            st["critic"][k], st["mq"][k], st["vq"][k] = WR.adam(st["critic"][k], gq[k], st["mq"][k], st["vq"][k], st["tq"], cfg["critic_lr"])
        if st["total_it"] % cfg["update_interval"] == 0:
            for dt in (dtype, np.float64):
                alog, ga, _ = B2.actor_step(st["actor"], st["critic"], *vae_pol, s, noise["policy"], cfg["vae_policy_beta"], cfg["lamda_policy"], ma,
                                            dtype=dt)
                out[dt].update(alog)
            st["ta"] += 1
            for k in WR.KEYS:
                st["actor"][k], st["ma"][k], st["va"][k] = WR.adam(st["actor"][k], ga[k], st["ma"][k], st["va"][k], st["ta"], cfg["actor_lr"])
            st["critic_target"] = B2.polyak(st["critic_target"], st["critic"], cfg["tau"])
            st["actor_target"] = B2.polyak(st["actor_target"], st["actor"], cfg["tau"])
        yield call, {k: float(v) for k, v in out[dtype].items()}, {k: float(v) for k, v in out[np.float64].items()}, st


@functools.lru_cache(maxsize=None)
def batch_reference():
    """([(call, fp64 scalars, mask [N])], the fp64 state after the last call) of the two calls at BATCH_SHAPE."""
    per_call = []
    for call, _, l64, st in stage2_calls("batch"):
        per_call.append((call, l64, st["mask"].copy()))
    return per_call, st
