"""Power-of-two scaling of the "f16x2" mode (csrc/tile_bf.h) against fp64 at adversarial magnitudes.

"f16x2" carries an fp32 operand as two fp16 terms: weight planes pre-scaled by 2^8 (F16_WSHIFT), activations / gradients
by one power of two per 32-row tile (f16_scale_exp), and the plane-fed weight-gradient GEMM brings the tiles of a wave's
row slice to one common exponent (mlp_bwd.hip wgrad_tile_f16).  Unit-scale data -- every other suite -- gives every tile
the same scale; here rows and tiles differ by up to 2^70, tiles are all zero or dead, rows are Inf / NaN and weights reach
255.  Every case runs in "f32" too: the same per-element bound (tests/f64_bounds.py) holding there shows it is sound.
Where the operands of one GEMM can be isolated (mlp3_forward(save=True) returns x, h1, h2) each layer is checked on the
kernel's own inputs, so a layer's error is not confused with its input's."""
import numpy as np
import pytest
import torch

import actor_ref as AR
import f64_bounds as fb
from f64_bounds import e2e_bound, grad_bounds, net_weights, robust_rows
import golden_util as gu
from oracle import mobody_oracle as O

pytestmark = pytest.mark.gpu
MODES = ["f32", "f16x2"]
S, A = 17, 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def q_params(seed, b1_mode):
    pq = {f"network{j}." + k: v for j in (1, 2) for k, v in gu.gi.mlp_params(seed + j, S + A, 1).items()}
    pa = {"network." + k: v for k, v in gu.gi.mlp_params(seed, S, A).items()}
    for p, pre in ((pq, "network1."), (pq, "network2."), (pa, "network.")):
        b = p[pre + "network.0.bias"]
        p[pre + "network.0.bias"] = np.zeros_like(b) if b1_mode == "zero" else -np.abs(b) if b1_mode == "neg" else b
    return pa, pq


def rows_pattern(name, rng):
    """(rows, per-row input scale, b1 mode): the row-magnitude patterns of the forward tests."""
    if name == "outlier":                     # one 2^20 row in a tile of unit rows
        f = np.ones(96); f[40] = 2.0 ** 20
        return 96, f, "zero"
    if name == "tile_scales":                 # one scale per tile, 2^-40 .. 2^30
        return 256, np.repeat(2.0 ** np.arange(-40, 31, 10), 32), "zero"
    if name == "zero_tile":                   # all-zero input tile, b1 <= 0: h1 of the tile is all zero (exponent 100)
        f = np.ones(96); f[32:64] = 0.0
        return 96, f, "neg"
    if name == "dead_tile":                   # layer 1 entirely dead on one tile: inputs far below |b1|, b1 < 0
        f = np.ones(96); f[32:64] = 2.0 ** -30
        return 96, f, "neg"
    rows = int(name.split("_")[1])            # ragged: the outlier in the partial last tile (padding rows hold act(b1))
    f = np.ones(rows); f[rows - 1] = 2.0 ** 20
    return rows, f, "keep"


FWD_PATTERNS = ["outlier", "tile_scales", "zero_tile", "dead_tile", "ragged_1", "ragged_31", "ragged_33", "ragged_65",
                "ragged_4097"]


@pytest.mark.parametrize("pattern", FWD_PATTERNS)
@pytest.mark.parametrize("mode", MODES)
def test_mlp3_forward_tile_patterns(mode, pattern, dev):
    from mobody_amd import ops, packing
    rng = np.random.default_rng(len(pattern))
    rows, f, b1m = rows_pattern(pattern, rng)
    pa, pq = q_params(301, b1m)
    s = (rng.standard_normal((rows, S)) * f[:, None]).astype(np.float32)
    a = (rng.uniform(-1, 1, (rows, A)) * f[:, None]).astype(np.float32)
    split = mode == "f16x2"
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."])
    ab = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
    kw_q, kw_a = gu.mlp_kw(qb, S + A, 1, 2, mode), gu.mlp_kw(ab, S, A, 1, mode)
    sd, ad = torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev)
    q, sx, h1, h2 = ops.mlp3_forward(qb, S + A, 1, 2, sd, ad, save=True, **kw_q)
    pi = ops.mlp3_forward(ab, S, A, 1, sd, out_mode=1, max_action=1.0, **kw_a)
    torch.cuda.synchronize()
    x = np.concatenate([s, a], 1)
    assert np.array_equal(fb.f64(sx)[:, :S + A], x)
    for m, pre in enumerate(("network1.", "network2.")):
        (W1, b1), (W2, b2), (W3, b3) = net_weights(pq, pre)
        z1, e1 = fb.layer_bound(x, W1, b1)                                 # layer 1: fp32 in both modes
        fb.check(h1[m], np.maximum(z1, 0), e1, f"{mode} {pattern} q{m} layer 1")
        z2, e2 = fb.layer_bound(h1[m], W2, b2, split=split, pad=np.maximum(b1, 0).max())
        fb.check(h2[m], np.maximum(z2, 0), e2, f"{mode} {pattern} q{m} layer 2")
        z3, e3 = fb.layer_bound(h2[m], W3, b3)
        fb.check(q[m], z3, e3, f"{mode} {pattern} q{m} layer 3")
    layers = net_weights(pa, "network.")
    z3, E = e2e_bound(s, layers, fb.C_E2E, split, np.maximum(layers[0][1], 0).max())
    fb.check(pi[0], np.tanh(z3), E, f"{mode} {pattern} actor")          # tanh is 1-Lipschitz


# ---- dynamics ensemble forward (Swish, 7 members) ------------------------------------------------------------------------
def dyn_params_nobias(seed, S_, A_):
    p = gu.gi.dyn_params(seed, S_, A_)
    for k in p:
        if k.endswith(".bias") and k.split(".")[0] in ("zs1", "zs2", "zs3", "za_trg1", "za_trg2", "transition1", "transition2"):
            p[k] = np.zeros_like(p[k])               # biases would mask the row magnitudes of the input
    return p


def dyn_bound(p, obs, act, c, split):
    """fp64 mean of dyn_forward (use_trg) and a propagated per-element bound (Swish is 1.1-Lipschitz; its fast evaluation
    adds c |y|).  Split layers: zs2, transition2 (tiles of up to 64 rows)."""
    def net(h, E, names):
        for li, nm in enumerate(names):
            W, b = p[nm + ".weight"].astype(np.float64), p[nm + ".bias"].astype(np.float64)
            z, bnd = fb.layer_bound(h, W, b, c, split=split and nm in ("zs2", "transition2"), tb=64)
            E = (fb.SWISH_LIP * E) @ np.abs(W) + bnd if not np.isscalar(E) else bnd
            if li < len(names) - 1:
                with np.errstate(over="ignore"):              # exp(-z) = Inf: swish(z) = -0
                    h = z / (1 + np.exp(-z))
                E = E + c * np.abs(h)
            else:
                h = z
        return h, E
    zs, Ezs = net(obs, 0.0, ("zs1", "zs2", "zs3"))
    zs, Ezs = zs[..., :16], Ezs[..., :16]
    x = np.concatenate([zs, np.broadcast_to(act, zs.shape[:-1] + (act.shape[-1],))], -1)
    Ex = np.concatenate([Ezs, np.zeros(zs.shape[:-1] + (act.shape[-1],))], -1)
    g, Eg = net(x, 0.0, ("za_trg1", "za_trg2"))
    W1 = p["za_trg1.weight"].astype(np.float64)
    Eg = Eg + fb.SWISH_LIP ** 2 * (Ex @ np.abs(W1)) @ np.abs(p["za_trg2.weight"].astype(np.float64))
    z, Ez = zs + g[..., :16], Ezs + Eg[..., :16]
    t = z
    Et = Ez
    for li, nm in enumerate(("transition1", "transition2", "transition3")):
        W, b = p[nm + ".weight"].astype(np.float64), p[nm + ".bias"].astype(np.float64)
        zz, bnd = fb.layer_bound(t, W, b, c, split=split and nm == "transition2", tb=64)
        Et = fb.SWISH_LIP * Et @ np.abs(W) + bnd
        if li < 2:
            with np.errstate(over="ignore"):
                t = zz / (1 + np.exp(-zz))
            Et = Et + c * np.abs(t)
        else:
            t = zz
    return t, Et


DYN_PATTERNS = ["outlier", "tile_scales", "zero_tile", "ragged_65"]


@pytest.mark.parametrize("pattern", DYN_PATTERNS)
@pytest.mark.parametrize("tag,S_,A_", [("walker", 17, 6), ("ant", 111, 8)])
@pytest.mark.parametrize("mode", MODES)
def test_dyn_forward_tile_patterns(mode, tag, S_, A_, pattern, dev):
    from mobody_amd import ops, packing
    rng = np.random.default_rng(7 + len(pattern))
    rows, f, _ = rows_pattern(pattern, rng)
    if pattern == "tile_scales":
        f = np.repeat(2.0 ** np.arange(-40, 21, 20), 32); rows = f.size    # Swish of 2^30-scale inputs overflows exp()
    p = dyn_params_nobias(31, S_, A_)
    obs = (rng.standard_normal((rows, S_)) * f[:, None]).astype(np.float32)
    act = rng.uniform(-1, 1, (rows, A_)).astype(np.float32)
    blob = packing.pack_dynamics(p, S_, A_, dev)
    kw = gu.dyn_kw(blob, S_, A_, mode)
    got = ops.dyn_forward(blob, S_, A_, torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), True, **kw)
    ref, E = dyn_bound(p, obs.astype(np.float64), act.astype(np.float64), fb.C_E2E, mode == "f16x2")
    with torch.no_grad():                                   # the bound's forward is the oracle's fp64 restatement
        o64 = O.dyn_forward(O.to_torch(p), obs, act, True, dtype=torch.float64)[0].numpy()
    np.testing.assert_allclose(ref, o64, rtol=1e-9, atol=1e-9 * np.abs(o64).max())
    fb.check(got, o64, E, f"{mode} {tag} {pattern} dyn_forward")


# ---- non-finite rows (defect 2) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("mode", MODES)
def test_nonfinite_row_stays_in_its_row(mode, bad, dev):
    """One +Inf / NaN input row in a tile of 1e-3, 1 and 1e3 (.. 1e5) rows: every other row meets its bound and stays finite
    (the tile maximum runs over finite magnitudes only).  Nothing is asserted about the bad row itself."""
    from mobody_amd import ops, packing
    rng = np.random.default_rng(3)
    rows, badrow = 96, 40
    f = np.ones(rows); f[32:64:4] = 1e-3; f[33:64:4] = 1e3; f[34:64:8] = 1e5
    s = (rng.standard_normal((rows, S)) * f[:, None]).astype(np.float32)
    a = rng.uniform(-1, 1, (rows, A)).astype(np.float32)
    s[badrow, 0] = bad                                       # one coordinate: W1 x is +-Inf (or NaN), not Inf - Inf
    ok = np.arange(rows) != badrow
    pa, pq = q_params(311, "keep")
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."])
    q, sx, h1, h2 = ops.mlp3_forward(qb, S + A, 1, 2, torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), save=True,
                                     **gu.mlp_kw(qb, S + A, 1, 2, mode))
    for m, pre in enumerate(("network1.", "network2.")):
        (W1, b1), (W2, b2), (W3, b3) = net_weights(pq, pre)
        assert np.isfinite(fb.f64(h2[m])[ok]).all() and np.isfinite(fb.f64(q[m])[ok]).all()
        hh1, hh2 = fb.f64(h1[m]), fb.f64(h2[m])
        hh1[~ok] = 0.0; hh2[~ok] = 0.0                       # tile maxima of the good rows only: the bad row must not enter them
        z2, e2 = fb.layer_bound(hh1, W2, b2, split=mode == "f16x2")
        fb.check(hh2[ok], np.maximum(z2, 0)[ok], e2[ok], f"{mode} {bad} q{m} layer 2")
        z3, e3 = fb.layer_bound(hh2, W3, b3)
        fb.check(fb.f64(q[m])[ok], z3[ok], e3[ok], f"{mode} {bad} q{m} layer 3")
    p = dyn_params_nobias(33, S, A)
    blob = packing.pack_dynamics(p, S, A, dev)
    got = fb.f64(ops.dyn_forward(blob, S, A, torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), True,
                                 **gu.dyn_kw(blob, S, A, mode)))[:, ok]
    assert np.isfinite(got).all()
    s0 = s.astype(np.float64); s0[~ok] = 0.0
    ref, E = dyn_bound(p, s0, a.astype(np.float64), fb.C_E2E, mode == "f16x2")
    fb.check(got, ref[:, ok], E[:, ok], f"{mode} {bad} dyn_forward")


# ---- weight range (defect 3) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_weights_up_to_255_meet_the_forward_bound(mode, dev):
    from mobody_amd import ops, packing
    rng = np.random.default_rng(5)
    pa, pq = q_params(321, "keep")
    for pre in ("network1.", "network2."):
        mag = 2.0 ** rng.uniform(-12, np.log2(255.0), (256, 256))
        pq[pre + "network.2.weight"] = (mag * rng.choice([-1.0, 1.0], (256, 256))).astype(np.float32)
    pq["network1.network.2.weight"][3, 5] = 255.0
    rows = 96
    s = rng.standard_normal((rows, S)).astype(np.float32); a = rng.uniform(-1, 1, (rows, A)).astype(np.float32)
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."])
    q, sx, h1, h2 = ops.mlp3_forward(qb, S + A, 1, 2, torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), save=True,
                                     **gu.mlp_kw(qb, S + A, 1, 2, mode))
    for m, pre in enumerate(("network1.", "network2.")):
        (W1, b1), (W2, b2), _ = net_weights(pq, pre)
        z2, e2 = fb.layer_bound(h1[m], W2, b2, split=mode == "f16x2")
        fb.check(h2[m], np.maximum(z2, 0), e2, f"{mode} wide-range W2 q{m}")


def test_plane_builders_refuse_weights_fp16_cannot_hold(dev):
    """|W2| = 300 >= 65504 / 2^8: every f16x2 plane builder raises instead of returning Inf planes; the other modes build."""
    from mobody_amd import ops, packing
    pa, pq = q_params(331, "keep")
    pq["network2.network.2.weight"][17, 200] = -300.0
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."])
    with pytest.raises(ValueError):
        ops.mlp_transpose(qb, S + A, 1, 2, precision="f16x2")
    ops.mlp_transpose(qb, S + A, 1, 2, precision="bf16x3")
    p = gu.gi.dyn_params(9, S, A)
    for nm in ("zs2", "transition2", "reward_model2"):
        q = {k: v.copy() for k, v in p.items()}
        q[nm + ".weight"][6, 100, 3] = 300.0
        blob = packing.pack_dynamics(q, S, A, dev)
        with pytest.raises(ValueError):
            ops.dyn_planes(blob, S, A, precision="f16x2")
        ops.dyn_planes(blob, S, A, precision="bf16x3")
        pb = packing.pack_pretrain(q, S, A, dev)
        with pytest.raises(ValueError):
            ops.pretrain_transpose(pb, S, A, precision="f16x2")
        ops.pretrain_transpose(pb, S, A, precision="f32")
    pm = gu.gi.dyn_params(9, S, A, mopo=True)
    for nm in ("za_src2", "reward_model2"):
        q = {k: v.copy() for k, v in pm.items()}
        q[nm + ".weight"][0, 1, 2] = -300.0
        blob = packing.pack_pretrain_mopo({k: torch.from_numpy(v) for k, v in q.items()}, S, A, dev)
        with pytest.raises(ValueError):
            ops.pretrain_mopo_transpose(blob, S, A, precision="f16x2")
        ops.pretrain_mopo_transpose(blob, S, A, precision="f32")
    # just below the limit: builds
    pq["network2.network.2.weight"][17, 200] = -255.5
    ops.mlp_transpose(packing.pack_mlp(pq, S + A, 1, dev, prefixes=["network1.", "network2."]), S + A, 1, 2, precision="f16x2")


# ---- critic / actor gradients of Engine.step -----------------------------------------------------------------------------
def engine_grads_check(mode, pa, pq, batch, n_true, dev):
    from mobody_amd.engine import Engine
    cfg = gu.policy_cfg(S, A, mfma=mode)
    eng = Engine(S, A, pa, pq, dev)
    eng.step(batch, n_true, cfg, apply=False)
    st = O.TrainState(pa, pq)
    with O.linear_tape() as tape:
        want = O.train_step(st, batch, n_true, cfg, apply=False, dtype=torch.float64)
    tape["_W"] = {k: fb.f64(v) for k, v in {**O.to_torch(pq), **O.to_torch(pa)}.items()}
    split = mode == "f16x2"
    got_q = eng.unpack(eng.gq, "q")
    # the forward error in dz3 = 2 (q - y) / N: E_q of q(s, a), and E_y of y = r + gamma nd min q'(s2, pi(s2))
    s, a, s2 = (x.astype(np.float64) for x in batch[:3])
    N = len(s)
    la = net_weights(pa, "network.")
    pi2, Epi2 = e2e_bound(s2, la, fb.C_E2E, split, np.maximum(la[0][1], 0).max())
    pi2 = np.tanh(pi2)
    Ey = 0.0
    for pre in ("network1.", "network2."):
        lq = net_weights(pq, pre)
        E0 = np.concatenate([np.zeros_like(s2), Epi2], 1)
        Ey = np.maximum(Ey, e2e_bound(np.concatenate([s2, pi2], 1), lq, fb.C_E2E, split, np.maximum(lq[0][1], 0).max(), E0=E0)[1])
    Ey = cfg["gamma"] * batch[4].astype(np.float64) * Ey
    Ey = Ey + 2.0 ** -22 * (np.abs(batch[3]) + np.abs(fb.f64(want["td_target"])))   # fp32 rounding of y and of q - y
    for pre in ("network1.", "network2."):
        lq = net_weights(pq, pre)
        Eq = e2e_bound(np.concatenate([s, a], 1), lq, fb.C_E2E, split, np.maximum(lq[0][1], 0).max())[1]
        (W1, b1), (W2, b2), _ = lq
        z1, e1 = fb.layer_bound(np.concatenate([s, a], 1), W1, b1, fb.C_E2E)
        _, e2 = fb.layer_bound(np.maximum(z1, 0), W2, b2, fb.C_E2E, split=split, pad=np.maximum(b1, 0).max())
        bd = grad_bounds(tape, fb.C_E2E, split, pre, edz3=2.0 / N * (Eq + Ey), ex={2: e1, 4: e1 @ np.abs(W2) + e2})
        for k, v in bd.items():
            fb.check(got_q[k], want["q_grads"][k], v, f"{mode} critic {k}")
    # the actor half: eng.ga against the same fp64 step with the derived bound of tests/actor_ref.py (apply=False: the critic the
    # actor phase sees is the one the step started with)
    h = dict(cfg, advantage=0)
    fw = AR.forward_ref(pa, pq, batch[0], batch[1], n_true, cfg["max_action"])
    cf = AR.closed_forms(fw["pi"], fw["qp"], fw["qb"], fw["dqda"], batch[1], h, N, n_true, N, n_true)
    ref_a, tape_a = AR.actor_grads_ref(pa, batch[0], fw, cf["dz3"])
    bd = AR.actor_bounds(pa, pq, batch[0], batch[1], h, N, n_true, N, n_true, fw, cf, tape_a, split)
    got_a = eng.unpack(eng.ga, "actor")
    for k, v in want["actor_grads"].items():
        np.testing.assert_allclose(ref_a[k], fb.f64(v), rtol=1e-9, atol=1e-9 * np.abs(fb.f64(v)).max(), err_msg=k)   # one reference
        fb.check(got_a[k], v, bd["grads"][k], f"{mode} actor {k}")
    return got_q, want


def build_batch(rng, pa, pq, N, modify):
    """N rows of gi.batch-like data, `modify(s, a)` applied, with ReLU-fragile rows replaced from a larger pool."""
    s, a, s2, r, nd = gu.gi.batch(int(rng.integers(1 << 30)), 4 * N, S, A)
    s, a = modify(s, a)
    keep = np.flatnonzero(robust_rows(pa, pq, s, a))
    return s, a, s2, r, nd, keep


@pytest.mark.parametrize("case", ["unit", "reward_outlier"])
@pytest.mark.parametrize("mode", MODES)
def test_engine_grads_vs_fp64(mode, case, dev):
    """Critic gradients per element against the fp64 train_step.  reward_outlier: one 32-row tile of 1e8 rewards
    shares each wave's 64-row slice of the critic's weight-gradient job (256 rows: rows_per_wave 64) with a unit tile,
    which then sits more than 2^24 below it."""
    rng = np.random.default_rng(11)
    pa, pq = q_params(341, "keep")
    N, n_true = 256, 128
    s, a, s2, r, nd, keep = build_batch(rng, pa, pq, N, lambda s, a: (s, a))
    assert keep.size >= N
    idx = keep[:N]
    batch = [x[idx].copy() for x in (s, a, s2, r, nd)]
    if case == "reward_outlier":
        batch[3][0:32] = 1e8
    engine_grads_check(mode, pa, pq, tuple(batch), n_true, dev)


@pytest.mark.parametrize("mode", MODES)
def test_wgrad_drops_tiles_far_below_their_slice(mode, dev):
    """Dead-column probe.  b1 = 0, and a few Q layer-1 features are -c e0 (active only where s0 < 0).  s0 > 0 on every row
    but those of one tile, whose (s, a) are 2^-36-scale with s0 < 0: rows k of dW2 (columns of the nn.Linear layout) come
    from that tile alone, which shares its wave slice with a unit tile far above it.  Dropping it is within the bound;
    amplifying it -- a scale factor clamped to 2^-24 -- is not."""
    rng = np.random.default_rng(12)
    pa, pq = q_params(351, "zero")
    dead = [3, 77, 200]
    for pre in ("network1.", "network2."):
        W1 = pq[pre + "network.0.weight"]
        W1[dead] = 0.0
        W1[dead, 0] = -1.0
    N, n_true, tiny = 256, 128, slice(32, 64)

    def normal(s, a):
        s = s.copy(); s[:, 0] = np.abs(s[:, 0]) + 0.1
        return s, a

    def small(s, a):
        s = s.copy(); s[:, 0] = -(np.abs(s[:, 0]) + 0.1)
        return (s * 2.0 ** -36).astype(np.float32), (a * 2.0 ** -36).astype(np.float32)
    s, a, s2, r, nd, keep = build_batch(rng, pa, pq, N, normal)
    t = build_batch(rng, pa, pq, N, small)
    idx = keep[:N]
    batch = [x[idx].copy() for x in (s, a, s2, r, nd)]
    batch[0][tiny], batch[1][tiny] = t[0][t[5][:32]], t[1][t[5][:32]]
    got_q, want = engine_grads_check(mode, pa, pq, tuple(batch), n_true, dev)
    for pre in ("network1.", "network2."):
        k = pre + "network.2.weight"
        g, ref = fb.f64(got_q[k]), fb.f64(want["q_grads"][k])
        assert (np.abs(ref[:, dead]) > 0).sum() > 100             # the probe reaches those columns
        lim = 2 * np.abs(ref[:, dead]) + 2.0 ** -30 * np.abs(ref).max()
        assert (np.abs(g[:, dead]) <= lim).all(), (mode, k, float((np.abs(g[:, dead]) / lim).max()))


# ---- dynamics pre-training gradients ---------------------------------------------------------------------------------------
def pretrain_bounds(tape, c, split, nets):
    out = {}
    for names in nets:
        for li, nm in enumerate(names):
            recs = tape.get(nm, [])
            if not recs:
                continue
            dz = lambda r: np.abs(fb.f64(r["dz"])) if "dz" in r else 0.0 * np.abs(fb.f64(r["z"]))
            gW = sum(np.swapaxes(np.abs(fb.f64(r["x"])), -1, -2) @ dz(r) for r in recs)
            gb = sum(dz(r).sum(-2, keepdims=True) for r in recs)
            if li < len(names) - 1 and len(tape.get(names[li + 1], [])) == len(recs):
                W = np.abs(fb.f64(tape["_W"][names[li + 1] + ".weight"]))
                for r, rn in zip(recs, tape[names[li + 1]]):
                    z = fb.f64(r["z"])
                    prop = (dz(rn) @ np.swapaxes(W, -1, -2)) * fb.SWISH_LIP
                    gW = gW + np.swapaxes(np.abs(fb.f64(r["x"])), -1, -2) @ prop
                    gb = gb + prop.sum(-2, keepdims=True)
            bW, bb = c * gW, c * gb
            if split and nm in ("zs2", "transition2", "reward_model2"):   # every call's rows in one contraction
                xs = [np.broadcast_to(fb.f64(r["x"]), dz(r).shape[:-1] + (r["x"].shape[-1],)) for r in recs]
                bW = bW + fb.wgrad_floor(np.concatenate(xs, -2), np.concatenate([dz(r) for r in recs], -2))
            out[nm + ".weight"], out[nm + ".bias"] = bW, bb
    return out


@pytest.mark.parametrize("case", ["unit", "residual_tile"])
@pytest.mark.parametrize("mode", MODES)
def test_pretrain_grads_vs_fp64(mode, case, dev):
    """pretrain_grads per element against the fp64 dyn_learn_step.  residual_tile: the rewards are 2^30 x larger on every
    row but one 32-row tile, whose reward residuals -- and, through the fake next state, the transition net's gradients --
    are then ~2^-30 of the others' (the tile drops out of its slice).  (Scaling next_state instead overflows the
    encoder's exp(logvar) long before 2^30.)"""
    from test_hip_pretrain import Trainer, noise7
    b = 96
    p = gu.gi.dyn_params(55, S, A)
    rows = list(gu.gi.pretrain_batch(57, b, S, A))
    if case == "residual_tile":
        big = np.full((1, b, 1), 2.0 ** 30); big[:, 32:64] = 1.0
        rows[3] = (rows[3] * big).astype(np.float32)
    nz = noise7(np.random.default_rng(58), b, S)
    tr = Trainer(p, S, A, b, dev, prec=mode)
    for use_trg in (False, True):
        tr.grad.zero_()
        tr.grads(rows, nz, use_trg)
        got = tr.unpack(tr.grad)
        st = O.DynTrainState(p)
        with O.linear_tape() as tape:
            want = O.dyn_learn_step(st, *rows, nz, use_trg, apply=False, dtype=torch.float64)
        tape["_W"] = {k: v for k, v in p.items()}
        pre = "za_trg" if use_trg else "za_src"
        bd = pretrain_bounds(tape, fb.C_E2E, mode == "f16x2",
                             [("zs1", "zs2", "zs3"), (pre + "1", pre + "2"), ("transition1", "transition2", "transition3"),
                              ("reward_model1", "reward_model2", "reward_model3")])
        for k, v in want["grads"].items():
            if v is None or k not in bd or k.startswith("za_"):
                continue                                   # (za_*2 holds only its mu half in the blob)
            fb.check(got[k], v, bd[k], f"{mode} {case} trg={use_trg} {k}")
