"""The "bf16x3" kernels (csrc/tile_bf.h, wgrad_tile_bf of csrc/mlp_bwd.hip) against fp64, per element.

"bf16x3" is where a run ends up once a weight has left the range of the "f16x2" planes (config['f16_guard'] = 'fallback'), so it
is held to what tests/test_hip_f16_scaling.py holds "f16x2" to, and run at the weights that cause the move: |W2| >= 255.875.
Every case runs in "f32" too (the control: the same bound holding there shows it is sound).  The bound of one GEMM is
c = C_BF16X3 (tests/f64_bounds.py) with split=False -- bf16 keeps fp32's exponent range: no tile scale, no subnormal floor, no
dropped tile; tests/test_bf16x3_ref.py shows on the CPU that a product without one of its term pairs misses that bound on the
"coherent" pattern below.  The cases of test_hip_f16_scaling.py are run through that file's own functions; the row geometry of the
bf16 weight-gradient job is compared bit for bit with the integer closed form of tests/test_hip_twinq_rank1.py.

Each test prints its worst err / bound (DESIGN.md keeps the figures of the commit that added this file)."""
import numpy as np
import pytest
import torch

import bf16x3_ref as B
import f64_bounds as fb
import golden_util as gu
import test_hip_f16_scaling as F16
from f64_bounds import e2e_bound, net_weights

pytestmark = pytest.mark.gpu
MODES = ["f32", "bf16x3"]
S, A = B.S, B.A
Q_PRE = ("network1.", "network2.")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def checked(monkeypatch, request):
    """fb.check, recording what it was given: the worst err / bound of the test is printed when the test ends, and a test can
    look at the bound an element was held to."""
    seen, check = {}, fb.check

    def recording(got, ref, bound, what):
        check(got, ref, bound, what)
        g, r, b = fb.f64(got), fb.f64(ref), np.broadcast_to(fb.f64(bound), np.shape(ref))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(b > 0, np.abs(g - r) / b, 0.0)              # (b == 0 passed the check: the error is 0 there)
        seen[what] = dict(got=g, ref=r, bound=b, ratio=float(np.max(ratio, initial=0.0)))
    monkeypatch.setattr(fb, "check", recording)
    yield seen
    if seen:
        w = max(seen, key=lambda k: seen[k]["ratio"])
        print(f"\n{request.node.name}: worst err / bound = {seen[w]['ratio']:.3g} ({w}; {len(seen)} tensors)")


# ---- a. forward, layer by layer on the kernel's own inputs ------------------------------------------------------------------
@pytest.mark.parametrize("pattern", F16.FWD_PATTERNS + ["coherent"])
@pytest.mark.parametrize("mode", MODES)
def test_mlp3_forward_layers_vs_fp64(mode, pattern, dev):
    from mobody_amd import ops, packing
    pa, pq, s, a = B.forward_case(pattern)
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=list(Q_PRE))
    ab = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
    sd, ad = torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev)
    q, sx, h1, h2 = ops.mlp3_forward(qb, S + A, 1, 2, sd, ad, save=True, **gu.mlp_kw(qb, S + A, 1, 2, mode))
    pi = ops.mlp3_forward(ab, S, A, 1, sd, out_mode=1, max_action=1.0, **gu.mlp_kw(ab, S, A, 1, mode))
    torch.cuda.synchronize()
    x = np.concatenate([s, a], 1)
    assert np.array_equal(fb.f64(sx)[:, :S + A], x)
    for m, pre in enumerate(Q_PRE):
        (W1, b1), (W2, b2), (W3, b3) = net_weights(pq, pre)
        z1, e1 = fb.layer_bound(x, W1, b1)                                 # layer 1: fp32 in both modes
        fb.check(h1[m], np.maximum(z1, 0), e1, f"{mode} {pattern} q{m} layer 1")
        z2, e2 = fb.layer_bound(h1[m], W2, b2, fb.C_BF16X3, split=False)
        fb.check(h2[m], np.maximum(z2, 0), e2, f"{mode} {pattern} q{m} layer 2")
        z3, e3 = fb.layer_bound(h2[m], W3, b3)
        fb.check(q[m], z3, e3, f"{mode} {pattern} q{m} layer 3")
        if pattern == "coherent":                                          # the selection layer: h1 is the input, exactly
            assert np.array_equal(fb.f64(h1[m]), np.maximum(z1, 0)) and (fb.f64(h2[m]) > 0).all()
    layers = net_weights(pa, "network.")
    z3, E = e2e_bound(s, layers, fb.C_E2E, False, 0.0)
    fb.check(pi[0], np.tanh(z3), E, f"{mode} {pattern} actor")             # tanh is 1-Lipschitz


@pytest.mark.parametrize("pattern", F16.DYN_PATTERNS)
@pytest.mark.parametrize("tag,S_,A_", [("walker", 17, 6), ("pen", 45, 24)])
@pytest.mark.parametrize("mode", MODES)
def test_dyn_forward_tile_patterns(mode, tag, S_, A_, pattern, dev):
    """The dynamics ensemble's forward on the patterns and against the reference of test_hip_f16_scaling.py (dyn_bound with
    split=False here); pen has the wide transition head."""
    F16.test_dyn_forward_tile_patterns(mode, tag, S_, A_, pattern, dev)


@pytest.mark.parametrize("bad", [np.inf, np.nan])
@pytest.mark.parametrize("mode", MODES)
def test_nonfinite_row_stays_in_its_row(mode, bad, dev):
    F16.test_nonfinite_row_stays_in_its_row(mode, bad, dev)


# ---- b. past the f16 range ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_case():
    """Twin-Q with W2 of 2^-12 .. 2^12 and the planted 255.875 .. -65536, and N rows whose ReLU masks and min(q0, q1) branch the
    kernels' error cannot flip -- judged by the fp64 reference alone, for THESE weights, before the GPU is touched."""
    N = 256
    pa, pq = B.wide_q_params()
    for pre in Q_PRE:
        for (n, v), k in zip(B.PLANTED, B.planted_inputs(pq, pre)):
            assert pq[pre + "network.2.weight"][n, k] == np.float32(v) and abs(v) >= 255.875
    rng = np.random.default_rng(21)
    pool = 4
    while True:
        s, a, s2, r, nd = gu.gi.batch(int(rng.integers(1 << 30)), pool * N, S, A)
        keep = np.flatnonzero(fb.robust_rows(pa, pq, s, a))
        if keep.size >= N or pool >= 64:
            break
        pool *= 2                                                          # enlarge the pool, never the criterion
    assert keep.size >= N, f"{keep.size} robust rows of {pool * N}"
    return pa, pq, tuple(x[keep[:N]].copy() for x in (s, a, s2, r, nd))


@pytest.mark.parametrize("mode", MODES)
def test_weights_past_the_f16_range_meet_the_forward_bound(mode, wide_case, dev):
    from mobody_amd import ops, packing
    pa, pq, batch = wide_case
    s, a = batch[0][:96], batch[1][:96]
    qb = packing.pack_mlp(pq, S + A, 1, dev, prefixes=list(Q_PRE))
    with pytest.raises(ValueError):
        ops.mlp_transpose(qb, S + A, 1, 2, precision="f16x2")               # these are the weights f16x2 cannot hold
    q, sx, h1, h2 = ops.mlp3_forward(qb, S + A, 1, 2, torch.from_numpy(s).to(dev), torch.from_numpy(a).to(dev), save=True,
                                     **gu.mlp_kw(qb, S + A, 1, 2, mode))
    for m, pre in enumerate(Q_PRE):
        (W1, b1), (W2, b2), (W3, b3) = net_weights(pq, pre)
        assert np.isfinite(fb.f64(h2[m])).all()
        z2, e2 = fb.layer_bound(h1[m], W2, b2, fb.C_BF16X3, split=False)
        fb.check(h2[m], np.maximum(z2, 0), e2, f"{mode} wide-range W2 q{m} layer 2")
        for k in B.planted_inputs(pq, pre):                                # the planted weights take part: their inputs are live
            assert (fb.f64(h1[m])[:, k] > 0).any(), (m, k)
        z3, e3 = fb.layer_bound(h2[m], W3, b3)
        fb.check(q[m], z3, e3, f"{mode} wide-range W2 q{m} layer 3")


@pytest.mark.parametrize("mode", MODES)
def test_engine_grads_past_the_f16_range_vs_fp64(mode, wide_case, dev):
    """Critic and actor gradients of Engine.step against the fp64 train_step with the wide-range twin-Q."""
    pa, pq, batch = wide_case
    F16.engine_grads_check(mode, pa, pq, batch, 128, dev)


@pytest.mark.parametrize("mode", MODES)
def test_dyn_forward_past_the_f16_range(mode, dev):
    """zs2 and transition2 of member 3 scaled like the twin-Q's W2 above; the planes are built by dyn_planes(precision=...)."""
    from mobody_amd import ops, packing
    rng = np.random.default_rng(23)
    p = F16.dyn_params_nobias(31, S, A)
    for nm in ("zs2", "transition2"):
        p[nm + ".weight"][3] = B.wide_w2(rng).T                             # EnsembleLinear layout [member][in][out]
    rows = 96
    obs = rng.standard_normal((rows, S)).astype(np.float32)
    act = rng.uniform(-1, 1, (rows, A)).astype(np.float32)
    blob = packing.pack_dynamics(p, S, A, dev)
    with pytest.raises(ValueError):
        ops.dyn_planes(blob, S, A, precision="f16x2")
    kw = {} if mode == "f32" else dict(planes=ops.dyn_planes(blob, S, A, precision="bf16x3"), precision="bf16x3")
    got = ops.dyn_forward(blob, S, A, torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), True, **kw)
    ref, E = F16.dyn_bound(p, obs.astype(np.float64), act.astype(np.float64), fb.C_E2E, False)
    assert np.isfinite(ref).all() and np.isfinite(fb.f64(got)).all()
    assert np.abs(ref[3]).max() > 2.0 ** 8 * np.abs(np.delete(ref, 3, 0)).max()          # the scaled member is the scaled member
    fb.check(got, ref, E, f"{mode} wide-range dyn_forward")


# ---- c. gradients at adversarial tile magnitudes -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["unit", "reward_outlier"])
@pytest.mark.parametrize("mode", MODES)
def test_engine_grads_vs_fp64(mode, case, dev):
    F16.test_engine_grads_vs_fp64(mode, case, dev)


@pytest.mark.parametrize("mode", MODES)
def test_wgrad_keeps_a_tile_far_below_its_slice(mode, checked, monkeypatch, dev):
    """The dead-column probe of test_wgrad_drops_tiles_far_below_their_slice: three columns of dW2 (nn.Linear layout) come from
    one 2^-36-scale tile alone.  "f16x2" may drop that tile; here nothing is dropped, so those columns must come out to their
    own relative accuracy, not merely within 2 |ref|.  The probe as it stands cannot show that: its general bound charges these
    columns the layer-1 forward error c |x| |W1| of h1 at the unit scale of the rows outside the tile (2^22 |ref|), and with
    unit rewards the forward error of q - y is a third of q - y itself.  So the probe runs a second time on the same rows with
      * every reward at 1e4: q - y is -1e4 on every row, known to ~2^-15, and dz2 has one sign per column -- no cancellation;
      * the bound formed again with ex[2] = 0 on the three columns: that layer-1 unit is -1 * s0 with no bias, exact in fp32, and
        exactly 0 behind the ReLU outside the tile.  What is left is c |dz2|^T |h1| and the error of dz2 times |h1|.
    That bound is below 2^-12 |ref| element by element (asserted first, from the reference alone; the CPU gives 2^-14.2)."""
    dead, own, runs = [3, 77, 200], {}, []
    grad_bounds, engine_grads_check = F16.grad_bounds, F16.engine_grads_check

    def also_with_exact_dead_inputs(tape, c, split, which, edz3=None, ex=None):
        e = np.array(ex[2]); e[:, dead] = 0.0
        own[which] = grad_bounds(tape, c, split, which, edz3=edz3, ex={**ex, 2: e})
        return grad_bounds(tape, c, split, which, edz3=edz3, ex=ex)

    def twice(mode_, pa, pq, batch, n_true, dev_):
        out = engine_grads_check(mode_, pa, pq, batch, n_true, dev_)                # the probe as it stands
        runs.append(dict(checked))
        engine_grads_check(mode_, pa, pq, batch[:3] + (np.full_like(batch[3], 1e4),) + batch[4:], n_true, dev_)
        return out
    monkeypatch.setattr(F16, "grad_bounds", also_with_exact_dead_inputs)
    monkeypatch.setattr(F16, "engine_grads_check", twice)
    F16.test_wgrad_drops_tiles_far_below_their_slice(mode, dev)
    assert len(runs) == 1
    for pre in Q_PRE:
        k = pre + "network.2.weight"
        c = checked[f"{mode} critic {k}"]                                           # the second run's
        assert not np.array_equal(c["ref"], runs[0][f"{mode} critic {k}"]["ref"])
        got, ref, bd = c["got"][:, dead], c["ref"][:, dead], own[pre][k][:, dead]
        live = np.abs(ref) > 0
        assert live.sum() > 100
        assert (bd[live] <= 2.0 ** -12 * np.abs(ref[live])).all() and np.abs(ref).max() < 2.0 ** -30 * np.abs(c["ref"]).max()
        fb.check(got, ref, bd, f"{mode} {pre} dW2 columns of the 2^-36 tile")
        print(f"{mode} {pre}: the tile's columns, worst |err| / |ref| = 2^{np.log2(max((np.abs(got - ref)[live] / np.abs(ref[live])).max(), 2.0 ** -60)):.1f}")


def test_pretraining_has_no_bf16x3_form(dev):
    """The two cases of test_pretrain_grads_vs_fp64 are left out: pre-training runs in 'f32' or 'f16x2' only (the dynamics object
    turns 'fallback' into 'raise' for that reason), and every entry point refuses 'bf16x3' by name."""
    from mobody_amd import _lib, ops, packing
    pb = packing.pack_pretrain(gu.gi.dyn_params(55, S, A), S, A, dev)
    with pytest.raises((_lib.MobodyError, ValueError), match="precision"):
        ops.pretrain_transpose(pb, S, A, precision="bf16x3")


# ---- d. row geometry of the bf16 weight-gradient job, bit for bit ------------------------------------------------------------
@pytest.mark.parametrize("N", B.WGRAD_ROWS)
def test_critic_integer_exact_at_every_row_geometry(N, dev):
    """k_wgrad_bf<3> has a row loop and a masked tail of its own: 16-row blocks, the tail's rows 8 h + j < tail.  N = 1 .. 33 puts
    a partial 8-row half, a partial block and a last wave of depth - 1, depth and depth + 1 rows in front of that tail; 257 ..
    1025 several waves and workgroups.  Integer nets and batch: with the preconditions of tests/test_bf16x3_ref.py (asserted
    first) every kernel result is determined to the bit."""
    from test_hip_twinq_rank1 import int_critic_case, run_critic, same_bits
    c = int_critic_case((S, A), N)
    B.assert_critic_case_exact(c, f"N{N}")
    grad, g, loss, _ = run_critic(c["pa"], c["pq"], c["batch"], S, A, N, c["Ng"], "bf16x3", dev)
    for m in range(2):
        for k, v in c["out"][m]["grads"].items():
            same_bits(g[m][k], v, f"N{N} bf16x3 member {m} {k}")
    same_bits([loss], [c["loss"]], "q_loss")
