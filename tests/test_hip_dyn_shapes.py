"""The dynamics kernels over the (S, A) edges of mobody_dyn_layout (tests/dyn_shapes.py lists them and says which branch, pad
width or row packing each one reaches) against fp64: the forward chain k_dyn_fwd in its K-split and generic heads, the sample /
penalty kernel k_dyn_sample at every rows-per-workgroup packing, the reward head at its widest inputs, validate(), and one
pre-training step of the latent model and of the MOPO ablation.  Every other GPU test of these kernels runs at the four shapes
of the D4RL fixtures.

Tolerances are the project's own, none is fitted to these shapes:
  forward, exact fp32      max|hip - f64| <= 3 max|torch fp32 - f64| + 1e-6 max|f64|   (test_mopo_grads_vs_fp64_restatement's form)
  forward, f16x2 / bf16x3  1e-5 max|f64|                                               (tests/test_hip_precision.py TOL)
  step                     1e-5 absolute + relative, on the kernel's own means         (test_hip_uncertainty.py / _dynamics.py)
  validate()               rtol 1e-5, atol 1e-7                                        (test_dyn_validate_vs_oracle)
  pre-training             losses rtol 2e-5 / atol 1e-6, gradients 1e-5 |g| + 1e-5 max|g| of the sub-network
                           (test_pretrain_grads_vs_oracle_shapes); the mopo step 3 x the fp32 restatement + 1e-6 max|g|
Each test prints its worst error / bound ratio next to the fp32 restatement's own (lines starting with RATIO; DESIGN.md holds
the table measured with them)."""
import numpy as np
import pytest
import torch

import dyn_shapes as D
import golden_util as gu
from test_hip_pretrain import Trainer
from test_hip_uncertainty import _positional_dyn_step, same_bits
from test_pretrain_mopo_fixture import TRAINED as MOPO_TRAINED

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)
shapes = lambda cases: pytest.mark.parametrize("shape", cases, ids=D.ident)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def report(test, shape, mode, hip, ref):
    print("RATIO %s %s %s hip %.4f ref %.4f" % (test, D.ident(shape), mode, hip, ref))


def latent_model(S, A, dev, mode):
    """(inference blob, planes= / precision= keywords of mode `mode`) of the latent model at dyn_shapes.params(S, A)."""
    from mobody_amd import packing
    blob = packing.pack_dynamics(D.params(S, A), S, A, dev)
    return blob, gu.dyn_kw(blob, S, A, mode)


def mopo_model(S, A, dev, mode):
    """(inference blob, keywords with mopo=(blob, T blob)) of the MOPO ablation at dyn_shapes.params(S, A, mopo=True)."""
    from mobody_amd import ops, packing
    p = D.params(S, A, True)
    blob = packing.pack_dynamics(D.mopo_inference_params(p, A), S, A, dev)
    g = lambda k: torch.as_tensor(p[k], dtype=torch.float32).to(dev)
    mlp = packing.pack_mlp(packing._ens_members(g, ("za_src1", "za_src2", "za_src3")), S + A, S, dev)
    kw = gu.dyn_kw(blob, S, A, mode)
    kw["mopo"] = (mlp, ops.mlp_transpose(mlp, S + A, S, 7, precision=mode))
    return blob, kw


# --------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("mode", ["f32", "f16x2", "bf16x3"])
@shapes(D.SHAPES)
def test_forward_vs_fp64(shape, mode, dev):
    from mobody_amd import ops
    S, A = shape
    blob, kw = latent_model(S, A, dev, mode)
    worst = ref = 0.0
    for B in (1, 71):
        obs, act, _, _ = D.step_inputs(S, A, B)
        o, a = torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev)
        for use_trg in (True, False):
            want, t32 = D.forward_ref(S, A, B, use_trg)
            got = ops.dyn_forward(blob, S, A, o, a, use_trg, **kw)
            again = ops.dyn_forward(blob, S, A, o, a, use_trg, **kw)
            assert got.shape == (7, B, S) and same_bits(got, again), (B, use_trg)
            bound = D.forward_bound(want, t32, mode)
            err = float(np.abs(f64(got) - want).max())
            worst, ref = max(worst, err / bound), max(ref, float(np.abs(t32 - want).max()) / bound)
            print("forward", shape, mode, B, use_trg, "err %.3e bound %.3e" % (err, bound))
            assert err <= bound, (B, use_trg, err, bound)
    report("forward", shape, mode, worst, ref)


# --------------------------------------------------------------------------------------------------------- 2. / 3. step
def check_step(shape, mfma, dev, mopo):
    from mobody_amd import ops
    S, A = shape
    blob, kw = (mopo_model if mopo else latent_model)(S, A, dev, mfma)
    p = D.params(S, A, mopo)
    worst = ref = 0.0
    for B in (1, 71):
        obs, act, eps, idx = D.step_inputs(S, A, B)
        o, a = torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev)
        run = lambda unc, up, task=1: ops.dyn_step(blob, S, A, task, o, a, noise=eps, elite_idx=idx, penalty_coef=D.COEF,
                                                   use_penalty=up, want_mean=True, uncertainty_mode=unc, **kw)
        m64, t32 = D.forward_ref(S, A, B, True, mopo)
        first = None
        for unc in D.ALL_MODES:
            for up in (True, False):
                r = run(unc, up)
                mean, nxt = f64(r["mean"]), r["next_obs"].cpu().numpy()
                assert np.abs(mean - m64).max() <= D.forward_bound(m64, t32, mfma), (B, unc)
                for dtype in (np.float64, np.float32):            # fp64: the check; fp32: the restatement's own distance from it
                    w = D.step_ref(p, obs, act, mean, eps, idx, nxt, unc, dtype)
                    if dtype == np.float64:
                        want = w
                    else:
                        ref = max(ref, max(D.ratio(w[k], want[k], 1e-5, 1e-5) for k in want))
                worst = max(worst, max(D.ratio(f64(r[k]), want[k], 1e-5, 1e-5) for k in want))
                for k in want:
                    np.testing.assert_allclose(f64(r[k]), want[k], err_msg=str((B, unc, up, k)), **TOL)
                raw = f64(r["raw_reward"])
                if up:                                             # reward = raw - coef * penalty (mobody_dynamics.py:261-263)
                    np.testing.assert_allclose(f64(r["reward"]), raw - D.COEF * want["penalty"], err_msg=str((B, unc)), **TOL)
                else:
                    assert same_bits(r["reward"], r["raw_reward"]), (B, unc)
                # the predicate on the kernel's own rows: exact, no row is excused for sitting near a threshold
                assert np.array_equal(r["terminal"].cpu().numpy().astype(bool), D.O.termination("halfcheetah", None, None, nxt)), (B, unc)
                if first is None:
                    first = r
                else:                                              # the mode and the penalty flag change penalty / reward only
                    for k in ("next_obs", "terminal", "raw_reward", "mean"):
                        assert same_bits(r[k], first[k]), (B, unc, up, k)
        for name, task in D.tasks_for(S, A)[1:]:
            r = run("pairwise-diff", True, task)
            assert same_bits(r["next_obs"], first["next_obs"]) and same_bits(r["penalty"], first["penalty"]), (B, name)
            done = D.O.termination(name, None, None, r["next_obs"].cpu().numpy())
            assert np.array_equal(r["terminal"].cpu().numpy().astype(bool), done), (B, name)
            if B == 71 and name in ("walker2d", "pen"):
                assert 0 < int(done.sum()) < B, name                # both outcomes are in the batch
        if not mopo:                                               # mode 0 of mobody_ens_step == the positional mobody_dyn_step
            old = _positional_dyn_step(blob, S, A, 1, o, a, eps, idx, kw)
            for k in old:
                assert same_bits(old[k], first[k]), (B, k)
    report("mopo_step" if mopo else "step", shape, mfma, worst, ref)


@shapes(D.SHAPES)
def test_step_vs_fp64_on_the_kernels_own_means(shape, mfma, dev):
    check_step(shape, mfma, dev, mopo=False)


@shapes(D.MOPO_SHAPES)
def test_mopo_step_vs_fp64_on_the_kernels_own_means(shape, mfma, dev):
    check_step(shape, mfma, dev, mopo=True)


@shapes(D.RNG_SHAPES)
def test_step_device_rng_equals_the_explicit_form(shape, mfma, dev):
    """noise=None / elite_idx=None: the draws made inside k_dyn_sample are those of the stand-alone generator at the same
    (seed, call) -- element b * S + d of the noise stream, element b of the elite stream -- bit for bit."""
    from mobody_amd import ops
    S, A = shape
    B, elites, seed, call = 71, (1, 2, 4, 5, 6), 42, 3
    blob, kw = latent_model(S, A, dev, mfma)
    obs, act, _, _ = D.step_inputs(S, A, B)
    o, a = torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev)
    got = ops.dyn_step(blob, S, A, 4, o, a, elites=elites, seed=seed, call=call, penalty_coef=D.COEF, want_mean=True, **kw)
    z = ops.rng_normal(seed, 1, call, B * S, dev).reshape(1, B, S).expand(7, B, S).contiguous()
    idx = torch.as_tensor(elites, device=dev)[ops.rng_index(seed, 2, call, B, len(elites), dev).long()]
    assert set(idx.tolist()) <= set(elites) and len(set(idx.tolist())) > 1
    want = ops.dyn_step(blob, S, A, 4, o, a, noise=z, elite_idx=idx, penalty_coef=D.COEF, want_mean=True, **kw)
    for k in want:
        assert same_bits(got[k], want[k]), k


# --------------------------------------------------------------------------------------------------------- 4. validate()
@shapes(D.VALIDATE_SHAPES)
def test_validate_vs_fp64(shape, dev):
    from mobody_amd import ops, packing
    S, A = shape
    blob = packing.pack_dynamics(D.params(S, A), S, A, dev)
    mblob, mkw = mopo_model(S, A, dev, "f32")
    td = lambda x: torch.from_numpy(x).to(dev)
    for B in (71, 300):
        s, a, s2, r = (td(x) for x in D.validate_inputs(S, A, B))
        runs = [(ops.dyn_validate(blob, S, A, s, a, s2, r, use_trg), D.validate_ref(S, A, B, use_trg), ("latent", use_trg))
                for use_trg in (True, False)]
        runs.append((ops.dyn_validate_mopo(mblob, mkw["mopo"][0], S, A, s, a, s2, r), D.validate_ref(S, A, B, True, True), "mopo"))
        for out, (tl, rl), what in runs:
            out = f64(out)
            np.testing.assert_allclose(out[:7], tl, rtol=1e-5, atol=1e-7, err_msg=str((B, what, "transition")))
            np.testing.assert_allclose(out[7:], rl, rtol=1e-5, atol=1e-7, err_msg=str((B, what, "reward")))


# --------------------------------------------------------------------------------------------------------- 5. pre-training
@shapes(D.PRETRAIN_CASES)
def test_pretrain_grads_vs_fp64(shape, mfma, dev):
    S, A, b = shape
    tr = Trainer(D.params(S, A), S, A, b, dev, prec=mfma)
    rows, nz = D.pretrain_inputs(S, A, b)
    worst, ref = [0.0, 0.0], [0.0, 0.0]
    for use_trg in (False, True):
        w64, w32 = D.pretrain_ref(S, A, b, use_trg)
        tr.grad.zero_()
        losses = tr.grads(rows, nz, use_trg)
        got = {k: f64(v) for k, v in tr.unpack(tr.grad).items()}
        rg, rl = D.pretrain_grad_ratios(got, w64["grads"]), D.ratio(losses, w64["losses"], 2e-5, 1e-6)
        g32 = {k: v for k, v in w32["grads"].items() if v is not None}
        worst = [max(worst[0], max(rg.values())), max(worst[1], rl)]
        ref = [max(ref[0], max(D.pretrain_grad_ratios(g32, w64["grads"]).values())), max(ref[1], D.ratio(w32["losses"], w64["losses"], 2e-5, 1e-6))]
        print("pretrain", shape, mfma, use_trg, "loss ratio %.4f" % rl, {k: round(v, 4) for k, v in rg.items() if v > 0.25})
        np.testing.assert_allclose(losses, w64["losses"], rtol=2e-5, atol=1e-6, err_msg=str(use_trg))
        other = "za_src" if use_trg else "za_trg"
        for k, v in w64["grads"].items():
            if v is None:
                assert k.startswith(other) and float(np.abs(got[k]).max()) == 0.0, k    # the other domain's action encoder
            else:
                assert rg[k] <= 1.0, (use_trg, k, rg[k])
    report("pretrain_grads", shape, mfma, worst[0], ref[0])
    report("pretrain_losses", shape, mfma, worst[1], ref[1])


def mopo_trainer(S, A, b, dev, mfma):
    from mobody_amd import ops, packing
    p = D.params(S, A, True)
    blob = packing.pack_pretrain_mopo({k: torch.from_numpy(p[k]) for k in MOPO_TRAINED}, S, A, dev)
    return blob, ops.pretrain_mopo_transpose(blob, S, A, precision=mfma), ops.pretrain_mopo_workspace(S, A, b, dev)


@shapes(D.MOPO_PRETRAIN_CASES)
def test_pretrain_mopo_grads_vs_fp64(shape, mfma, dev):
    from mobody_amd import ops, packing
    S, A, b = shape
    blob, blob_T, ws = mopo_trainer(S, A, b, dev, mfma)
    (s, a, s2, r), eps = D.mopo_pretrain_inputs(S, A, b)
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    grad, loss = torch.zeros_like(blob), torch.zeros(5, device=dev)
    worst = ref = 0.0
    for use_trg in (False, True):
        (l64, g64), (l32, g32) = D.mopo_pretrain_ref(S, A, b, use_trg)
        grad.zero_()
        ops.pretrain_mopo_grads(S, A, b, use_trg, 1.0, blob, blob_T, td(np.concatenate([s, s2], 1)), td(a), td(r[..., 0]), grad, loss,
                                ws, noise=td(eps), precision=mfma)
        got = packing.unpack_pretrain_mopo(grad, S, A)
        np.testing.assert_allclose(f64(loss)[[0, 1, 2, 4]], np.array(l64), rtol=2e-5, atol=1e-7, err_msg=str(use_trg))
        for k in MOPO_TRAINED:
            e_hip, e_t32 = np.abs(f64(got[k]) - g64[k]).max(), np.abs(g32[k].astype(np.float64) - g64[k]).max()
            bound = 3 * e_t32 + 1e-6 * np.abs(g64[k]).max() + 1e-12
            worst, ref = max(worst, e_hip / bound), max(ref, e_t32 / bound)
            assert e_hip <= bound, (k, use_trg, e_hip, e_t32)
    report("pretrain_mopo_grads", shape, mfma, worst, ref)


# --------------------------------------------------------------------------------------------------------- 6. padding
def _pad_is_zero(t, real, what):
    pad = t.cpu()[~real]
    assert pad.numel() == 0 or float(pad.abs().max()) == 0.0, (what, int((pad != 0).sum()), int((~real).sum()))


@shapes(D.PAD_SHAPES)
def test_padding_stays_padding(shape, mfma, dev):
    """The floats of the training blobs no parameter lives in -- K / N pad of every layer, alignment gaps -- carry a gradient of
    exactly 0.0, and stay 0.0 in the weights and in both Adam moments over three fused updates that alternate the domains.  A
    pad weight that drifts corrupts later steps without showing in the unpacked tensors every other test compares."""
    from mobody_amd import _lib, ops, packing
    S, A = shape
    b = 9
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    # the inference blob: the real floats are the inference halves of the 13 layers, the rest is zero as packed
    L = _lib.dyn_layout(S, A)
    real = packing.pack_dynamics(D.ones_like_params(D.params(S, A)), S, A, "cpu") != 0
    assert int(real.sum()) == 7 * sum((l.in_dim + 1) * l.out_dim for l in L.layer) < L.total_floats
    _pad_is_zero(packing.pack_dynamics(D.params(S, A), S, A, dev), real, "inference blob")
    # latent model
    p = D.params(S, A)
    real = packing.pack_pretrain(D.ones_like_params(p), S, A, "cpu") != 0
    assert 0 < int((~real).sum())
    tr = Trainer(p, S, A, b, dev, prec=mfma)
    rows, nz = D.pretrain_inputs(S, A, b)
    for use_trg in (False, True):
        tr.grad.zero_()
        tr.grads(rows, nz, use_trg)
        assert float(tr.grad.abs().max()) > 0.0
        _pad_is_zero(tr.grad, real, ("grad", use_trg))
    (s, a, s2, r) = rows
    xenc, act, rew = td(np.concatenate([s, s2], 1)), td(a), td(r[..., 0])
    n6, n7 = td(np.stack(nz[:6])), td(nz[6])
    start = tr.blob.clone()
    t_za = {False: 0, True: 0}
    for t, use_trg in enumerate((False, True, False), 1):
        t_za[use_trg] += 1
        ops.pretrain_update(S, A, b, use_trg, 1.0, tr.blob, tr.blob_T, xenc, act, rew, tr.m, tr.v, t, t_za[use_trg], 1e-3, tr.loss,
                            tr.ws, noise6=n6, noise7=n7, precision=mfma)
    assert not torch.equal(tr.blob, start)
    for name, t in (("blob", tr.blob), ("m", tr.m), ("v", tr.v)):
        _pad_is_zero(t, real, name)
    # MOPO ablation
    pm = D.params(S, A, True)
    real = packing.pack_pretrain_mopo({k: torch.ones(pm[k].shape) for k in MOPO_TRAINED}, S, A, "cpu") != 0
    blob, blob_T, ws = mopo_trainer(S, A, b, dev, mfma)
    (s, a, s2, r), eps = D.mopo_pretrain_inputs(S, A, b)
    xenc, act, rew, eps = td(np.concatenate([s, s2], 1)), td(a), td(r[..., 0]), td(eps)
    grad, m, v, loss = torch.zeros_like(blob), torch.zeros_like(blob), torch.zeros_like(blob), torch.zeros(5, device=dev)
    for use_trg in (False, True):
        grad.zero_()
        ops.pretrain_mopo_grads(S, A, b, use_trg, 1.0, blob, blob_T, xenc, act, rew, grad, loss, ws, noise=eps, precision=mfma)
        assert float(grad.abs().max()) > 0.0
        _pad_is_zero(grad, real, ("mopo grad", use_trg))
    start = blob.clone()
    for t, use_trg in enumerate((False, True, False), 1):
        ops.pretrain_mopo_update(S, A, b, use_trg, 1.0, blob, blob_T, xenc, act, rew, m, v, t, 1e-3, loss, ws, noise=eps, precision=mfma)
    assert not torch.equal(blob, start)
    for name, t in (("mopo blob", blob), ("mopo m", m), ("mopo v", v)):
        _pad_is_zero(t, real, name)
