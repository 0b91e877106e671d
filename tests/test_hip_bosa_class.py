"""GPU checks of the BOSA mirror class (algo/offline_offline/bosa.py): train() in the VAE stage against the fp64
restatement, graph replay against eager steps bit for bit, checkpoints, the refusal at the stage boundary, the estimators' front
ends, and the CLI.  Tolerances as tests/test_hip_bosa.py: losses rtol 1e-5, parameters params_close at the VAE's lr."""
import json
import os

import numpy as np
import pytest
import torch

import bosa_ref as BR
import wide_ref as WR
from test_bosa_ref import bosa_config
from test_hip_train import params_close

pytestmark = pytest.mark.gpu
S, A = 17, 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make(dev, **over):
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.bosa import BOSA
    torch.manual_seed(5)
    pol = call_algo("bosa", bosa_config(**over), 3, dev)
    assert isinstance(pol, BOSA)
    return pol


def load_scaled(pol, seed=21):
    """The restatement's 1 / sqrt(fan_in) weights (EnsembleFC's unit-variance ones saturate the clamp); returns them."""
    out = []
    for vae in (pol.vae_policy, pol.vae_dyna):
        enc, dec = BR.vae_params(seed, vae.kind, S, A, vae.hidden, vae.ensemble_size)
        vae.load_state_dict({k: torch.from_numpy(x) for k, x in BR.state_dict(enc, dec, vae.kind).items()})
        out.append((enc, dec))
    return out


def buffers(dev, rows=64, rng="numpy", seed=0):
    from mobody_amd.algo import utils
    out = []
    for k in (1, 2):
        r = np.random.default_rng(seed + k)
        rb = utils.ReplayBuffer(S, A, dev, max_size=rows, rng=rng, seed=seed + k)
        rb.convert_D4RL(dict(observations=r.standard_normal((rows, S)).astype(np.float32), actions=np.tanh(r.standard_normal((rows, A))).astype(np.float32),
                             next_observations=r.standard_normal((rows, S)).astype(np.float32), rewards=r.standard_normal(rows).astype(np.float32),
                             terminals=np.zeros(rows, np.float32)))
        out.append(rb)
    return out


def state(pol):
    return [t.clone() for t in (pol.vae_policy.blob, pol.vae_dyna.blob, pol.vae_policy_optimizer.m, pol.vae_policy_optimizer.v,
                                pol.vae_dyna_optimizer.m, pol.vae_dyna_optimizer.v)]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_train_vs_fp64_with_the_reference_draw_order(dev):
    """Three train() calls: rows [tar | src] with src drawn first from NumPy's generator, recorded noise, both VAEs."""
    bs = 8
    pol = make(dev, vae_iteration=7, vae_dyna_ensemble=2)
    (penc, pdec), (denc, ddec) = load_scaled(pol)
    src, tar = buffers(dev)
    rows = lambda rb: tuple(getattr(rb, f)[:rb.size].cpu().numpy() for f in ("state", "action", "next_state"))
    noise = []
    rng = np.random.default_rng(3)
    pol.noise_fn = lambda kind, shape: (noise.append((kind, rng.standard_normal(shape).astype(np.float32))), noise[-1][1])[1]
    nets = {"policy": [WR.f64(penc), WR.f64(pdec)], "dynamics": [WR.f64(denc), WR.f64(ddec)]}
    mom = {k: [[{q: 0.0 for q in WR.KEYS} for _ in range(2)] for _ in range(2)] for k in nets}
    np.random.seed(11)
    want_idx = np.random.RandomState(11)
    seen = []

    class W:
        def add_scalar(self, k, v, step):
            seen.append((k, v, step))
    for call in (1, 2, 3):
        i_src, i_tar = want_idx.randint(0, 64, size=bs), want_idx.randint(0, 64, size=bs)
        pol.train(src, tar, bs, W(), None)
        assert pol.total_it == 2 * call and not seen
        b = tuple(np.concatenate([t[i_tar], s[i_src]]) for s, t in zip(rows(src), rows(tar)))
        got = pol._loss.cpu().numpy()
        for j, kind in enumerate(("policy", "dynamics")):
            k2, eps = noise[2 * (call - 1) + j]
            assert k2 == kind
            enc, dec = nets[kind]
            losses, grads, _ = BR.vae_step(enc, dec, kind, *b, eps, 0.5, 1.0)
            np.testing.assert_allclose(got[3 * j:3 * j + 3], losses, rtol=1e-5)
            for p, g, (m, v) in zip((enc, dec), grads, zip(*mom[kind])):
                for q in WR.KEYS:
                    p[q], m[q], v[q] = WR.adam(p[q], g[q], m[q], v[q], call, 1e-3)
    from mobody_amd import packing
    for vae, kind in ((pol.vae_policy, "policy"), (pol.vae_dyna, "dynamics")):
        ein, Lz, din, dout = BR.dims(kind, S, A)
        E = vae.ensemble_size
        for blob, (i, o), p in ((vae.blob[:vae.n_enc], (ein, 2 * Lz), nets[kind][0]), (vae.blob[vae.n_enc:], (din, dout), nets[kind][1])):
            for q, t in zip(WR.KEYS, packing.unpack_wide(blob.cpu(), i, vae.hidden, o, E)):
                params_close(t.numpy(), p[q], 1e-3)
    assert pol.vae_policy_optimizer.t == pol.vae_dyna_optimizer.t == 3
    # call 4 would enter the critic / actor stage: refused, nothing moves
    before, draws = state(pol), (np.random.get_state()[2], len(noise))
    with pytest.raises(NotImplementedError, match="critic / actor stage is not built"):
        pol.train(src, tar, bs, None, None)
    assert pol.total_it == 6 and same_bits(before, state(pol)) and (np.random.get_state()[2], len(noise)) == draws


def test_logging_step_writes_the_six_scalars(dev):
    pol = make(dev, vae_iteration=20000)
    load_scaled(pol)
    src, tar = buffers(dev, rng="device")
    seen = []

    class W:
        def add_scalar(self, k, v, step):
            seen.append((k, v, step))
    pol.total_it = 4998
    pol.train(src, tar, 8, W(), None)
    from mobody_amd.algo.offline_offline.bosa import LOG_KEYS
    assert [k for k, _, _ in seen] == ["train/" + k for k in LOG_KEYS] and {s for _, _, s in seen} == {5000}
    assert all(np.isfinite(v) for _, v, _ in seen)
    # a short buffer: total_it counts once and nothing else happens
    before = state(pol)
    pol.train(src, tar, 65, W(), None)
    assert pol.total_it == 5001 and same_bits(before, state(pol)) and len(seen) == 6


def test_graph_replay_equals_eager_steps_bit_for_bit_and_checkpoints_resume(dev, tmp_path):
    steps, bs = 6, 8
    runs = []
    for graph in (0, 1):
        pol = make(dev, vae_iteration=1000, rng="device", seed=3, graph=graph)
        load_scaled(pol)
        src, tar = buffers(dev, rng="device", seed=9)
        for _ in range(steps):
            pol.train(src, tar, bs, None, None)
        torch.cuda.synchronize()
        assert (pol._graph is not None) == bool(graph)
        runs.append((pol, src, tar))
    (e, es, et), (g, gs, gt) = runs
    assert same_bits(state(e), state(g)), "graph replay and eager steps differ"
    assert same_bits([e._loss], [g._loss])
    for a, b in ((e, g), (es, gs), (et, gt)):
        for f in ("total_it", "_noise_calls", "_draws"):
            assert getattr(a, f, None) == getattr(b, f, None), f
    assert e.total_it == 2 * steps and e.vae_policy_optimizer.t == g.vae_policy_optimizer.t == steps == g.vae_dyna_optimizer.t
    assert g._ctr.tolist() == [steps - 1, steps, steps]          # the first call ran eagerly (it allocates the batch)
    # save -> load into a fresh object -> one more step == the uninterrupted run
    prefix = str(tmp_path / "model")
    g.save(prefix)
    assert sorted(os.listdir(tmp_path)) == ["model_vae_dynamics", "model_vae_dynamics_optimizer", "model_vae_policy", "model_vae_policy_optimizer"]
    sd = torch.load(prefix + "_vae_policy_optimizer", weights_only=True)
    assert sorted(sd["state"]) == list(range(14)) and float(sd["state"][0]["step"]) == steps and sd["param_groups"][0]["lr"] == 1e-3
    assert list(torch.load(prefix + "_vae_dynamics", weights_only=True)) == [k + s for k in ("encoder_shared.0", "encoder_shared.2", "mean", "log_std",
                                                                                              "decoder.0", "decoder.2", "decoder.4") for s in (".W", ".b")]
    fresh = make(dev, vae_iteration=1000, rng="device", seed=3, graph=0)
    fresh.load(prefix)
    assert same_bits(state(fresh), state(g))
    fresh.total_it, fresh._noise_calls = g.total_it, g._noise_calls
    fs, ft = buffers(dev, rng="device", seed=9)
    fs._draws, ft._draws = gs._draws, gt._draws
    fresh.train(fs, ft, bs, None, None)
    g.train(gs, gt, bs, None, None)
    e.train(es, et, bs, None, None)
    torch.cuda.synchronize()
    assert same_bits(state(fresh), state(g)) and same_bits(state(e), state(g))


def test_estimator_front_ends(dev):
    pol = make(dev, vae_dyna_ensemble=3, num_samples=4, epsilon_dyna_exp=0.01)
    (penc, pdec), (denc, ddec) = load_scaled(pol)
    r = np.random.default_rng(1)
    B = 10
    s, a, s2 = (r.standard_normal((B, S)).astype(np.float32), np.tanh(r.standard_normal((B, A))).astype(np.float32),
                r.standard_normal((B, S)).astype(np.float32))
    noise = {}
    pol.noise_fn = lambda kind, shape: noise.setdefault(kind, np.random.default_rng(2).standard_normal(shape).astype(np.float32))
    ll = pol.policy_log_likelihood(s, a)
    assert ll.shape == (B,) and noise["policy_ll"].shape == (B, 4, 2 * A)
    want = BR.loglik(penc, pdec, "policy", s, a, s2, noise["policy_ll"], 0.5)
    np.testing.assert_allclose(ll.cpu().numpy(), want[0][0], rtol=1e-5, atol=1e-5 * np.abs(want[1]).max())
    lld = pol.dyna_log_likelihood(s, a, s2)
    assert lld.shape == (3, B) and noise["dynamics_ll"].shape == (4, 3, B, 2 * S)
    want = BR.loglik(denc, ddec, "dynamics", s, a, s2, noise["dynamics_ll"], 0.5)
    np.testing.assert_allclose(lld.cpu().numpy(), want[0], rtol=1e-5, atol=1e-5 * np.abs(want[1]).max())
    mask, ratio = pol.dyna_mask(s, a, s2)
    assert mask.shape == (B,) and torch.equal(mask, (lld.min(0)[0] > np.log(0.01)).float()) and float(ratio) == float(mask.mean())
    assert pol.policy_log_likelihood(s, a, num_samples=1).shape == (B,)
    with pytest.raises(ValueError, match="num_samples"):
        pol.policy_log_likelihood(s, a, num_samples=65)
    act = pol.select_action(s[0])
    assert act.shape == (A,) and np.abs(act).max() <= 1.0


def config_tree(tmp_path, **over):
    import yaml
    d = tmp_path / "config" / "mujoco" / "bosa"
    os.makedirs(d, exist_ok=True)
    c = bosa_config(eval_freq=3, **over)
    for k in ("state_dim", "action_dim", "max_action"):
        del c[k]
    with open(d / "walker2d.yaml", "w") as f:
        yaml.safe_dump(c, f)
    return str(tmp_path / "config")


def test_cli_runs_the_vae_stage_and_refuses_one_more_step(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.bosa import BOSA, vae_steps
    built = []
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: built.append("build_dynamics"))
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path, vae_iteration=13, batch_size=16))
    out_dir = tmp_path / "out"
    argv = ["--policy", "BOSA", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", "1",
            "--rng", "device", "--src_rows", "300", "--tar_rows", "200", "--save-model", "--eval_freq", "3", "--log_every", "2",
            "--dir", str(out_dir), "--params", json.dumps(dict(graph=1))]
    n = vae_steps(13)
    pol = tm.main(argv + ["--max_step", str(n)])
    assert n == 6 and isinstance(pol, BOSA) and pol.total_it == 12 and pol.dynamics is None and built == [] and pol._graph is not None
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3 and all("VAE_Policy/vae_loss" in ln and "VAE_Dynamics/KL_loss" in ln and "q_loss" not in ln for ln in lines)
    files = [f for _, _, fs in os.walk(out_dir) for f in fs if f.startswith("model_")]
    assert sorted(files) == ["model_vae_dynamics", "model_vae_dynamics_optimizer", "model_vae_policy", "model_vae_policy_optimizer"]
    with pytest.raises(SystemExit, match="the largest max_step is 6"):
        tm.main(argv + ["--max_step", str(n + 1)])


@pytest.mark.parametrize("tag", list(BR.VARIANTS))
def test_mirror_train_vs_reference_fixture(dev, tag):
    """The class's train() on the fixture's fixed rows and recorded noise: losses, parameters and total_it of the real reference."""
    from test_bosa_ref import load_fixture, sub
    from test_hip_iql import FixedRows
    from mobody_amd.algo.call_algo import call_algo
    g, nets, mixed, (rows_src, rows_tar) = load_fixture(tag)
    S_, A_, H, E, bs = BR.VARIANTS[tag]
    pol = call_algo("bosa", BR.bosa_cfg(S_, A_, H, E, vae_iteration=7), 3, dev)
    for vae, kind in ((pol.vae_policy, "policy"), (pol.vae_dyna, "dynamics")):
        vae.load_state_dict({k: torch.from_numpy(x) for k, x in BR.state_dict(*nets[kind], kind).items()})
    src, tar = FixedRows(rows_src, S_, A_, dev), FixedRows(rows_tar, S_, A_, dev)
    call = [0]
    pol.noise_fn = lambda kind, shape: g["t%d_%s_eps" % (call[0], kind)].reshape(shape)
    for call[0] in (1, 2, 3):
        pol.train(src.rb, tar.rb, bs, None, None)
        assert pol.total_it == int(g["total_it_seq"][call[0] - 1]) and src.calls == [bs] * call[0] == tar.calls
        loss = pol._loss.cpu().numpy()
        for j, kind in enumerate(("policy", "dynamics")):
            np.testing.assert_allclose(loss[3 * j:3 * j + 3], g["t%d_%s_loss" % (call[0], kind)], rtol=1e-5)
        for vae, kind in ((pol.vae_policy, "policy"), (pol.vae_dyna, "dynamics")):
            for name, got in vae.state_dict().items():
                params_close(sub(got.cpu().numpy()), g["t%d_%s_p::%s" % (call[0], kind, name)], float(g["lr"]))
    with pytest.raises(NotImplementedError, match="critic / actor stage is not built"):      # where the reference moved on
        pol.train(src.rb, tar.rb, bs, None, None)
    assert pol.total_it == 6 and src.calls == [bs] * 3


def test_refusal_at_the_stage_boundary_leaves_the_device_rng_call_ids_unchanged(dev):
    """rng='device', graph replay: vae_iteration = 7 allows three calls; the fourth raises and moves no count, word or parameter."""
    pol = make(dev, vae_iteration=7, rng="device", seed=3, graph=1)
    load_scaled(pol)
    src, tar = buffers(dev, rng="device", seed=9)
    for _ in range(3):
        pol.train(src, tar, 8, None, None)
    torch.cuda.synchronize()
    assert pol.total_it == 6 and pol._graph is not None
    before = (state(pol), pol._ctr.clone(), pol._noise_calls, src._draws, tar._draws, pol.vae_policy_optimizer.t, pol.vae_dyna_optimizer.t)
    with pytest.raises(NotImplementedError, match="critic / actor stage is not built"):
        pol.train(src, tar, 8, None, None)
    torch.cuda.synchronize()
    assert pol.total_it == 6 and same_bits(before[0], state(pol)) and torch.equal(before[1], pol._ctr)
    assert before[2:] == (pol._noise_calls, src._draws, tar._draws, pol.vae_policy_optimizer.t, pol.vae_dyna_optimizer.t) == (3, 3, 3, 3, 3)
