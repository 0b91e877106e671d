"""Pre-training of the MOPO ablation (config mopo = 1) on the GPU: the mopo kernels of csrc/pretrain.hip through the C ABI
and the mirror, against the reference's own runs (fixtures g20 / g21, tests/golden/make_golden_mopo.py) and the fp64 torch
restatement of tests/test_pretrain_mopo_fixture.py.  Tolerances are those of tests/test_hip_pretrain.py; every test that
takes the `mfma` fixture runs in exact fp32 and in f16x2 at the same tolerances."""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from test_pretrain_mopo_fixture import TRAINED, mopo_params_g20, mopo_step_grads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def close(a, b, rtol=1e-5, atol=1e-5):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a.astype(np.float64), b.astype(np.float64), rtol=rtol, atol=atol)


def mirror(p, S, A, dev, cfg_over=None):
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    cfg = gu.policy_cfg(S, A, **dict(dict(mopo=1, no_vae=0, inverse_sep_reward_loss=0, train_together=0,
                                          train_with_src_threshold=1, dynamics_lr=1e-3), **(cfg_over or {})))
    m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    return MOBODYEnsembleDynamics(cfg, m, None, None, get_termination_fn("walker2d-medium-v2"), penalty_coef=0.1), m


def noise_fn(rng, dev, S):
    return lambda b: torch.from_numpy(rng.standard_normal((7, b, S)).astype(np.float32)).to(dev)


@pytest.mark.parametrize("tag", ["walker", "ant", "walker_novae"])
def test_mopo_steps_vs_reference_golden(tag, dev, mfma):
    """Four learn() calls (src, trg, src, trg) of the mirror against the reference's: the reported losses, every gradient,
    post-Adam parameters, the untouched layers bit-identical, one Adam step count."""
    from mobody_amd import packing
    from test_hip_train import params_close
    g = gu.load(f"g20_pretrain_mopo_{tag}")
    S, A, b, seed = int(g["S"]), int(g["A"]), int(g["b"]), int(g["seed"])
    p = mopo_params_g20(g)
    dyn, m = mirror(p, S, A, dev, dict(no_vae=int(g["no_vae"])))
    dyn.train_noise_fn = noise_fn(gu.gi.noise_stream(int(g["noise_seed"])), dev, S)
    for step, use_trg in enumerate((False, True, False, True)):
        rows = gu.gi.pretrain_batch(4000 + 10 * seed + step, b, S, A)
        stats = dyn.learn(use_trg, *[torch.from_numpy(x) for x in rows], b, 0.01)
        close(np.array(stats), g[f"s{step}_losses"], rtol=2e-5, atol=1e-6)
        st = m.mopo_train_state()
        got = packing.unpack_pretrain_mopo(st["grad"], S, A)
        has = [str(x) for x in g[f"s{step}_has_grad"]]
        assert sorted(got) == has == TRAINED
        scale = {}
        for k in has:
            scale[k[:2]] = max(scale.get(k[:2], 0.0), float(np.abs(g[f"s{step}_g::{k}"]).max()))
        for k in has:
            close(gu.sub101(got[k].cpu().numpy()), g[f"s{step}_g::{k}"], rtol=1e-5, atol=1e-5 * scale[k[:2]])
            gk = got[k].double()
            close(float((gk * gk).sum()), g[f"s{step}_gsum::{k}"][1], rtol=1e-4, atol=1e-30)
        cur = packing.unpack_pretrain_mopo(st["blob"], S, A)
        for k in has:
            params_close(gu.sub101(cur[k].cpu().numpy()), g[f"s{step}_p::{k}"], 1e-3)
    sd = m.state_dict()
    for k, v in p.items():                               # zs*, transition*, za_trg*: no gradient, Adam never touches them
        if k.split(".")[0] + "." + k.split(".")[1] not in TRAINED:
            assert torch.equal(sd[k].cpu(), torch.from_numpy(v)), k
    steps = {x.split("=")[0]: int(x.split("=")[1]) for x in g["adam_steps"]}
    assert m.mopo_train_state()["t"] == 4 and set(steps.values()) == {4}


@pytest.mark.parametrize("S,A,b", [(17, 6, 1), (17, 6, 33), (17, 6, 256), (111, 8, 40), (45, 24, 65)])
def test_mopo_grads_vs_fp64_restatement(S, A, b, dev, mfma):
    """mobody_pretrain_mopo_grads against the torch restatement in fp64: the HIP error is at most 3x the fp32 restatement's
    (plus a floor of 1e-6 of the tensor's gradient scale), in both domains."""
    from mobody_amd import ops, packing
    p = gu.gi.dyn_params(40 + S + b, S, A, mopo=True)
    s, a, s2, r = gu.gi.pretrain_batch(70 + b, b, S, A)
    eps = np.random.default_rng(b).standard_normal((7, b, S)).astype(np.float32)
    blob = packing.pack_pretrain_mopo({k: torch.from_numpy(p[k]) for k in TRAINED}, S, A, dev)
    blob_T = ops.pretrain_mopo_transpose(blob, S, A, precision=mfma)
    grad, loss = torch.zeros_like(blob), torch.zeros(5, device=dev)
    ws = ops.pretrain_mopo_workspace(S, A, b, dev)
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for use_trg in (False, True):
        ops.pretrain_mopo_grads(S, A, b, use_trg, 1.0, blob, blob_T, td(np.concatenate([s, s2], 1)), td(a), td(r[..., 0]), grad,
                                loss, ws, noise=td(eps), precision=mfma)
        got = packing.unpack_pretrain_mopo(grad, S, A)
        l64, g64 = mopo_step_grads(p, (s, a, s2, r), eps, use_trg, dtype=torch.float64)
        l32, g32 = mopo_step_grads(p, (s, a, s2, r), eps, use_trg, dtype=torch.float32)
        close(loss.cpu().numpy()[[0, 1, 2, 4]], np.array(l64), rtol=2e-5, atol=1e-7)
        for k in TRAINED:
            ref = g64[k]
            e_hip = np.abs(got[k].cpu().numpy().astype(np.float64) - ref).max()
            e_t32 = np.abs(g32[k].astype(np.float64) - ref).max()
            assert e_hip <= 3 * e_t32 + 1e-6 * np.abs(ref).max() + 1e-12, (k, use_trg, e_hip, e_t32)


def test_mirror_train_vs_reference_golden(dev, mfma):
    """train() end to end in NumPy-RNG parity mode (fixture g21: 150 + 90 rows, max_epochs 2, batch 32): validate records,
    elites, the trained layers; afterwards forward_trg / step read the trained weights (the packed_mopo cache is rebuilt)."""
    g = gu.load("g21_dyn_train_mopo")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    dyn, m = mirror(mopo_params_g20(g), S, A, dev)
    dyn.train_noise_fn = noise_fn(gu.gi.noise_stream(int(g["noise_seed"])), dev, S)
    src = gu.gi.batch(911, int(g["n_src"]), S, A); trg = gu.gi.batch(912, int(g["n_trg"]), S, A)
    before = m.packed_mopo()[0].clone()
    torch.manual_seed(int(g["rng_seed"])); np.random.seed(int(g["rng_seed"]))
    dyn.train(tuple(torch.from_numpy(x) for x in src), tuple(torch.from_numpy(x) for x in trg), max_epochs=2, batch_size=bs)
    assert dyn.total_steps == int(g["total_steps"]) and dyn._train_calls == int(g["n_noise"])
    want = g["validate"]
    got = []
    for h in dyn.history:
        got += [h["src_val"], h["trg_val"]]
    close(np.array(got), want[:, 0], rtol=1e-4, atol=1e-8)
    close(np.array(dyn.history[-1]["trg_reward_val"]), want[-1, 1], rtol=1e-4, atol=1e-8)
    el, wel = [int(x) for x in m.elites.tolist()], [int(x) for x in g["elites"]]
    assert sorted(el) == sorted(wel)
    fin = want[-1, 0]
    for a_, b_ in zip(el, wel):
        assert a_ == b_ or abs(fin[a_] - fin[b_]) <= 1e-4 * abs(fin[b_]), (el, wel)
    sd = m.state_dict()
    for k in g:
        if k.startswith("sd::"):
            d = np.abs(gu.sub101(sd[k[4:]].cpu().numpy()).astype(np.float64) - g[k])
            assert d.max() <= 5e-4, (k, d.max())
            assert (d <= 1e-5 + 1e-4 * np.abs(g[k])).mean() >= 0.98, k
    assert torch.equal(sd["za_src1.weight"], sd["za_src1.saved_weight"])
    assert not torch.equal(m.packed_mopo()[0], before)
    _check_forward_reads_state_dict(dyn, m, S, A, dev)


def _check_forward_reads_state_dict(dyn, m, S, A, dev):
    from test_pretrain_mopo_fixture import _mlp
    sd = m.state_dict()
    rng = np.random.default_rng(1)
    obs = torch.from_numpy(gu.gi.walker_like_obs(rng, 19, S)).to(dev)
    act = torch.from_numpy(rng.uniform(-1, 1, (19, A)).astype(np.float32)).to(dev)
    with torch.no_grad():
        P = {k: sd[k].double() for k in TRAINED}
        want = obs.double() + _mlp(P, "za_src", torch.cat([obs, act], -1).double().unsqueeze(0).repeat(7, 1, 1))
    close(m.forward_trg(obs, act)[0], want, rtol=2e-5, atol=2e-5)
    close(m.forward_src(obs, act)[0], want, rtol=2e-5, atol=2e-5)
    r = dyn.step_device(obs, act, want_mean=True)
    close(r["mean"], want, rtol=2e-5, atol=2e-5)


def test_forward_uses_weights_after_fused_training(dev, mfma):
    """_learn_indexed (fused update, device RNG) moves the weights; forward_trg / step then equal s + MLP(state_dict)."""
    S, A, b, n = 17, 6, 32, 200
    dyn, m = mirror(gu.gi.dyn_params(6, S, A, mopo=True), S, A, dev)
    s, a, s2, r, _ = gu.gi.batch(4, n, S, A)
    td = lambda x: torch.from_numpy(x).to(dev)
    _check_forward_reads_state_dict(dyn, m, S, A, dev)               # builds the packed_mopo cache before training
    idx = td(np.random.default_rng(2).integers(0, n, (7, 3 * b)).astype(np.int32)).contiguous()
    stats = dyn._learn_indexed(True, [td(s), td(a), td(s2), td(r)], idx, b)
    assert all(np.isfinite(stats)) and m.mopo_train_state()["t"] == 3
    _check_forward_reads_state_dict(dyn, m, S, A, dev)
    m.update_save(range(7)); m.load_save()                           # saved <- weight, then weight <- saved: a no-op
    _check_forward_reads_state_dict(dyn, m, S, A, dev)


def test_graph_replay_equals_eager_fused_steps(dev, mfma):
    """One pass of _learn_indexed (5 full batches + a ragged one, device-Philox noise) as captured-graph replays equals the
    eager fused steps; and the fused step equals grads + Adam."""
    from mobody_amd import ops, packing
    from test_hip_train import params_close
    S, A, b, n = 17, 6, 32, 400
    p = gu.gi.dyn_params(5, S, A, mopo=True)
    s, a, s2, r, _ = gu.gi.batch(4, n, S, A)
    td = lambda x: torch.from_numpy(x).to(dev)
    data = [td(s), td(a), td(s2), td(r)]
    idx = td(np.random.default_rng(2).integers(0, n, (7, 5 * b + 7)).astype(np.int32)).contiguous()
    out = {}
    for mode in ("graph", "eager"):
        dyn, m = mirror(p, S, A, dev, dict(train_graph=int(mode == "graph")))
        dyn.seed = 9
        st1 = dyn._learn_indexed(True, data, idx, b)
        st2 = dyn._learn_indexed(False, data, idx, b)
        assert (len(dyn._pre_graphs) == 2) == (mode == "graph")
        assert m.mopo_train_state()["t"] == 12
        out[mode] = (st1, st2, {k: v.cpu() for k, v in m.state_dict().items() if k in p})
    for k in out["graph"][2]:
        np.testing.assert_allclose(out["graph"][2][k].numpy(), out["eager"][2][k].numpy(), rtol=2e-6, atol=1e-8, err_msg=k)
    close(np.array(out["graph"][0]), np.array(out["eager"][0]), rtol=1e-5, atol=1e-6)
    close(np.array(out["graph"][1]), np.array(out["eager"][1]), rtol=1e-5, atol=1e-6)
    # fused (mobody_pretrain_mopo_update) == unfused (grads + adam) on the same rows and the same device noise
    dyn, m = mirror(p, S, A, dev)
    dyn.seed = 9
    dyn._learn_indexed(True, data, idx[:, :b].contiguous(), b)
    blob = packing.pack_pretrain_mopo({k: torch.from_numpy(p[k]) for k in TRAINED}, S, A, dev)
    blob_T = ops.pretrain_mopo_transpose(blob, S, A, precision=mfma)
    grad, mm, vv = (torch.zeros_like(blob) for _ in range(3))
    loss = torch.zeros(5, device=dev)
    xenc, act, rew = ops.pretrain_gather(*data, idx, 0, b)
    ops.pretrain_mopo_grads(S, A, b, True, 1.0, blob, blob_T, xenc, act, rew, grad, loss, ops.pretrain_mopo_workspace(S, A, b, dev),
                            seed=9 + 77, call=1, precision=mfma)
    ops.pretrain_mopo_adam(S, A, blob, blob_T, grad, mm, vv, 1, 1e-3, precision=mfma)
    got = m.state_dict()
    for k, v in packing.unpack_pretrain_mopo(blob, S, A).items():
        params_close(got[k], v, 1e-3)


def test_dyn_validate_mopo_vs_torch(dev):
    """mobody_dyn_validate_mopo at a ragged B: mean = s + MLP(s, a), the reward head of the inference blob on (s, a, mean)."""
    from mobody_amd import ops, packing
    from test_pretrain_mopo_fixture import _mlp
    S, A, B = 17, 6, 45
    p = gu.gi.dyn_params(8, S, A, mopo=True)
    dyn, m = mirror(p, S, A, dev)
    s, a, s2, r, _ = gu.gi.batch(3, B, S, A)
    td = lambda x: torch.from_numpy(x).to(dev)
    out = ops.dyn_validate_mopo(m.packed(), m.packed_mopo()[0], S, A, td(s), td(a), td(s2), td(r)).cpu().numpy()
    P = {k: torch.from_numpy(p[k]).double() for k in TRAINED}
    x = lambda v: torch.from_numpy(v).double().unsqueeze(0).repeat(7, 1, 1)
    mean = x(s) + _mlp(P, "za_src", torch.cat([x(s), x(a)], -1))
    rr = _mlp(P, "reward_model", torch.cat([x(s), x(a), mean], -1))[..., :1]
    close(out[:7], ((mean - x(s2)) ** 2).mean(dim=(1, 2)).numpy(), rtol=2e-5, atol=1e-8)
    close(out[7:], ((rr - x(r)) ** 2).mean(dim=(1, 2)).numpy(), rtol=2e-5, atol=1e-8)
    tv, rv = dyn.validate(True, s, a, s2, r)
    close(np.array(tv), out[:7], rtol=1e-6, atol=0); close(np.array(rv), out[7:], rtol=1e-6, atol=0)


@pytest.mark.parametrize("over", [dict(train_together=1), dict(inverse_sep_reward_loss=1), dict(train_with_src_threshold=0.5),
                                  dict(latent_reward=1), "dp"])
def test_mopo_refuses_what_is_not_built(over, dev):
    S, A = 17, 6
    dyn, m = mirror(gu.gi.dyn_params(5, S, A, mopo=True), S, A, dev)
    if over == "dp":
        dyn._world = lambda: (2, 0)
    else:
        dyn.config = dict(dyn.config, **over)
    rows = [torch.from_numpy(x) for x in gu.gi.pretrain_batch(1, 8, S, A)]
    with pytest.raises(NotImplementedError, match="mopo"):
        dyn.learn(False, *rows, 8, 0.01)
    with pytest.raises(NotImplementedError):
        m.train_state()                                  # the latent layout's copy does not apply to a mopo model


def test_cli_mopo_trains_saves_and_reloads(tmp_path, monkeypatch, capsys):
    """--mopo 1 --train_dynamics 1 on dataset files: the ensemble is pre-trained and saved with the reference mopo module's
    state_dict layout; a second run with --train_dynamics 0 loads it and reproduces the forward."""
    from mobody_amd import train_mobody as tm
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(7)
    S, A, n, m_ = 17, 6, 1200, 401
    mu = np.zeros(S, np.float32); mu[0] = 1.25
    obs = (mu + 0.1 * rng.standard_normal((n, S))).astype(np.float32)
    np.savez(tmp_path / "src.npz", observations=obs, actions=rng.uniform(-1, 1, (n, A)).astype(np.float32),
             next_observations=(obs + 0.01 * rng.standard_normal((n, S))).astype(np.float32),
             rewards=rng.standard_normal(n).astype(np.float32), terminals=np.zeros(n, bool))
    tobs = (mu + 0.1 * rng.standard_normal((m_, S))).astype(np.float32)
    np.savez(tmp_path / "tar.npz", observations=tobs, actions=rng.uniform(-1, 1, (m_, A)).astype(np.float32),
             rewards=rng.standard_normal((m_, 1)).astype(np.float32), terminals=np.zeros(m_, bool), timeouts=np.zeros(m_, bool))
    argv = ["--policy", "MOBODY", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "3", "--mopo", "1",
            "--synthetic", "0", "--src_data", str(tmp_path / "src.npz"), "--tar_data", str(tmp_path / "tar.npz"),
            "--penalty_type", "none", "--src_rollout_batch_size", "300", "--trg_rollout_batch_size", "100", "--max_step", "2",
            "--params", '{"batch_size": 64, "max_step": 2}', "--dir", str(tmp_path / "logs"), "--dynamics_max_epochs", "1"]
    pol = tm.main(argv + ["--train_dynamics", "1"])
    assert "dynamics trained and saved" in capsys.readouterr().out
    assert pol.dynamics.model.mopo and pol.dynamics.total_steps > 0
    leaf = "srcdatatype-medium-tardatatype-medium-2.0"
    path = tmp_path / "pretrained_dynamics" / "walker2d-friction" / leaf / "dynamics.pth"
    sd = torch.load(path, weights_only=True)
    want = json.load(open(os.path.join(gu.GOLDEN, "g21_mopo_dynamics_pth.json")))
    assert {k: list(v.shape) for k, v in sd.items()} == {d["name"]: d["shape"] for d in want["keys"]}
    assert all(str(sd[d["name"]].dtype) == "torch." + d["dtype"] for d in want["keys"])
    x = torch.from_numpy(obs[:13]).to(pol.dynamics.model.device)
    u = torch.from_numpy(rng.uniform(-1, 1, (13, A)).astype(np.float32)).to(x.device)
    f1 = pol.dynamics.model.forward_trg(x, u)[0].clone()
    pol2 = tm.main(argv + ["--train_dynamics", "0"])
    assert "pretrained dynamics loaded" in capsys.readouterr().out
    sd2 = pol2.dynamics.model.state_dict()
    assert all(torch.equal(sd[k].to(sd2[k].device), sd2[k]) for k in sd)
    assert torch.equal(pol2.dynamics.model.forward_trg(x, u)[0], f1)
