"""The MOPO ablation (config['mopo'] = 1) past pre-training stays on the device path: the on-device rollout
(`mobody_ens_rollout` with the member MLP), the device-RNG refresh of the fake buffer through it, and the captured
`penalty_type='par'` step whose ensemble step reads its noise call id from the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
from test_hip_mirror import close, make_dynamics
from test_hip_replay import make_buf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def mopo_model(S, A, dev, seed=801, shift=-0.35):
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    p = gu.gi.dyn_params(seed, S, A, mopo=True)
    p["za_src3.bias"][:, 0, 0] += np.float32(shift)               # a share of the rows leaves the alive box every step
    m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=gu.policy_cfg(S, A, mopo=1))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    return m, p


def positional_mopo_step(m, task, obs, act, alive, elites, seed, call, coef, prec):
    """mobody_mopo_step itself (the positional entry point of the parent ABI)."""
    from mobody_amd import _lib
    S, A, dev, B = m.obs_dim, m.action_dim, obs.device, obs.shape[0]
    lib = _lib.load()
    ws = torch.empty(max(lib.mobody_dyn_step_workspace(S, A, B), 1), device=dev)
    o = dict(next_obs=torch.empty(B, S, device=dev), reward=torch.empty(B, 1, device=dev),
             terminal=torch.empty(B, 1, dtype=torch.uint8, device=dev), penalty=torch.empty(B, 1, device=dev))
    mb, mbt = m.packed_mopo()
    _lib.check(lib.mobody_mopo_step(m.packed().data_ptr(), _lib.ptr(m.planes() if prec else None), mb.data_ptr(), mbt.data_ptr(), prec,
                                    S, A, task, obs.data_ptr(), act.data_ptr(), B, None, None, _lib.ptr(alive),
                                    (C.c_int32 * len(elites))(*elites), len(elites), seed, call, coef, 1, o["next_obs"].data_ptr(),
                                    o["reward"].data_ptr(), o["terminal"].data_ptr(), o["penalty"].data_ptr(), None, None,
                                    ws.data_ptr(), _lib.cur_stream()), "mobody_mopo_step")
    return o


@pytest.mark.parametrize("mode", ["pairwise-diff", "ensemble_std"])
def test_mopo_rollout_on_device_equals_the_step_by_step_composition(mode, mfma, dev):
    """`mobody_ens_rollout` with a mopo model, device RNG, H = 5, a ring that wraps == the host loop over the stand-alone
    entry points with the same (seed, call0 + t): actor forward -> mobody_mopo_step (the default mode; mobody_ens_step for
    the other) -> mobody_rollout_mask -> mobody_ring_append.  Ring contents and {ptr, size} bit for bit."""
    from mobody_amd import ops, packing
    S, A, B, H, cap, task = 17, 6, 3000, 5, 3000, 4
    m, _ = mopo_model(S, A, dev)
    prec = ops.prec_id(mfma)
    pa, _, _ = gu.policy_params(301, S, A)
    actor = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
    akw = gu.mlp_kw(actor, S, A, 1, mfma)
    init = torch.from_numpy(gu.gi.walker_like_obs(np.random.default_rng(4), B, S)).to(dev)
    elites, seed, call0 = (0, 2, 3, 5, 6), 21, 7
    dkw = dict(planes=m.planes() if prec else None, precision=mfma, mopo=m.packed_mopo(), uncertainty_mode=mode)
    # the filter sits at the median penalty of the first step, so it drops about half of the live rows
    act0 = ops.mlp3_forward(actor, S, A, 1, init, out_mode=1, max_action=1.0, **akw)[0]
    filt = float(ops.dyn_step(m.packed(), S, A, task, init, act0, elites=elites, seed=seed, call=call0, **dkw)["penalty"].median())

    def ring():
        return make_buf("ring", cap, S, A, dev), torch.tensor([2000, 2000], dtype=torch.int64, device=dev)

    buf1, ps1 = ring()
    ops.rollout(m.packed(), actor, S, A, task, 1.0, init, H, elites, seed, call0, 0.1, True, True, filt, True, buf1, cap, ps1,
                dyn_planes=m.planes() if prec else None, actor_blob_T=akw.get("blob_T"), precision=mfma, mopo=m.packed_mopo(),
                uncertainty_mode=mode)
    buf2, ps2 = ring()
    obs, alive = init, None
    keep = torch.empty(B, dtype=torch.uint8, device=dev)
    kept_per_step = []
    for t in range(H):
        act = ops.mlp3_forward(actor, S, A, 1, obs, out_mode=1, max_action=1.0, **akw)[0]
        if mode == "pairwise-diff":
            r = positional_mopo_step(m, task, obs, act, alive, elites, seed, call0 + t, 0.1, prec)
        else:
            r = ops.dyn_step(m.packed(), S, A, task, obs, act, alive=alive, elites=elites, seed=seed, call=call0 + t,
                             penalty_coef=0.1, **dkw)
        nalive = torch.empty(B, dtype=torch.uint8, device=dev)
        ops.rollout_mask(alive, r["terminal"], r["penalty"], filt, True, keep, nalive)
        kept_per_step.append(int(keep.sum()))
        ops.ring_append(buf2, cap, ps2, S, A, obs, act, r["next_obs"], r["reward"], r["terminal"], keep)
        obs, alive = r["next_obs"], nalive
    # the case exercises what it claims: the filter drops and keeps rows, rows die, the ring wraps
    assert 0 < kept_per_step[0] < B and int(alive.sum()) < B and 2000 + sum(kept_per_step) > cap
    assert ps1.tolist() == ps2.tolist() and ps1.tolist()[1] == cap
    assert torch.equal(buf1.store.view(torch.int32), buf2.store.view(torch.int32))


def test_device_rng_refresh_of_a_mopo_model_rolls_out_on_the_device(mfma, dev, monkeypatch):
    """rng='device', mopo model: the first train() call fills the fake buffer through _rollout_into_fake (the host loop
    MOBODY.rollout is not entered); the rows are finite and the buffer holds exactly the kept rows -- counted here from
    step_device at the same (seed, call) with the alive mask carried along."""
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    g = gu.load("g18_mopo_walker")
    S, A, task = int(g["S"]), int(g["A"]), str(g["task"])
    cfg = gu.policy_cfg(S, A, mopo=1, rng="device", seed=3, src_rollout_length=2, trg_rollout_length=3,
                        use_src_sa_to_get_target_next_state=0)
    pol = MOBODY(cfg, dev)
    dyn = pol.dynamics = make_dynamics(gu.mopo_params_for(g, "walker"), S, A, task, dev, cfg, rng="device", seed=4)
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=60000, rng="device", seed=1), 60000, task, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=3000, rng="device", seed=2), 3000, task, 1)
    # the filter at the median penalty of a probe step on source rows: it drops some rows and keeps some
    probe = src.state[:512].contiguous()
    filt = float(dyn.step_device(probe, pol.policy(probe).reshape(-1, A), call=0)["penalty"].median())
    pol.config["env_filter"] = filt

    def no_host_loop(*a, **k):
        raise AssertionError("the device-RNG refresh of a mopo model entered the host loop MOBODY.rollout")

    monkeypatch.setattr(MOBODY, "rollout", no_host_loop)
    real, seen = MOBODY._rollout_into_fake, []

    def counted(self, init, H, use_trg=True):
        obs, alive, n = init.contiguous(), torch.ones(init.shape[0], dtype=torch.bool, device=dev), 0
        for t in range(H):
            r = dyn.step_device(obs, self.policy(obs).reshape(-1, A), use_trg, alive=alive.to(torch.uint8), call=dyn._calls + 1 + t)
            n += int((alive & (r["penalty"].flatten() <= filt)).sum())
            alive = alive & (r["terminal"].flatten() == 0)
            obs = r["next_obs"].clone()
        seen.append((init.shape[0], H, n))
        return real(self, init, H, use_trg)

    monkeypatch.setattr(MOBODY, "_rollout_into_fake", counted)
    pol.train(src, tar, 64, None, None)
    fb = pol.fake_replay_buffer
    assert [(b, h) for b, h, _ in seen] == [(50000, 2), (2000, 3)]
    kept = sum(n for _, _, n in seen)
    assert 0 < kept < 50000 * 2 + 2000 * 3 and fb.size == kept == fb.ptr
    for t in (fb.state, fb.action, fb.next_state, fb.reward, fb.not_done):
        assert torch.isfinite(t[:kept]).all()
    assert set(fb.not_done[:kept].unique().tolist()) <= {0.0, 1.0}
    assert all(v == v for v in pol.losses())


def test_par_graph_replay_of_a_mopo_model_matches_eager_steps(mfma, dev):
    """penalty_type='par' (the CLI's default), mopo model, device RNG: the steady-state step is captured (_graph_ok) and
    N replayed steps equal N eager steps fed with the same draws -- the assertions of
    test_graph_replay_matches_eager_steps[par] of the latent model."""
    from mobody_amd import synthetic, ops
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.mobody import GRAPH_DYN_SEED
    S, A, task, bs = 17, 6, "walker2d-medium-v2", 64
    fake_rows = gu.gi.batch(9, 300, S, A)
    p_dyn = gu.gi.dyn_params(31, S, A, mopo=True)

    def make(graph):
        torch.manual_seed(3)
        cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, src_rollout_length=0, trg_rollout_length=0,
                            use_src_sa_to_get_target_next_state=0, penalty_type="par", mopo=1)
        pol = call_algo("mobody", cfg, 3, dev)
        pol.dynamics = make_dynamics(p_dyn, S, A, task, dev, cfg, rng="device", seed=13)
        assert pol.dynamics.model.mopo
        pol.fake_replay_buffer.add_batch(dict(obss=fake_rows[0], actions=fake_rows[1], next_obss=fake_rows[2],
                                              rewards=fake_rows[3], terminals=1.0 - fake_rows[4]))
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, task, 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, task, 1)
        return pol, src, tar

    g, gs, gt = make(1)
    g.train(gs, gt, bs, None, None)              # step 1: eager (refresh step; rollouts disabled by the config)
    assert g._graph_ok(None) is False            # (still on the refresh step)
    for _ in range(3):
        g.train(gs, gt, bs, None, None)          # steps 2-4: captured graph
        assert g._graph_ok(None)
    assert g._graph is not None and g.q_optimizer.t == 4 and g._ctr.tolist()[:3] == [3, 4, 4]

    e, es, et = make(0)
    e.train(es, et, bs, None, None)
    for call in (1, 2, 3):
        e.total_it += 1
        c = torch.tensor([call], dtype=torch.int64, device=dev)
        idx = [ops.sample_indices(7 + 101, 3, c, 0, bs, es.ptr_size[1:2]), ops.sample_indices(7 + 102, 3, c, 0, bs, et.ptr_size[1:2]),
               ops.sample_indices(7 + 103, 3, c, 0, bs // 2, e.fake_replay_buffer.ptr_size[1:2])]
        ops.gather_batch([es._fields(), et._fields(), e.fake_replay_buffer._fields()], idx, S, A, out=e._batch)
        b = e._batch
        r = e.dynamics.step_device(b[0][:bs], b[1][:bs], call=call, seed_offset=GRAPH_DYN_SEED)
        ops.par_penalty(b[2][:bs], r["next_obs"], b[3][:bs], e.config["penalty_coef"])
        e._update(e._batch, int(2.5 * bs), 2 * bs)
    torch.cuda.synchronize()
    # the device-side Adam bias corrections use the GPU's double pow; the host path uses libm: allow 1 ulp of fp32
    close(g.q_funcs.blob, e.q_funcs.blob, rtol=1e-6, atol=1e-8)
    close(g.policy.blob, e.policy.blob, rtol=1e-6, atol=1e-8)
    close(g.target_q_funcs.blob, e.target_q_funcs.blob, rtol=1e-6, atol=1e-8)
    close(g._batch[3], e._batch[3], rtol=1e-6, atol=1e-7)       # the shaped source rewards of the last step agree too
