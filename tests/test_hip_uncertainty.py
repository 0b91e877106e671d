"""The three uncertainty modes of MOBODYEnsembleDynamics.step (mobody_dynamics.py:241-252) on the HIP path: the mirror's
step and rollout against the reference's g22 fixtures, and the sample kernel through the C ABI against an fp64
restatement of the formulas on the kernel's own ensemble means (latent model and MOPO ablation, both MFMA modes)."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
from test_hip_mirror import close, feed, make_dynamics
from test_uncertainty_fixture import FLAGS, MODES, params_for, penalty_f64

pytestmark = pytest.mark.gpu
ALL_MODES = ("pairwise-diff",) + MODES
SHAPES = ((17, 6, 4), (111, 8, 3), (45, 24, 6))          # (S, A, termination id): walker, ant, pen


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def dynamics_in_mode(p, S, A, task, dev, cfg, mode, **kw):
    """make_dynamics' model under a MOBODYEnsembleDynamics of uncertainty mode `mode`."""
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    d = make_dynamics(p, S, A, task, dev, cfg, **kw)
    return MOBODYEnsembleDynamics(cfg, d.model, None, None, d.terminal_fn, penalty_coef=d._penalty_coef,
                                  uncertainty_mode=mode, rng=d.rng, seed=d.seed)


@pytest.mark.parametrize("tag", ["walker", "ant", "pen", "mopo_walker"])
def test_mirror_step_vs_reference_golden(tag, mfma, dev):
    g = gu.load(f"g22_uncertainty_{tag}")
    S, A, task = int(g["S"]), int(g["A"]), str(g["task"])
    cfg = gu.policy_cfg(S, A, mopo=int(tag == "mopo_walker"))
    obs, act = torch.from_numpy(g["obs"]).to(dev), torch.from_numpy(g["act"]).to(dev)
    for mode in MODES:
        dyn = dynamics_in_mode(params_for(g, tag), S, A, task, dev, cfg, mode)
        assert dyn.model.mopo == (tag == "mopo_walker")
        for up, ut in FLAGS:
            k = f"{mode}_p{up}_t{ut}_"
            feed(dyn, [g["eps"]])
            np.random.seed(int(g["seed"]))                      # the golden run drew its elite ids from this NumPy state
            no, rw, term, info = dyn.step(obs, act, bool(up), bool(ut))
            close(info["samples"], g[f"samples_t{ut}"])
            close(no, g[k + "next_obs"]); close(rw, g[k + "reward"]); close(info["raw_reward"], g[k + "raw_reward"])
            close(info["penalty"], g[k + "penalty"])
            assert (term == g[k + "terminal"]).all()
        feed(dyn, [g["eps"]])                                    # model_error carries the mode too
        np.random.seed(int(g["seed"]))
        close(dyn.model_error(obs, act, g[f"{mode}_p0_t1_next_obs"], g[f"{mode}_p0_t1_reward"])["penalty"], g[f"{mode}_p0_t1_penalty"])


@pytest.mark.parametrize("mode", MODES)
def test_mirror_rollout_vs_reference_golden(mode, mfma, dev):
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    g = gu.load("g22_uncertainty_walker")
    S, A, task = int(g["S"]), int(g["A"]), str(g["task"])
    cfg = gu.policy_cfg(S, A, env_filter=float(g[f"roll_{mode}_env_filter"]))
    pol = MOBODY(cfg, dev)
    pa, _, _ = gu.policy_params(int(g["actor_seed"]), S, A)
    pol.policy.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    pol.dynamics = dynamics_in_mode(gu.dyn_params_for(g), S, A, task, dev, cfg, mode)
    feed(pol.dynamics, [g[f"roll_eps{t}"] for t in range(int(g["n_steps"]))])
    np.random.seed(78)
    res, info = pol.rollout(torch.from_numpy(g["obs"]).to(dev), 3, True)
    assert info["num_transitions"] == int(g[f"roll_{mode}_num_transitions"])
    for k in ("obss", "next_obss", "actions", "rewards", "terminals", "penalty"):
        assert tuple(res[k].shape) == g[f"roll_{mode}_{k}"].shape, k
        close(res[k], g[f"roll_{mode}_{k}"], rtol=2e-5, atol=2e-5)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _inputs(S, A, B, seed, dev):
    rng = np.random.default_rng(seed)
    obs = gu.gi.walker_like_obs(rng, B, S); act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    eps = rng.standard_normal((7, B, S)).astype(np.float32); idx = rng.integers(0, 5, B)
    return torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), eps, idx


def _positional_dyn_step(blob, S, A, task, obs, act, eps, idx, kw):
    """mobody_dyn_step itself (the positional entry point), outputs as ops.dyn_step returns them."""
    from mobody_amd import _lib, ops
    dev, B = obs.device, obs.shape[0]
    noise = torch.from_numpy(eps).to(dev).contiguous()
    eid = torch.as_tensor(idx).to(device=dev, dtype=torch.int32).contiguous()
    ws = torch.empty(max(_lib.load().mobody_dyn_step_workspace(S, A, B), 1), device=dev)
    out = dict(next_obs=torch.empty(B, S, device=dev), reward=torch.empty(B, 1, device=dev),
               terminal=torch.empty(B, 1, dtype=torch.uint8, device=dev), penalty=torch.empty(B, 1, device=dev),
               raw_reward=torch.empty(B, 1, device=dev), mean=torch.empty(7, B, S, device=dev))
    planes = kw.get("planes")
    _lib.check(_lib.load().mobody_dyn_step(blob.data_ptr(), _lib.ptr(planes), ops.prec_id(kw.get("precision", 0)), S, A, task,
                                           obs.data_ptr(), act.data_ptr(), B, noise.data_ptr(), eid.data_ptr(), None,
                                           (C.c_int32 * 5)(0, 1, 2, 3, 4), 5, 0, 0, None, 0.25, 1, 1, out["next_obs"].data_ptr(),
                                           out["reward"].data_ptr(), out["terminal"].data_ptr(), out["penalty"].data_ptr(),
                                           out["raw_reward"].data_ptr(), out["mean"].data_ptr(), ws.data_ptr(), _lib.cur_stream()),
               "mobody_dyn_step")
    return out


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
def test_penalty_of_every_mode_vs_fp64_on_the_kernels_own_means(B, mfma, dev):
    """C ABI at ragged batch sizes and three (S, A) shapes, latent model and (walker shape) the MOPO ablation: the penalty
    equals the fp64 formula applied to the kernel's own mean_out at 1e-5 abs + rel, the reward is raw - coef * penalty, a
    second launch gives identical bits, and mode 0 through mobody_ens_step is bit-identical to mobody_dyn_step."""
    from mobody_amd import ops, packing
    for S, A, task in SHAPES:
        p = gu.gi.dyn_params(7, S, A)
        blob = packing.pack_dynamics(p, S, A, dev)
        kw = gu.dyn_kw(blob, S, A, mfma)
        obs, act, eps, idx = _inputs(S, A, B, 100 * S + B, dev)
        mopos = [None]
        if S == 17:
            from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
            m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=gu.policy_cfg(S, A, mopo=1))
            m.load_state_dict({k: torch.from_numpy(v) for k, v in gu.gi.dyn_params(8, S, A, mopo=True).items()}, strict=False)
            mopos.append(m)
        for m in mopos:
            run = (lambda mode: ops.dyn_step(blob, S, A, task, obs, act, noise=eps, elite_idx=idx, penalty_coef=0.25,
                                             want_mean=True, uncertainty_mode=mode, **kw)) if m is None else \
                  (lambda mode: ops.dyn_step(m.packed(), S, A, task, obs, act, noise=eps, elite_idx=idx, penalty_coef=0.25,
                                             want_mean=True, uncertainty_mode=mode, mopo=m.packed_mopo(),
                                             planes=m.planes() if mfma != "f32" else None, precision=mfma))
            seen = []
            for mode in ALL_MODES:
                r1 = run(mode)
                r2 = run(mode)
                for k in r1:
                    assert same_bits(r1[k], r2[k]), (S, mode, k)
                want = penalty_f64(mode, r1["mean"].cpu().numpy())
                close(r1["penalty"], want)
                close(r1["reward"], r1["raw_reward"].cpu().numpy().astype(np.float64) - 0.25 * want)
                seen.append(r1)
            for r in seen[1:]:                                 # the mode changes the penalty and the reward only
                assert torch.equal(r["next_obs"], seen[0]["next_obs"]) and torch.equal(r["terminal"], seen[0]["terminal"])
                assert torch.equal(r["raw_reward"], seen[0]["raw_reward"]) and torch.equal(r["mean"], seen[0]["mean"])
                assert not torch.allclose(r["penalty"], seen[0]["penalty"], rtol=1e-3, atol=0)
            if m is None:
                old = _positional_dyn_step(blob, S, A, task, obs, act, eps, idx, kw)
                for k in old:
                    assert same_bits(old[k], seen[0][k]), (S, k)


def test_nan_member_poisons_every_mode_and_the_row_is_dropped(mfma, dev):
    """One member with a NaN weight: torch's amax / norm / var / sqrt all propagate it, so the penalty is NaN in every mode,
    `penalty <= env_filter` is False and no row reaches the ring through the fused filter of the on-device rollout."""
    from mobody_amd import ops, packing
    from test_hip_replay import make_buf
    S, A, B = 17, 6, 70
    p = gu.gi.dyn_params(7, S, A)
    p["transition3.bias"][:, 0, 0] += np.float32(0.85)
    p["transition3.bias"][2, 0, 5] = np.nan
    blob = packing.pack_dynamics(p, S, A, dev)
    kw = gu.dyn_kw(blob, S, A, mfma)
    pa, _, _ = gu.policy_params(301, S, A)
    actor = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
    akw = gu.mlp_kw(actor, S, A, 1, mfma)
    obs, act, eps, idx = _inputs(S, A, B, 3, dev)
    for mode in ALL_MODES:
        got = ops.dyn_step(blob, S, A, 4, obs, act, noise=eps, elite_idx=idx, penalty_coef=0.1, uncertainty_mode=mode, **kw)
        assert torch.isnan(got["penalty"]).all(), mode
        keep = torch.empty(B, dtype=torch.uint8, device=dev); alive = torch.empty(B, dtype=torch.uint8, device=dev)
        ops.rollout_mask(None, got["terminal"], got["penalty"], 1e9, True, keep, alive)
        assert int(keep.sum()) == 0
        # terminal / alive follow the predicate on the kernel's own next_obs
        done = ops.termination(4, got["next_obs"])
        assert torch.equal(done, got["terminal"]) and torch.equal(alive, 1 - done.flatten())
        # the fused filter of the rollout (keep / alive_out formed in the sample kernel): nothing is appended
        ring, ps = make_buf("ring", 512, S, A, dev), torch.zeros(2, dtype=torch.int64, device=dev)
        ops.rollout(blob, actor, S, A, 4, 1.0, obs, 2, (0, 1, 2, 3, 4), 5, 1, 0.1, True, True, 1e9, True, ring, 512, ps,
                    dyn_planes=kw.get("planes"), actor_blob_T=akw.get("blob_T"), precision=mfma, uncertainty_mode=mode)
        assert ps.tolist() == [0, 0], mode
        ops.rollout(blob, actor, S, A, 4, 1.0, obs, 2, (0, 1, 2, 3, 4), 5, 1, 0.1, True, True, 1e9, False, ring, 512, ps,
                    dyn_planes=kw.get("planes"), actor_blob_T=akw.get("blob_T"), precision=mfma, uncertainty_mode=mode)
        n = ps.tolist()[1]                                       # without the filter: every row at step 1, the alive ones at 2
        assert B <= n <= 2 * B
