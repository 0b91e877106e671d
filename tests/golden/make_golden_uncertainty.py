"""Generate the uncertainty-mode fixtures (g22) by running the REAL reference with uncertainty_mode = 'aleatoric' and
'ensemble_std' (mobody_dynamics.py:241-252), for the latent model and the MOPO ablation.

Same conventions as make_golden.py (whose helpers it imports and which it leaves unchanged): runs only where the
reference checkout is available, stores the reference's outputs and small explicit inputs, regenerates the weights from
`gen_inputs.dyn_params` (checksum stored as `wsum`).

  g22_uncertainty_{walker,ant,pen}   latent model, the inputs of g234 (same weights, same rows): per mode step() with
                                     (use_penalty, use_trg) in {(1,1), (0,1), (1,0)} and penalty_coef = 0.1
  g22_uncertainty_mopo_walker        the same for the mopo = 1 model, the inputs of g18
  (walker file only)                 per mode one MOBODY.rollout of H = 3 with filter_bad_rollout and env_filter = the median
                                     of that mode's step penalty

The noise and the elite ids do not depend on the mode or the flags (the tap regenerates them from its seed, NumPy is
re-seeded before every step), so they are stored once per file (`eps`, `idx`; `roll_eps{t}`, `roll_idx{t}`); the ensemble
means depend on use_trg only (`samples_t1`, `samples_t0`).  Keys of a step: `{mode}_p{use_penalty}_t{use_trg}_{next_obs,
reward, raw_reward, penalty, terminal}`; of a rollout: `roll_{mode}_{obss, next_obss, actions, rewards, terminals, penalty}`,
`roll_{mode}_env_filter`, `roll_{mode}_num_transitions`, `roll_{mode}_rows` (rows entering every step).

Usage:  python tests/golden/make_golden_uncertainty.py [latent] [mopo]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path)
from make_golden import RngTap, save, gi, policy_cfg, make_policy  # noqa: E402
from algo.dynamics.mobody_module import MOBODYModule  # noqa: E402
from algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics  # noqa: E402
from algo.mb_utils.terminal_funs import get_termination_fn  # noqa: E402

MODES = ("aleatoric", "ensemble_std")
FLAGS = ((1, 1), (0, 1), (1, 0))          # (use_penalty, use_trg)
ACTOR_SEED = 301


def steps(out, m, cfg_dyn, task, obs, act, seed):
    """step() of both modes in the three flag combinations into `out`; returns the dynamics objects by mode."""
    dyns = {}
    for mode in MODES:
        dyn = MOBODYEnsembleDynamics(dict(cfg_dyn), m, None, None, get_termination_fn(task), penalty_coef=0.1, uncertainty_mode=mode)
        dyns[mode] = dyn
        for up, ut in FLAGS:
            np.random.seed(seed)
            with RngTap(seed + 7) as tap:
                no, rw, term, info = dyn.step(torch.from_numpy(obs), torch.from_numpy(act), bool(up), bool(ut))
            for name, v in (("eps", tap.eps[0]), ("idx", tap.idx[0]), (f"samples_t{ut}", info["samples"].numpy())):
                if name in out:
                    assert np.array_equal(out[name], v), name          # mode / flag independent: stored once
                out[name] = v
            k = f"{mode}_p{up}_t{ut}_"
            out.update({k + "next_obs": no.numpy(), k + "reward": rw.numpy(), k + "terminal": term,
                        k + "penalty": info["penalty"].numpy(), k + "raw_reward": info["raw_reward"].numpy()})
    return dyns


def rollouts(out, dyns, S, A, obs, **cfg_over):
    """Per mode one MOBODY.rollout of H = 3 from `obs`, env_filter at the median of the mode's step penalty."""
    for mode in MODES:
        cfg = policy_cfg(S, A, **cfg_over)
        pol, pa, _, _ = make_policy(cfg, ACTOR_SEED)
        pol.dynamics = dyns[mode]
        cfg["env_filter"] = float(np.median(out[f"{mode}_p1_t1_penalty"]))
        np.random.seed(78)
        with RngTap(204) as tap:
            tr, inf = pol.rollout(torch.from_numpy(obs), 3, True)
        rows = [e.shape[1] for e in tap.eps]
        kept = len(tr["obss"])
        # conditions on the fixture: the filter drops some rows and keeps some, a row terminates before the last step
        assert 0 < kept < inf["num_transitions"], (mode, kept, inf["num_transitions"])
        assert len(rows) == 3 and rows[-1] < rows[0], (mode, rows)
        for t, (e, i) in enumerate(zip(tap.eps, tap.idx)):
            for name, v in ((f"roll_eps{t}", e), (f"roll_idx{t}", i)):
                if name in out:
                    assert np.array_equal(out[name], v), name
                out[name] = v
        out.update({f"roll_{mode}_env_filter": cfg["env_filter"], f"roll_{mode}_num_transitions": inf["num_transitions"],
                    f"roll_{mode}_rows": np.array(rows)})
        for k, v in tr.items():
            out[f"roll_{mode}_" + k] = v.numpy()
        print("rollout", mode, "rows", rows, "kept", kept, "filter", cfg["env_filter"])
    out.update(actor_seed=ACTOR_SEED, wsum_actor=gi.checksum(pa), n_steps=3)


def latent():
    for tag, S, A, B, task, ad, av, seed in mg.SHAPES:
        m, p = mg.load_dyn(S, A, seed, ad, av)
        rng = np.random.default_rng(seed + 1000)
        obs = gi.walker_like_obs(rng, B, S); act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
        out = dict(S=S, A=A, seed=seed, alive_dim=ad, alive_val=av, task=task, wsum=gi.checksum(p), obs=obs, act=act)
        dyns = steps(out, m, mg.DYN_CFG, task, obs, act, seed)
        if tag == "walker":
            rollouts(out, dyns, S, A, obs)
        print(tag, "terminated rows:", int(out["aleatoric_p1_t1_terminal"].sum()), "/", B,
              "penalty", [float(out[f"{mode}_p1_t1_penalty"].mean()) for mode in MODES])
        save(f"g22_uncertainty_{tag}", **out)


def mopo():
    cfg_dyn = dict(mg.DYN_CFG, mopo=1)
    S, A, B, task, seed = 17, 6, 48, "walker2d-medium-v2", 801          # g18's walker inputs
    p = gi.dyn_params(seed, S, A, mopo=True)
    p["za_src3.bias"][:, 0, 0] += np.float32(-0.35)                       # a few rows leave the alive box
    m = MOBODYModule(S, A, 256, 7, 5, device="cpu", config=dict(cfg_dyn))
    sd = m.state_dict()
    for k, v in p.items():
        assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    m.inference()
    rng = np.random.default_rng(seed + 1000)
    obs = gi.walker_like_obs(rng, B, S); act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    out = dict(S=S, A=A, seed=seed, task=task, wsum=gi.checksum(p), obs=obs, act=act)
    steps(out, m, cfg_dyn, task, obs, act, seed)
    print("mopo walker terminated rows:", int(out["aleatoric_p1_t1_terminal"].sum()), "/", B,
          "penalty", [float(out[f"{mode}_p1_t1_penalty"].mean()) for mode in MODES])
    save("g22_uncertainty_mopo_walker", **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["latent", "mopo"]:
        globals()[w]()
