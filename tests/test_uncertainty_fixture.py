"""The uncertainty-mode fixtures (g22, written by the reference with uncertainty_mode = 'aleatoric' / 'ensemble_std',
mobody_dynamics.py:241-252) are internally consistent, and the CPU-visible side of the feature: the struct-argument
entry points validate their arguments without a GPU and the mirror's constructor accepts the three modes.

fp64 restatement of the two penalties on the ensemble means m[e, b, d] (7 members), var_d = unbiased variance over e:
  aleatoric     sqrt(sum_{d < S} var_d)          (amax over seven equal norms of the repeated std; ALL S dims)
  ensemble_std  sqrt(mean_{d < S-1} var_d)       (last state dim dropped)
Tolerance: the project's step tolerance, 1e-5 absolute + relative."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import golden_util as gu

MODES = ("aleatoric", "ensemble_std")
FLAGS = ((1, 1), (0, 1), (1, 0))
FILES = ("walker", "ant", "pen", "mopo_walker")
TOL = dict(rtol=1e-5, atol=1e-5)


def penalty_f64(mode, mean):
    """The reference's penalty of `mode` from the ensemble means [7, B, S], in fp64."""
    m = np.asarray(mean, np.float64)
    var = m.var(axis=0, ddof=1)                                   # [B, S]
    if mode == "aleatoric":
        return np.sqrt(var.sum(axis=1))[:, None]
    if mode == "ensemble_std":
        return np.sqrt(var[:, :-1].mean(axis=1))[:, None]
    assert mode == "pairwise-diff"
    d = m[..., :-1] - m[..., :-1].mean(axis=0)
    return np.sqrt((d ** 2).sum(axis=2)).max(axis=0)[:, None]


def params_for(g, tag):
    if tag == "mopo_walker":
        p = gu.gi.dyn_params(int(g["seed"]), int(g["S"]), int(g["A"]), mopo=True)
        p["za_src3.bias"][:, 0, 0] += np.float32(-0.35)
        return p
    return gu.dyn_params_for(g)


@pytest.mark.parametrize("tag", FILES)
def test_g22_steps_are_consistent_with_the_formulas(tag):
    g = gu.load(f"g22_uncertainty_{tag}")
    S, B = int(g["S"]), g["obs"].shape[0]
    p = params_for(g, tag)
    assert abs(gu.gi.checksum(p) - float(g["wsum"])) <= 1e-9 * abs(float(g["wsum"])), "weight generator drifted from the fixture"
    assert g["eps"].shape == (7, B, S) and g["idx"].shape == (B,)
    assert os.path.getsize(os.path.join(gu.GOLDEN, f"g22_uncertainty_{tag}.npz")) < 830 * 1024
    for mode in MODES:
        for up, ut in FLAGS:
            k = f"{mode}_p{up}_t{ut}_"
            pen, raw, rew = g[k + "penalty"], g[k + "raw_reward"], g[k + "reward"]
            assert pen.shape == raw.shape == rew.shape == (B, 1)
            np.testing.assert_allclose(pen.astype(np.float64), penalty_f64(mode, g[f"samples_t{ut}"]), **TOL)
            if up:
                np.testing.assert_allclose(rew, raw - np.float32(0.1) * pen, rtol=1e-6, atol=1e-7)
            else:
                assert np.array_equal(rew, raw)
            # the sample is the elite member's mean plus eps * the unbiased std
            m = g[f"samples_t{ut}"].astype(np.float64)
            nxt = m[g["idx"], np.arange(B)] + g["eps"][g["idx"], np.arange(B)] * m.std(axis=0, ddof=1)
            np.testing.assert_allclose(g[k + "next_obs"], nxt, **TOL)
        # the modes differ from each other and from the default on the same means
        assert not np.allclose(g[f"{mode}_p1_t1_penalty"], penalty_f64("pairwise-diff", g["samples_t1"]), **TOL)
    assert 0 < int(g["aleatoric_p1_t1_terminal"].sum()) < B                    # some rows terminate, some do not


def test_g22_rollouts_are_consistent_with_their_filter():
    g = gu.load("g22_uncertainty_walker")
    S, A = int(g["S"]), int(g["A"])
    pa, _, _ = gu.policy_params(int(g["actor_seed"]), S, A)
    assert abs(gu.gi.checksum(pa) - float(g["wsum_actor"])) <= 1e-9 * abs(float(g["wsum_actor"]))
    for mode in MODES:
        rows = g[f"roll_{mode}_rows"].tolist()
        filt = float(g[f"roll_{mode}_env_filter"])
        assert filt == float(np.median(g[f"{mode}_p1_t1_penalty"]))
        assert len(rows) == int(g["n_steps"]) == 3 and rows[-1] < rows[0]      # a row terminated before the last step
        assert int(g[f"roll_{mode}_num_transitions"]) == sum(rows)
        assert [g[f"roll_eps{t}"].shape[1] for t in range(3)] == rows
        kept = g[f"roll_{mode}_obss"].shape[0]
        assert 0 < kept < sum(rows)                                             # the filter drops some rows and keeps some
        for k, w in (("obss", S), ("next_obss", S), ("actions", A), ("rewards", 1), ("terminals", 1), ("penalty", 1)):
            assert g[f"roll_{mode}_{k}"].shape == (kept, w), k
        assert (g[f"roll_{mode}_penalty"] <= np.float32(filt)).all()
        assert set(np.unique(g[f"roll_{mode}_terminals"])) <= {0.0, 1.0}


# ---------------------------------------------------------------------------------------------- C ABI, no GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _step(mode, B, **over):
    from mobody_amd import _lib
    a = _lib.MobodyEnsStep()
    a.struct_bytes, a.uncertainty_mode, a.S, a.A, a.task, a.B = C.sizeof(_lib.MobodyEnsStep), mode, 17, 6, 4, B
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _rollout(mode, B, H, **over):
    from mobody_amd import _lib
    a = _lib.MobodyEnsRollout()
    a.struct_bytes, a.uncertainty_mode, a.S, a.A, a.task, a.B, a.H = C.sizeof(_lib.MobodyEnsRollout), mode, 17, 6, 4, B, H
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_struct_entry_points_validate_without_a_gpu(lib):
    from mobody_amd import _lib
    assert _lib.UNCERTAINTY_MODES == {"pairwise-diff": 0, "aleatoric": 1, "ensemble_std": 2}
    # natural C layout of the header's structs on LP64 (no implicit padding: every member is declared)
    assert C.sizeof(_lib.MobodyEnsStep) == 8 + 4 * 8 + 16 + 2 * 8 + 8 + 4 * 8 + 16 + 8 + 8 + 7 * 8
    assert C.sizeof(_lib.MobodyEnsRollout) == 8 + 6 * 8 + 16 + 8 + 8 + 8 + 8 + 8 + 8 + 24 + 8 + 8 + 8 + 8
    # empty batches: 0 in every mode, no pointer touched
    for mode in (0, 1, 2):
        assert lib.mobody_ens_step(C.byref(_step(mode, 0)), None) == 0
        assert lib.mobody_ens_rollout(C.byref(_rollout(mode, 0, 3)), None) == 0
        assert lib.mobody_ens_rollout(C.byref(_rollout(mode, 5, 0)), None) == 0
    # an unknown mode: -1 with a text, before any pointer is looked at
    for bad in (3, -1, 99):
        assert lib.mobody_ens_step(C.byref(_step(bad, 5)), None) == -1
        assert b"uncertainty_mode" in lib.mobody_last_error() and b"mobody_ens_step" in lib.mobody_last_error()
        assert lib.mobody_ens_rollout(C.byref(_rollout(bad, 5, 2)), None) == -1
        assert b"uncertainty_mode" in lib.mobody_last_error() and b"mobody_ens_rollout" in lib.mobody_last_error()
    # the other argument checks of the positional entry points hold for the struct form
    assert lib.mobody_ens_step(C.byref(_step(1, 5)), None) == -1 and b"null pointer" in lib.mobody_last_error()
    assert lib.mobody_ens_step(C.byref(_step(0, 5, struct_bytes=12)), None) == -1 and b"struct_bytes" in lib.mobody_last_error()
    assert lib.mobody_ens_rollout(C.byref(_rollout(0, 5, 2, struct_bytes=12)), None) == -1
    assert lib.mobody_ens_step(None, None) == -1
    assert lib.mobody_ens_step(C.byref(_step(0, 0, S=1000)), None) == -1 and b"unsupported" in lib.mobody_last_error()
    # workspace query == the positional one
    for B in (0, 1, 4096):
        assert lib.mobody_ens_rollout_workspace(C.byref(_rollout(2, B, 3))) == lib.mobody_rollout_workspace(17, 6, B)
    assert lib.mobody_ens_rollout_workspace(C.byref(_rollout(0, 5, 3, struct_bytes=4))) < 0


def test_mirror_constructor_accepts_the_three_modes():
    """Raised NotImplementedError for 'aleatoric' / 'ensemble_std' before the modes ran on the kernel path."""
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    cfg = dict(encoder_loss_coef=1, domain_loss_coef=0.0, cycle_loss_coef=0.3)
    model = types.SimpleNamespace(device="cpu")
    term = types.SimpleNamespace(task_id=4)
    for k, (mode, uid) in enumerate((("pairwise-diff", 0), ("aleatoric", 1), ("ensemble_std", 2))):
        d = MOBODYEnsembleDynamics(cfg, model, None, None, term, penalty_coef=0.1, uncertainty_mode=mode)
        assert d._uncertainty_mode == mode and d._unc_id == uid == k
    assert MOBODYEnsembleDynamics(cfg, model, None, None, term)._unc_id == 0
    for bad in ("pairwise", "std", "", "Aleatoric"):
        with pytest.raises(ValueError, match="aleatoric.*ensemble_std.*pairwise-diff"):
            MOBODYEnsembleDynamics(cfg, model, None, None, term, uncertainty_mode=bad)
