"""Open-loop model error over recorded trajectories on the device (`mobody_ens_replay`,
MOBODYEnsembleDynamics.open_loop_error, the CLI's `model_error_*` keys).

The reference is the COMPOSITION of the entry points the parent build already has, with the same seed and call ids: a host
gather from the data -> `mobody_ens_step` (alive = NULL, use_penalty = 0) -> the accounting of tests/open_loop_ref.py on the
host.  Everything but `obs_err` has to carry the composition's bits; `obs_err` is sqrtf of a sequential fp32 sum, and the
build's sqrtf is the correctly rounded one (v_sqrt_f32 plus the one-ulp fix-up), so it is held to `np.sqrt` of the restated
fp32 sum exactly as well."""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import open_loop_ref as ref
from test_hip_mirror import make_dynamics
from test_hip_model_eval import MODELS, TASKS, dyn_kw, dyn_params, setup

pytestmark = pytest.mark.gpu

ELITES, SEED, CALL0 = (0, 2, 3, 5, 6), 21, 7
N_DATA = 300
RATIOS = {}
_data = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_OPEN_LOOP_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst err / bound over the elements, tests/test_hip_open_loop.py: obs_err against fp64 of the same fp32 "
                               "inputs and against the mirror's model_error, bound (S + 4) 2^-24 value; squared reward error against "
                               "the mirror's, bound 4 2^-24 value", "cases": RATIOS}, f, indent=1, sort_keys=True)


def bits(x):
    return np.ascontiguousarray(x).view(np.int32 if np.asarray(x).dtype == np.float32 else np.uint8)


def dataset(tag, dev):
    """N_DATA recorded-looking rows near the model's alive box: (NumPy dict, ring view, five-array view), built once."""
    from mobody_amd import ops
    if tag not in _data:
        S, A, task = MODELS[tag][:3]
        rng = np.random.default_rng(11)
        st = gu.gi.walker_like_obs(rng, N_DATA, S)
        if task == 3:
            st[:, 0] = 0.6
        d = dict(state=st, action=rng.uniform(-1, 1, (N_DATA, A)).astype(np.float32),
                 next_state=(st + 0.05 * rng.standard_normal((N_DATA, S))).astype(np.float32),
                 reward=rng.standard_normal(N_DATA).astype(np.float32), not_done=(rng.random(N_DATA) < 0.8).astype(np.float32))
        store = torch.zeros(N_DATA, ops.ring_pitch(S, A), dtype=torch.float32, device=dev)
        ring = ops.RingView(store, S, A)
        five = []
        for view, k in zip(ring.fields(), ("state", "action", "next_state", "reward", "not_done")):
            t = torch.from_numpy(d[k].reshape(N_DATA, -1)).to(dev)
            view.copy_(t)
            five.append(t.contiguous())
        _data[tag] = (d, ring, tuple(five))
    return _data[tag]


def windows(B, H, seed=0):
    """B window starts inside the data; the last one reaches the last data row (row0 + H == N_DATA) and does not pass it."""
    row0 = np.random.default_rng(seed).integers(0, N_DATA - H + 1, B).astype(np.int64)
    row0[-1] = N_DATA - H
    return row0


def compose(tag, mfma, dev, row0, H, K, mode=0, use_trg=True, data_rows=N_DATA):
    """The composition.  Returns (tables [H][B], final obs_state, final act_state, the model's obs' per step)."""
    from mobody_amd import ops
    S, A, task = MODELS[tag][:3]
    m = setup(tag, mfma, dev)[0]
    d = dataset(tag, dev)[0]
    nexts = []

    def step(t, obs, act):
        r = ops.dyn_step(m.packed(), S, A, task, torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), alive=None,
                         elites=ELITES, seed=SEED, call=CALL0 + t, use_penalty=False, use_trg=use_trg, **dyn_kw(m, mfma, mode))
        nexts.append(r["next_obs"].cpu().numpy())
        return (nexts[-1], r["raw_reward"].cpu().numpy().reshape(-1), r["penalty"].cpu().numpy().reshape(-1),
                r["terminal"].cpu().numpy().reshape(-1) != 0)

    tab, obs, act = ref.replay(d, row0, data_rows, H, K, step)
    return tab, obs, act, nexts


def fused(tag, mfma, dev, row0, H, K, mode=0, use_trg=True, five=False, call0=CALL0, call_dev=None, data_rows=N_DATA):
    from mobody_amd import ops
    S, A, task = MODELS[tag][:3]
    m = setup(tag, mfma, dev)[0]
    _, ring, arrays = dataset(tag, dev)
    state = ops.replay_state(len(row0), H, S, A, dev)
    for v in state.values():                              # the call has to set every word
        v.view(torch.uint8).fill_(0xA5)
    kw = dyn_kw(m, mfma, mode)
    ops.ens_replay(m.packed(), S, A, task, arrays if five else ring, data_rows, torch.from_numpy(row0).to(dev), H, ELITES, SEED,
                   call0, state, reset_every=K, use_trg=use_trg, dyn_planes=kw["planes"], precision=mfma, mopo=kw["mopo"],
                   uncertainty_mode=mode, call_dev=call_dev)
    return {k: v.cpu().numpy() for k, v in state.items()}


def assert_bits(got, want):
    """The fused tables and row state == the composition's, bit for bit (obs_err included: a correctly rounded sqrtf)."""
    tab, obs, act = want[:3]
    for k in ("rew_err", "penalty", "obs_err"):
        assert got[k].shape == tab[k].shape and np.array_equal(bits(got[k]), bits(tab[k])), k
    assert np.array_equal(got["term_model"] != 0, tab["term_model"]) and set(np.unique(got["term_model"])) <= {0, 1}
    assert np.array_equal(bits(got["obs_state"]), bits(obs)) and np.array_equal(bits(got["act_state"]), bits(act))
    # within one ulp of np.sqrt of the restated sum whatever the sqrtf: implied by the equality above, stated for the record
    ulp = np.spacing(np.abs(tab["obs_err"]))
    assert (np.abs(got["obs_err"].astype(np.float64) - tab["obs_err"].astype(np.float64)) <= ulp).all()


# ---- 1. bit for bit against the composition ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("tag", list(MODELS))
def test_fused_replay_equals_the_composition_bit_for_bit(tag, B, mfma, dev):
    for H in (1, 5):
        row0 = windows(B, H)
        assert row0[-1] + H == N_DATA
        seen = []
        for K in (0, 1, 2):
            want = compose(tag, mfma, dev, row0, H, K)
            assert np.isfinite(want[0]["obs_err"]).all() and (want[0]["obs_err"] > 0).all()
            assert_bits(fused(tag, mfma, dev, row0, H, K), want)
            seen.append(want[0]["obs_err"])
        if H == 5:                                         # the reset rule reaches the tables: the three curves differ
            assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[1], seen[2])
            assert np.array_equal(seen[0][:2], seen[2][:2]) and np.array_equal(seen[0][0], seen[1][0])


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_replay_in_the_other_uncertainty_modes(mode, mfma, dev):
    row0 = windows(65, 5)
    want = compose("walker", mfma, dev, row0, 5, 2, mode=mode)
    base = compose("walker", mfma, dev, row0, 5, 2, mode=0)
    assert not np.array_equal(want[0]["penalty"], base[0]["penalty"])           # the mode reaches the penalty ...
    assert np.array_equal(want[0]["rew_err"], base[0]["rew_err"])               # ... and only the penalty
    assert_bits(fused("walker", mfma, dev, row0, 5, 2, mode=mode), want)


def test_source_encoder_five_array_view_call_word_and_zero_horizon(mfma, dev):
    row0 = windows(65, 5)
    want = compose("walker", mfma, dev, row0, 5, 0)
    src = compose("walker", mfma, dev, row0, 5, 0, use_trg=False)
    assert not np.array_equal(src[0]["rew_err"], want[0]["rew_err"])
    assert_bits(fused("walker", mfma, dev, row0, 5, 0, use_trg=False), src)
    assert_bits(fused("walker", mfma, dev, row0, 5, 0, five=True), want)                        # pitch == 0
    word = torch.tensor([3], dtype=torch.int64, device=dev)                                        # call id = call0 + t + call_dev[0]
    assert_bits(fused("walker", mfma, dev, row0, 5, 0, call0=CALL0 - 3, call_dev=word), want)
    other = fused("walker", mfma, dev, row0, 5, 0, call0=CALL0 + 1)
    assert not np.array_equal(other["obs_err"], want[0]["obs_err"])                                # another call id: another draw
    d = dataset("walker", dev)[0]
    got = fused("walker", mfma, dev, row0, 0, 0)                                                   # H == 0: only the row state
    assert np.array_equal(got["obs_state"], d["state"][row0]) and np.array_equal(got["act_state"], d["action"][row0])
    assert got["obs_err"].shape == (0, 65)


def test_windows_that_leave_the_data_are_clamped_to_the_last_row(mfma, dev):
    """row0 is not checked on the host; the kernels clamp r = min(row0 + t, data_rows - 1) (and the action's row likewise), so
    a window that runs past the end compares against the last row again and no load leaves the view.  data_rows = 200 of
    the 300 allocated rows: whatever the clamp did, every load stays inside the allocation."""
    rows = 200
    row0 = np.array([rows - 2, rows - 1, 0, rows - 5], np.int64)
    for K in (0, 2):
        assert_bits(fused("walker", mfma, dev, row0, 5, K, data_rows=rows), compose("walker", mfma, dev, row0, 5, K, data_rows=rows))


# ---- 2. self-consistency, independent of the restatement ------------------------------------------------------------
def make_policy(dev, tag="walker", graph=0, **over):
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    S, A, task, mopo, _ = MODELS[tag]
    torch.manual_seed(3)
    cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, mopo=int(mopo), **over)
    pol = MOBODY(cfg, dev)
    pa, _, _ = gu.policy_params(301, S, A)
    pol.policy.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    pol.dynamics = make_dynamics(dyn_params(tag), S, A, TASKS[task], dev, cfg, rng="device", seed=13)
    return pol


def buffer_of(rows, S, A, dev):
    from mobody_amd.algo import utils
    buf = utils.ReplayBuffer(S, A, dev, max_size=rows["observations"].shape[0], rng="device", seed=5)
    buf.convert_D4RL(rows)
    return buf


@pytest.mark.parametrize("tag", ["walker", "mopo_walker"])
def test_a_dataset_recorded_from_the_model_replays_with_zero_error(tag, mfma, dev):
    from mobody_amd.algo.dynamics.mobody_dynamics import MODEL_EVAL_SEED, OPEN_LOOP_SEED
    assert OPEN_LOOP_SEED != MODEL_EVAL_SEED
    S, A, task = MODELS[tag][:3]
    B, H = 65, 5
    pol = make_policy(dev, tag)
    dyn = pol.dynamics
    rng = np.random.default_rng(2)
    obs = torch.from_numpy(gu.gi.walker_like_obs(rng, B, S)).to(dev)
    acts = torch.from_numpy(rng.uniform(-1, 1, (H, B, A)).astype(np.float32)).to(dev)
    rec = {k: [] for k in ("observations", "actions", "next_observations", "rewards", "terminals")}
    for t in range(H):                                    # the composition's own obs', raw reward and flags at the call's ids
        r = dyn.step_device(obs, acts[t], use_penalty=False, call=1 + t, seed_offset=OPEN_LOOP_SEED)
        for k, v in zip(rec, (obs, acts[t], r["next_obs"], r["raw_reward"].reshape(-1), r["terminal"].reshape(-1) != 0)):
            rec[k].append(v)
        obs = r["next_obs"]
    # window b occupies rows b * H .. b * H + H - 1 of the dataset
    rows = {k: torch.stack(v, dim=1).reshape((B * H,) + tuple(v[0].shape[1:])).cpu().numpy() for k, v in rec.items()}
    print(f"recorded from the model {tag} {mfma}: share of terminal rows {rows['terminals'].mean():.3f}")
    buf = buffer_of(rows, S, A, dev)
    row0 = np.arange(B, dtype=np.int64) * H
    runs = []
    for K in (0, 1, 2):
        dyn._replay_calls = 0                              # the same call ids for the three forms
        out = pol.open_loop_error(buf, row0 if K else torch.from_numpy(row0).to(dev), H, reset_every=K)
        assert dyn._replay_calls == H and dyn._calls == 0
        assert out["obs_err"].shape == (H, B) and out["term_model"].dtype == torch.bool
        assert torch.equal(out["obs_err"], torch.zeros_like(out["obs_err"])) and torch.equal(out["rew_err"], torch.zeros_like(out["rew_err"]))
        assert torch.equal(out["term_agree"], torch.ones(H, device=dev))
        assert torch.equal(out["obs_err_mean"], torch.zeros(H, device=dev)) and torch.equal(out["rew_mse"], torch.zeros(H, device=dev))
        assert torch.equal(out["term_model"].T.reshape(-1).cpu(), torch.from_numpy(rows["terminals"]))
        runs.append(out)
    for other in runs[1:]:
        for k in ("obs_err", "rew_err", "penalty", "term_model"):
            assert torch.equal(runs[0][k].view(torch.uint8), other[k].view(torch.uint8)), k
    # a second call is a new draw (a call counter of its own): the recorded outcome is no longer met
    again = pol.open_loop_error(buf, row0, H)
    assert dyn._replay_calls == 2 * H and not torch.equal(again["obs_err"], torch.zeros_like(again["obs_err"]))
    # windows that leave the buffer are refused on the host
    for bad in (np.array([-1]), np.array([B * H - H + 1]), np.array([0.5])):
        with pytest.raises(ValueError):
            pol.open_loop_error(buf, bad, H)
    assert dyn._replay_calls == 2 * H


# ---- 3. H = 1 against the mirror's model_error ------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["walker", "ant"])
def test_one_step_against_the_mirrors_model_error(tag, mfma, dev):
    """obs_err[0] against model_error's `obs_mse_individual` on the same rows and draws: torch's sum order differs from the
    sequential one, both within (S - 1 adds + subtraction + square + sqrt) roundings of the exact value --
    |d| <= (S + 4) 2^-24 value.  The squared reward error: one subtraction and one square on each side, 4 2^-24 relative.
    Measured worst err / bound: profiles/open_loop_bounds.json (set MOBODY_OPEN_LOOP_BOUNDS_JSON=<path> to rewrite)."""
    from mobody_amd.algo.dynamics.mobody_dynamics import OPEN_LOOP_SEED
    S, A, task = MODELS[tag][:3]
    B = 257
    dyn = make_dynamics(dyn_params(tag), S, A, TASKS[task], dev, gu.policy_cfg(S, A, rng="device", seed=7), rng="device", seed=13)
    d = dataset(tag, dev)[0]
    buf = buffer_of(dict(observations=d["state"], actions=d["action"], next_observations=d["next_state"], rewards=d["reward"],
                         terminals=1.0 - d["not_done"]), S, A, dev)
    row0 = windows(B, 1, seed=3)
    out = dyn.open_loop_error(buf, row0, 1)
    idx = torch.from_numpy(row0).to(dev)
    step = dyn.step_device
    dyn.step_device = lambda o, a, pen: step(o, a, pen, call=1, seed_offset=OPEN_LOOP_SEED)       # model_error at the call's draw
    err = dyn.model_error(buf.state[idx], buf.action[idx], buf.next_state[idx], buf.reward[idx])
    r = dyn.step_device(buf.state[idx].contiguous(), buf.action[idx].contiguous(), False)
    dyn.step_device = step
    want = err["obs_mse_individual"].double().cpu().numpy()
    got = out["obs_err"][0].double().cpu().numpy()
    ratio = np.abs(got - want) / ((S + 4) * 2.0 ** -24 * want)
    sq_want = ((buf.reward[idx].reshape(-1) - r["reward"].reshape(-1)) ** 2).double().cpu().numpy()
    sq_got = (out["rew_err"][0] ** 2).double().cpu().numpy()
    sq_ratio = np.abs(sq_got - sq_want) / (4 * 2.0 ** -24 * sq_want)
    RATIOS[f"model_error-obs-{tag}-B{B}-{mfma}"] = float(ratio.max())
    RATIOS[f"model_error-reward-{tag}-B{B}-{mfma}"] = float(sq_ratio.max())
    print(f"H=1 against model_error {tag} {mfma}: obs worst err/bound {ratio.max():.4f}, reward^2 worst err/bound {sq_ratio.max():.4f}")
    assert (want > 0).all() and (sq_want > 0).all()
    assert (ratio <= 1.0).all() and (sq_ratio <= 1.0).all(), (ratio.max(), sq_ratio.max())
    assert float(out["obs_err_mean"][0]) == pytest.approx(float(err["obs_mse"]), rel=1e-5)
    assert float(out["rew_mse"][0]) == pytest.approx(float(err["reward_mse"]), rel=1e-5)
    rec = (1.0 - d["not_done"][row0]) != 0
    assert float(out["term_agree"][0]) == pytest.approx(float(np.mean(out["term_model"][0].cpu().numpy() == rec)))


# ---- 4. obs_err against fp64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(MODELS))
def test_obs_err_against_fp64(tag, mfma, dev):
    """sqrt(sum_d (a_d - b_d)^2) in fp32: one rounding per subtraction (doubled by the square) and one per square, 3 2^-24
    relative on every term, all terms non-negative; S - 1 adds, each 2^-24 of a partial sum no larger than the total; the
    square root halves the relative error and adds its own rounding: (3 + S - 1) / 2 + 1 <= S + 4 units of 2^-24,
    relative, per element.  The fp64 value is formed from the same fp32 obs' (the composition's) and the same data."""
    S = MODELS[tag][0]
    B, H = 257, 5
    row0 = windows(B, H, seed=5)
    _, _, _, nexts = compose(tag, mfma, dev, row0, H, 0)
    got = fused(tag, mfma, dev, row0, H, 0)["obs_err"].astype(np.float64)
    d = dataset(tag, dev)[0]
    want = np.stack([ref.obs_err_f64(nexts[t], d["next_state"][ref.data_row(row0, t, N_DATA)]) for t in range(H)])
    ratio = np.abs(got - want) / ((S + 4) * 2.0 ** -24 * want)
    RATIOS[f"fp64-{tag}-B{B}-H{H}-{mfma}"] = float(ratio.max())
    print(f"obs_err against fp64 {tag} B={B} H={H} {mfma}: worst err/bound {ratio.max():.4f}")
    assert (want > 0).all() and (ratio <= 1.0).all(), ratio.max()


# ---- 5. training is untouched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_a_replay_between_train_steps_changes_nothing(graph, mfma, dev):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    S, A, task = MODELS["walker"][:3]
    row0 = np.arange(0, 330, 10, dtype=np.int64)

    def run(measure):
        pol = make_policy(dev, graph=graph, penalty_type="par")
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, TASKS[task], 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, TASKS[task], 1)
        out = None
        for t in range(10):
            pol.train(src, tar, 64, None, None)
            if measure and t == 4:
                out = pol.open_loop_error(tar, row0, 5)
        torch.cuda.synchronize()
        return pol, src, tar, out

    a, asrc, atar, out = run(True)
    b, bsrc, btar, _ = run(False)
    assert out is not None and bool(torch.isfinite(out["obs_err"]).all()) and a.dynamics._replay_calls == 5
    if graph:
        assert a._graph is not None and b._graph is not None
    same = lambda x, y: torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for n in ("q_funcs", "target_q_funcs", "policy", "v_func"):
        assert same(getattr(a, n).blob, getattr(b, n).blob) and same(getattr(a, n).blob_T, getattr(b, n).blob_T), n
    for oa, ob in zip(a._opts(), b._opts()):
        assert same(oa.m, ob.m) and same(oa.v, ob.v) and oa.t == ob.t
    assert a._ctr.tolist() == b._ctr.tolist() and a.total_it == b.total_it == 10
    assert a.dynamics._calls == b.dynamics._calls and a.dynamics._train_calls == b.dynamics._train_calls
    assert a.dynamics._eval_calls == b.dynamics._eval_calls == 0
    fa, fb = a.fake_replay_buffer, b.fake_replay_buffer
    assert fa.ptr_size.tolist() == fb.ptr_size.tolist() and fa.size > 0 and same(fa.store, fb.store)
    assert same(asrc.store, bsrc.store) and same(atar.store, btar.store)
    assert (asrc._draws, atar._draws, fa._draws) == (bsrc._draws, btar._draws, fb._draws)
    assert a.losses() == b.losses()


# ---- 6. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_logs_the_open_loop_error_only_when_asked(tmp_path, capsys):
    from mobody_amd import train_mobody as tm
    rng = np.random.default_rng(5)
    S, A, n, m, ep = 17, 6, 3000, 401, 50
    mu = np.zeros(S, np.float32); mu[0] = 1.25
    obs = (mu + 0.1 * rng.standard_normal((n, S))).astype(np.float32)
    np.savez(tmp_path / "src.npz", observations=obs, actions=rng.uniform(-1, 1, (n, A)).astype(np.float32),
             next_observations=(obs + 0.01 * rng.standard_normal((n, S))).astype(np.float32),
             rewards=rng.standard_normal(n).astype(np.float32), terminals=np.zeros(n, bool))
    # the target file holds raw arrays: transition i is (obs[i], obs[i + 1]), so its rows are contiguous by construction and
    # a terminal every 50 rows cuts them into episodes of 50
    tobs = (mu + 0.02 * np.cumsum(rng.standard_normal((m, S)), axis=0) / np.sqrt(m)).astype(np.float32)
    term = np.zeros(m, bool); term[ep - 1::ep] = True
    np.savez(tmp_path / "tar.npz", observations=tobs, actions=rng.uniform(-1, 1, (m, A)).astype(np.float32),
             rewards=rng.standard_normal((m, 1)).astype(np.float32), terminals=term, timeouts=np.zeros(m, bool))
    os.makedirs(tmp_path / "dyn" / "walker2d-friction", exist_ok=True)

    def run(name, extra, train, policy="MOBODY"):
        params = dict(batch_size=64, max_step=12, eval_freq=10, **extra)
        tm.main(["--policy", policy, "--env", "walker2d_friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                 "--synthetic", "0", "--src_data", str(tmp_path / "src.npz"), "--tar_data", str(tmp_path / "tar.npz"),
                 "--rng", "device", "--penalty_type", "none", "--src_rollout_batch_size", "500", "--trg_rollout_batch_size", "200",
                 "--train_dynamics", str(train), "--dynamics_max_epochs", "1", "--dynamics_path", str(tmp_path / "dyn"),
                 "--max_step", "12", "--params", json.dumps(params), "--log_every", "6", "--dir", str(tmp_path / name),
                 "--eval_freq", "10"])
        path = tmp_path / name / policy / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "tb" / "scalars.csv"
        return [l.strip().split(",") for l in open(path)][1:]

    keys = dict(model_error_horizon=7, model_error_windows=32)
    tags = [f"test/open-loop {what} h{k}" for k in (1, 2, 5, 7) for what in ("obs error", "reward mse", "term agree")]
    tags.append("test/one-step obs error")
    first = run("first", keys, 1)                          # pre-trains the ensemble (one epoch) and saves it; the next two load it
    on = run("on", keys, 0)
    off = run("off", {}, 0)
    for rows in (first, on):
        logged = {r[0]: r for r in rows if r[0].startswith("test/open-loop") or r[0].startswith("test/one-step")}
        assert sorted(logged) == sorted(tags) and len([r for r in rows if r[0] in tags]) == len(tags)      # once per tag ...
        assert all(int(r[1]) == 10 for r in logged.values())                                                # ... at the eval cadence
        assert all(np.isfinite(float(r[2])) for r in logged.values())
        assert all(0.0 <= float(r[2]) <= 1.0 for t, r in logged.items() if "term agree" in t)
        assert all(float(r[2]) >= 0.0 for r in logged.values())
    assert not [r for r in off if r[0].startswith("test/open-loop") or r[0].startswith("test/one-step")]
    assert [r for r in on if r[0] not in tags] == off                                                       # the other rows are identical
    assert [r for r in off if r[0] == "test/model error next_obs"]
    # a horizon longer than every episode: the run ends at start-up, naming the longest run
    with pytest.raises(ValueError) as e:
        run("long", dict(model_error_horizon=ep + 1), 0)
    assert f"longest run of contiguous rows is {ep}" in str(e.value)
    assert not os.path.exists(tmp_path / "long")
    # a model-free baseline has no model: the keys are ignored with one printed line
    capsys.readouterr()
    run("bc", keys, 0, policy="TD3_BC")
    assert capsys.readouterr().out.count("model_error_horizon / model_error_windows ignored") == 1
