"""Policy evaluation in the learned model on the device (`mobody_ens_evaluate`, MOBODYEnsembleDynamics.evaluate_policy,
the CLI's `model_eval_*` keys).

The reference is the COMPOSITION of the entry points the parent build already has, with the same seed and call ids:
`ops.mlp3_forward(out_mode 1)` -> `mobody_ens_step` under the carried alive mask -> the accounting of
tests/model_eval_ref.py on the host.  With discount 1 the return is a sequential fp32 sum, so the fused call has to give the
composition's bits; with discount 0.99 it is held to the rounding bound of its 2 H operations against fp64."""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import model_eval_ref as ref
from test_hip_mirror import make_dynamics

pytestmark = pytest.mark.gpu

ELITES, SEED, CALL0 = (0, 2, 3, 5, 6), 21, 7
# (S, A, termination id, mopo, shift of the alive coordinate's output bias).  The shifts were chosen with the CPU oracle's
# step on the same Philox draws so that the 33-row, 5-step case spreads over all five lengths (walker 10/6/6/4/7 rows of
# length 1..5, ant 10/6/4/4/9, mopo 2/9/11/5/6); the tests assert the spread from the composition's own flags.
MODELS = {"walker": (17, 6, 4, False, 0.88), "ant": (111, 8, 3, False, 0.92), "mopo_walker": (17, 6, 4, True, -0.22)}
TASKS = {4: "walker2d-medium-v2", 3: "ant-medium-v2"}
RATIOS = {}
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_MODEL_EVAL_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst |ret - fp64| / (2 H 2^-24 sum_t |0.99^t raw_t|) over the rows, tests/test_hip_model_eval.py",
                       "cases": RATIOS}, f, indent=1, sort_keys=True)


def dyn_params(tag, seed=801):
    S, A, _, mopo, shift = MODELS[tag]
    p = gu.gi.dyn_params(seed, S, A, mopo=mopo)
    p["za_src3.bias" if mopo else "transition3.bias"][:, 0, 0] += np.float32(shift)
    return p


def setup(tag, mfma, dev):
    """(model, actor blob, mlp3_forward keywords) of one (shape, MFMA mode), built once."""
    from mobody_amd import packing
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    if (tag, mfma) not in _cache:
        S, A, _, mopo, _ = MODELS[tag]
        m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=gu.policy_cfg(S, A, mopo=int(mopo)))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in dyn_params(tag).items()}, strict=False)
        pa, _, _ = gu.policy_params(301, S, A)
        actor = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, A, dev)
        _cache[(tag, mfma)] = (m, actor, gu.mlp_kw(actor, S, A, 1, mfma))
    return _cache[(tag, mfma)]


def init_obs(tag, B, dev):
    S, _, task, _, _ = MODELS[tag]
    x = gu.gi.walker_like_obs(np.random.default_rng(4), B, S)
    if task == 3:
        x[:, 0] = 0.6
    return torch.from_numpy(x).to(dev)


def dyn_kw(m, mfma, mode):
    from mobody_amd import ops
    return dict(planes=m.planes() if ops.prec_id(mfma) else None, precision=mfma,
                mopo=m.packed_mopo() if m.mopo else None, uncertainty_mode=mode)


def compose(tag, mfma, dev, init, H, mode=0, discount=1.0, use_trg=True):
    """The composition: per step policy forward, mobody_ens_step under the carried alive mask, host accounting.
    Returns (row state as NumPy, final observation tensor, raw[H][B], terminal[H][B])."""
    from mobody_amd import ops
    S, A, task = MODELS[tag][:3]
    m, actor, akw = setup(tag, mfma, dev)
    st, obs, raws, terms = ref.new_state(init.shape[0]), init, [], []
    for t in range(H):
        act = ops.mlp3_forward(actor, S, A, 1, obs, out_mode=1, max_action=1.0, **akw)[0]
        alive = torch.from_numpy(st["alive"].astype(np.uint8)).to(dev)
        r = ops.dyn_step(m.packed(), S, A, task, obs, act, alive=alive, elites=ELITES, seed=SEED, call=CALL0 + t,
                         use_penalty=False, use_trg=use_trg, **dyn_kw(m, mfma, mode))
        raw, term = r["raw_reward"].cpu().numpy().reshape(-1), r["terminal"].cpu().numpy().reshape(-1) != 0
        raws.append(raw); terms.append(term)
        ref.account(st, raw, r["penalty"].cpu().numpy().reshape(-1), term, discount)
        obs = r["next_obs"]
    return st, obs, np.array(raws), np.array(terms)


def fused(tag, mfma, dev, init, H, mode=0, discount=1.0, use_trg=True, state=None, resume=False, call0=CALL0, call_dev=None):
    from mobody_amd import ops
    S, A, task = MODELS[tag][:3]
    m, actor, akw = setup(tag, mfma, dev)
    if state is None:
        state = ops.eval_state(init.shape[0], S, dev)
        for v in state.values():                          # the first call has to initialise every word
            v.view(torch.uint8).fill_(0xA5)
    kw = dyn_kw(m, mfma, mode)
    ops.ens_evaluate(m.packed(), actor, S, A, task, 1.0, None if resume else init, H, ELITES, SEED, call0, state, use_trg=use_trg,
                     discount=discount, resume=resume, dyn_planes=kw["planes"], actor_blob_T=akw.get("blob_T"), precision=mfma,
                     mopo=kw["mopo"], uncertainty_mode=mode, call_dev=call_dev)
    return state


def assert_state_bits(state, st, obs):
    """The fused row state == the composition's, bit for bit."""
    bits = lambda x: np.ascontiguousarray(x).view(np.int32)
    for k in ("ret", "pen_sum", "disc"):
        assert np.array_equal(bits(state[k].cpu().numpy()), bits(st[k])), k
    assert np.array_equal(state["length"].cpu().numpy(), st["length"])
    assert np.array_equal(state["alive"].cpu().numpy() != 0, st["alive"])
    assert torch.equal(state["obs_state"].view(torch.int32), obs.view(torch.int32))


def lengths_from_flags(terms):
    alive, length = np.ones(terms.shape[1], bool), np.zeros(terms.shape[1], int)
    for t in range(terms.shape[0]):
        length += alive
        alive &= ~terms[t]
    return length


# ---- 1. bit for bit against the composition ------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("tag", list(MODELS))
def test_fused_evaluation_equals_the_composition_bit_for_bit(tag, B, mfma, dev):
    init = init_obs(tag, B, dev)
    for H in (1, 5):
        st, obs, raws, terms = compose(tag, mfma, dev, init, H)
        if (B, H) == (33, 5):                              # the case exercises what it claims (from the composition alone)
            got = set(lengths_from_flags(terms).tolist())
            assert len(got) >= 3 and {1, 5} <= got, got
        assert_state_bits(fused(tag, mfma, dev, init, H), st, obs)
        assert np.array_equal(st["length"], lengths_from_flags(terms)) and np.isfinite(st["ret"]).all()


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_evaluation_in_the_other_uncertainty_modes(mode, mfma, dev):
    init = init_obs("walker", 33, dev)
    st, obs, _, _ = compose("walker", mfma, dev, init, 5, mode=mode)
    st0 = compose("walker", mfma, dev, init, 5, mode=0)[0]
    assert not np.array_equal(st["pen_sum"], st0["pen_sum"])            # the mode reaches the penalty ...
    assert np.array_equal(st["ret"], st0["ret"])                        # ... and only the penalty
    assert_state_bits(fused("walker", mfma, dev, init, 5, mode=mode), st, obs)


def test_source_encoder_and_zero_horizon(mfma, dev):
    init = init_obs("walker", 33, dev)
    st, obs, _, _ = compose("walker", mfma, dev, init, 5, use_trg=False)
    assert not np.array_equal(st["ret"], compose("walker", mfma, dev, init, 5)[0]["ret"])
    assert_state_bits(fused("walker", mfma, dev, init, 5, use_trg=False), st, obs)
    assert_state_bits(fused("walker", mfma, dev, init, 0), ref.new_state(33), init)      # H == 0, resume == 0: only initialises


# ---- 2. resume ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["walker", "mopo_walker"])
def test_resume_continues_the_row_state(tag, mfma, dev):
    init = init_obs(tag, 33, dev)
    one = fused(tag, mfma, dev, init, 5)
    two = fused(tag, mfma, dev, init, 2)
    fused(tag, mfma, dev, init, 3, state=two, resume=True, call0=CALL0 + 2)
    three = fused(tag, mfma, dev, init, 2, call_dev=torch.zeros(1, dtype=torch.int64, device=dev))
    fused(tag, mfma, dev, init, 3, state=three, resume=True, call_dev=torch.tensor([2], dtype=torch.int64, device=dev))
    for other in (two, three):
        for k, v in one.items():
            assert torch.equal(v.view(torch.uint8), other[k].view(torch.uint8)), k
    assert len(set(one["length"].tolist())) >= 3


# ---- 3. the mirror: chunk graph --------------------------------------------------------------------------------------
def make_policy(dev, graph=0, **over):
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    S, A, task = MODELS["walker"][:3]
    torch.manual_seed(3)
    cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, **over)
    pol = MOBODY(cfg, dev)
    pa, _, _ = gu.policy_params(301, S, A)
    pol.policy.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    pol.dynamics = make_dynamics(dyn_params("walker"), S, A, TASKS[task], dev, cfg, rng="device", seed=13)
    return pol


def test_chunk_graph_equals_one_eager_call(mfma, dev):
    pol = make_policy(dev)
    dyn = pol.dynamics
    init = init_obs("walker", 33, dev)
    keys = ("returns", "lengths", "penalty_sums", "alive")

    def run(h, chunk):
        dyn._eval_calls = 0                                # the same call ids for both forms
        return pol.evaluate_in_model(init, h, chunk=chunk)

    def same(a, b):
        return all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in keys)

    eager = run(6, 0)
    assert dyn.eval_captures == 0 and len(set(eager["lengths"].tolist())) >= 3
    graph = run(6, 2)
    assert dyn.eval_captures == 1 and same(eager, graph)
    assert same(eager, run(6, 2)) and dyn.eval_captures == 1           # the same key replays
    assert same(run(5, 0), run(5, 2)) and dyn.eval_captures == 1       # a shorter last chunk runs eagerly
    assert eager["return_mean"] == pytest.approx(float(eager["returns"].mean())) and 1.0 <= eager["length_mean"] <= 6.0
    assert eager["alive_frac"] == pytest.approx(float((eager["alive"] != 0).float().mean()))
    assert eager["penalty_mean"] == pytest.approx(float(eager["penalty_sums"].mean()))
    # a second evaluation is a new draw (a call counter of its own), on a stream that is not the training step's
    assert not same(eager, pol.evaluate_in_model(init, 6, chunk=0)) and dyn._calls == 0
    # other parameters loaded: the model re-packs its blob, the captured pointers are stale, the graph is captured again
    dyn.model.load_state_dict({k: torch.from_numpy(v) for k, v in dyn_params("walker", seed=802).items()}, strict=False)
    other = run(6, 2)
    assert dyn.eval_captures == 2 and not same(eager, other) and same(other, run(6, 0))


# ---- 4. discount 0.99 against fp64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,B", [("walker", 33), ("walker", 257), ("ant", 33), ("mopo_walker", 33)])
def test_discounted_return_against_fp64(tag, B, mfma, dev):
    """ret = fma(disc, raw, ret), disc *= discount: H roundings in disc and H in the sum, each at most 2^-24 relative of a
    partial result no larger than sum_t |disc^t raw_t| -- the bound is 2 H 2^-24 sum_t |0.99^t raw_t| per row.  The fp64
    sum runs over the composition's own rewards and flags with the discount the call receives, float32(0.99).
    Measured worst err / bound: see profiles/model_eval_bounds.json (set MOBODY_MODEL_EVAL_BOUNDS_JSON=<path> to rewrite)."""
    H, disc = 5, float(np.float32(0.99))
    init = init_obs(tag, B, dev)
    st, obs, raws, terms = compose(tag, mfma, dev, init, H, discount=disc)
    state = fused(tag, mfma, dev, init, H, discount=disc)
    want, mag = ref.returns_f64(raws, terms, disc)
    err = np.abs(state["ret"].cpu().numpy().astype(np.float64) - want)
    bound = 2 * H * 2.0 ** -24 * mag
    worst = float(np.max(err / bound))
    RATIOS[f"{tag}-B{B}-H{H}-{mfma}"] = worst
    print(f"discounted return {tag} B={B} H={H} {mfma}: worst err/bound {worst:.4f} (max err {err.max():.3e})")
    assert (mag > 0).all() and (err <= bound).all(), worst
    assert_state_bits(state, st, obs)                      # and the fp32 restatement is met exactly here too
    assert np.array_equal(state["length"].cpu().numpy(), lengths_from_flags(terms))


# ---- 5. training is untouched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_an_evaluation_between_train_steps_changes_nothing(graph, mfma, dev):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    S, A, task = MODELS["walker"][:3]
    init = init_obs("walker", 33, dev)

    def run(evaluate):
        pol = make_policy(dev, graph=graph, penalty_type="par")
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, TASKS[task], 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, TASKS[task], 1)
        ev = None
        for t in range(10):
            pol.train(src, tar, 64, None, None)
            if evaluate and t == 4:
                ev = pol.evaluate_in_model(init, 5, chunk=2)
        torch.cuda.synchronize()
        return pol, src, tar, ev

    a, asrc, atar, ev = run(True)
    b, bsrc, btar, _ = run(False)
    assert ev is not None and a.dynamics.eval_captures == 1 and np.isfinite(ev["return_mean"])
    if graph:
        assert a._graph is not None and b._graph is not None
    same = lambda x, y: torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    for n in ("q_funcs", "target_q_funcs", "policy", "v_func"):
        assert same(getattr(a, n).blob, getattr(b, n).blob) and same(getattr(a, n).blob_T, getattr(b, n).blob_T), n
    for oa, ob in zip(a._opts(), b._opts()):
        assert same(oa.m, ob.m) and same(oa.v, ob.v) and oa.t == ob.t
    assert a._ctr.tolist() == b._ctr.tolist() and a.total_it == b.total_it == 10
    assert a.dynamics._calls == b.dynamics._calls and a.dynamics._train_calls == b.dynamics._train_calls
    fa, fb = a.fake_replay_buffer, b.fake_replay_buffer
    assert fa.ptr_size.tolist() == fb.ptr_size.tolist() and fa.size > 0 and same(fa.store, fb.store)
    assert (asrc._draws, atar._draws, fa._draws) == (bsrc._draws, btar._draws, fb._draws)
    assert a.losses() == b.losses()


# ---- 6. CLI ------------------------------------------------------------------------------------------------------------
def test_cli_logs_the_model_evaluation_only_when_asked(tmp_path, capsys):
    from mobody_amd import train_mobody as tm
    tags = ["test/model target return", "test/model target normalized score", "test/model episode length",
            "test/model penalty", "test/model alive frac"]

    def run(name, extra):
        params = dict(batch_size=64, max_step=12, eval_freq=10, **extra)
        tm.main(["--policy", "MOBODY", "--env", "walker2d_friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                 "--synthetic", "1", "--rng", "device", "--penalty_type", "none", "--src_rows", "4000", "--tar_rows", "500",
                 "--src_rollout_batch_size", "1000", "--trg_rollout_batch_size", "500", "--max_step", "12",
                 "--params", json.dumps(params), "--log_every", "6", "--dir", str(tmp_path / name), "--eval_freq", "10"])
        path = tmp_path / name / "MOBODY" / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "tb" / "scalars.csv"
        return [l.strip().split(",") for l in open(path)][1:]

    on = run("on", dict(model_eval_episodes=64, model_eval_horizon=5))
    off = run("off", {})
    logged = {r[0]: r for r in on if r[0].startswith("test/model ") and "error" not in r[0]}
    assert sorted(logged) == sorted(tags) and all(int(r[1]) == 10 for r in logged.values())      # once, at the eval cadence
    assert not [r for r in off if r[0] in tags]
    assert [r for r in on if r[0] not in tags] == off                                             # the other rows are identical
    assert not [r for r in on + off if r[0] == "test/target return"]                              # the simulator's name stays free
    assert 1.0 <= float(logged["test/model episode length"][2]) <= 5.0
    assert 0.0 <= float(logged["test/model alive frac"][2]) <= 1.0
    from mobody_amd.envs.infos import get_normalized_score
    ret = float(logged["test/model target return"][2])
    if ret == ret:
        assert float(logged["test/model target normalized score"][2]) == pytest.approx(get_normalized_score(ret, "walker2d-friction-2.0"))
    # a model-free baseline has no model: the keys are ignored with one printed line
    capsys.readouterr()
    tm.main(["--policy", "TD3_BC", "--env", "walker2d_friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", "1",
             "--rng", "device", "--src_rows", "4000", "--tar_rows", "500", "--max_step", "2", "--log_every", "1",
             "--params", json.dumps(dict(batch_size=64, max_step=2, eval_freq=2, model_eval_episodes=8)),
             "--dir", str(tmp_path / "bc"), "--eval_freq", "2"])
    out = capsys.readouterr().out
    assert out.count("model_eval_episodes / model_eval_horizon ignored") == 1
