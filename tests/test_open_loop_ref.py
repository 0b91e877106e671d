"""Open-loop model error over recorded trajectories, the parts that need no GPU: the C ABI of `mobody_ens_replay`
(declared, bound, exported, refusals before any runtime call), the CLI's window helper, the NumPy restatement of the
accounting on hand-made tables, and the merged config staying as it is without the two optional keys."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import open_loop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000          # a non-NULL pointer value: only compared with NULL before the refusal under test
ENTRY = "mobody_ens_replay"
POINTERS = ("dyn_blob", "data", "row0", "elites", "obs_state", "act_state", "obs_err", "rew_err", "penalty", "term_model", "workspace")
DATA_POINTERS = ("state", "action", "next_state", "reward")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _header():
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


# ---- ABI contract --------------------------------------------------------------------------------------------------
def test_abi_declares_binds_and_exports_the_entry_points(lib):
    from mobody_amd import _lib
    hdr = re.sub(r"\s+", " ", _header())
    assert "int64_t mobody_ens_replay_workspace(const MobodyEnsReplay* a);" in hdr
    assert "int mobody_ens_replay(const MobodyEnsReplay* a, void* stream);" in hdr
    assert "typedef struct MobodyEnsReplay MobodyEnsReplay;" in hdr
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7
    assert _lib.PROTOTYPES["mobody_ens_replay_workspace"] == (C.c_int64, [C.POINTER(_lib.MobodyEnsReplay)])
    assert _lib.PROTOTYPES["mobody_ens_replay"] == (C.c_int, [C.POINTER(_lib.MobodyEnsReplay), C.c_void_p])
    assert hasattr(lib, "mobody_ens_replay") and hasattr(lib, "mobody_ens_replay_workspace")


def test_block_fields_match_the_header_in_order_and_size():
    from mobody_amd import _lib
    body = re.search(r"struct MobodyEnsReplay \{(.*?)\};", _header(), flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", part).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]
    assert names == [f[0] for f in _lib.MobodyEnsReplay._fields_]
    assert names[:2] == ["struct_bytes", "uncertainty_mode"] and names[-1] == "workspace"
    assert names == ["struct_bytes", "uncertainty_mode", "dyn_blob", "dyn_planes", "mopo_blob", "mopo_blob_T", "precision", "S", "A",
                     "task", "data", "data_rows", "row0", "B", "H", "reset_every", "n_elites", "elites", "seed", "call0", "call_dev",
                     "use_trg", "obs_state", "act_state", "obs_err", "rew_err", "penalty", "term_model", "workspace"]
    # 2 int32 | 4 pointers | 4 int32 | pointer | int64 | pointer | int64 | 3 int32 + pad | pointer | 2 uint32 | pointer |
    # int32 + pad | 7 pointers
    assert C.sizeof(_lib.MobodyEnsReplay) == 8 + 32 + 16 + 8 + 8 + 8 + 8 + 16 + 8 + 8 + 8 + 8 + 56


# ---- refusals: MOBODY_E_ARG before any runtime call, device pointers never dereferenced ------------------------------
def _good(_lib, view=None, **over):
    """A block that passes every check (nothing may be launched with it: its device pointers are fake).  `data` is a real
    host struct, as the ABI asks; the block keeps it alive."""
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    v = dict(state=PTR, action=PTR, next_state=PTR, reward=PTR, not_done=PTR, pitch=48)
    v.update(view or {})
    view = _lib.MobodyBufferView(**v)
    f = dict(struct_bytes=C.sizeof(_lib.MobodyEnsReplay), uncertainty_mode=0, precision=0, S=17, A=6, task=4, data=C.pointer(view),
             data_rows=100, B=4, H=1, reset_every=0, n_elites=5, elites=el, seed=1, call0=1, use_trg=1)
    f.update({k: PTR for k in POINTERS if k not in ("elites", "data")})
    f.update(over)
    blk = _lib.MobodyEnsReplay(**f)
    blk._keep = (view, el)
    return blk


def _refused(lib, blk, *words):
    assert lib.mobody_ens_replay(C.byref(blk), None) == -1
    msg = lib.mobody_last_error().decode()
    assert msg.startswith(ENTRY + ":"), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


@pytest.mark.parametrize("over,words", [
    (dict(struct_bytes=8), ("struct_bytes", "sizeof(MobodyEnsReplay)")),
    (dict(B=-1), ("B < 0",)),
    (dict(H=-1), ("H < 0",)),
    (dict(reset_every=-1), ("reset_every < 0",)),
    (dict(uncertainty_mode=3), ("uncertainty_mode 3",)),
    (dict(uncertainty_mode=-1), ("uncertainty_mode",)),
    (dict(data_rows=0), ("data_rows",)),
    (dict(data_rows=-5), ("data_rows",)),
    (dict(n_elites=0), ("n_elites",)),
    (dict(n_elites=8), ("n_elites",)),
    (dict(task=7), ("task",)),
    (dict(task=-1), ("task",)),
    (dict(task=6), ("task", "S > 26")),                                     # the pen predicate reads coordinate 26
    (dict(precision=5), ("precision 5",)),
    (dict(precision=-1), ("precision",)),
    (dict(precision=4), ("planes",)),                                        # split precision without the ensemble's planes
    (dict(precision=4, dyn_planes=PTR, mopo_blob=PTR), ("mopo_blob_T",)),
])
def test_refusals_name_the_field(lib, over, words):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **over), *words)


@pytest.mark.parametrize("field", POINTERS)
def test_every_null_pointer_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **{field: None}), "null pointer", field)


@pytest.mark.parametrize("field", DATA_POINTERS)
def test_every_null_field_of_the_view_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, view={field: None}), "null pointer", "data", field)


@pytest.mark.parametrize("pitch", [-1, 1, 17, 2 * 17 + 6 + 1])
def test_a_pitch_that_cannot_hold_a_row_is_refused(lib, pitch):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, view=dict(pitch=pitch)), "pitch")


def test_refusal_edges_that_are_not_errors(lib):
    from mobody_amd import _lib
    # B == 0 returns 0 whatever the pointers and data_rows are; not_done is never read, so a null one passes
    none = {k: None for k in POINTERS}
    assert lib.mobody_ens_replay(C.byref(_good(_lib, B=0, data_rows=0, **none)), None) == 0
    assert "not_done" not in _refused(lib, _good(_lib, view=dict(not_done=None), n_elites=0), "n_elites")
    # the four tables are written only when H > 0: with H == 0 null ones get past the pointer checks
    tables = dict(obs_err=None, rew_err=None, penalty=None, term_model=None)
    assert "null pointer" not in _refused(lib, _good(_lib, H=0, n_elites=0, **tables), "n_elites")
    _refused(lib, _good(_lib, H=0, obs_state=None), "null pointer", "obs_state")
    # both storage forms get past the pitch check: the smallest ring pitch and the five-array form
    for pitch in (0, 2 * 17 + 6 + 2, lib.mobody_ring_pitch(17, 6)):
        assert "pitch" not in _refused(lib, _good(_lib, view=dict(pitch=pitch), n_elites=0), "n_elites")
    assert lib.mobody_ens_replay(None, None) == -1 and lib.mobody_last_error().decode().startswith(ENTRY + ":")
    assert lib.mobody_ens_replay_workspace(C.byref(_good(_lib, struct_bytes=8))) == -1
    assert lib.mobody_last_error().decode().startswith("mobody_ens_replay_workspace:")
    # the workspace holds at least the next observation, the penalty and the step's own workspace
    need = lib.mobody_ens_replay_workspace(C.byref(_good(_lib, B=33)))
    assert need >= 33 * (17 + 1) + lib.mobody_dyn_step_workspace(17, 6, 33)


# ---- the CLI's window helper ----------------------------------------------------------------------------------------
def _dataset():
    """Ten rows of one continuous trajectory with two terminals (rows 3 and 7 start episodes) and one discontinuity (row 5
    starts one, no terminal before it): episodes of 3, 2, 2 and 3 rows."""
    obs = np.arange(10, dtype=np.float32).reshape(10, 1) * np.ones((1, 3), np.float32)
    nxt = obs + 1.0
    term = np.zeros(10, bool)
    term[2] = term[6] = True
    obs[5:] += 100.0; nxt[5:] += 100.0
    return obs, nxt, term


def test_open_loop_windows_on_a_hand_made_dataset():
    from mobody_amd import train_mobody as tm
    obs, nxt, term = _dataset()
    starts = tm.episode_starts(obs, nxt, term)
    assert starts.tolist() == [0, 3, 5, 7]
    state = np.random.get_state()[1].copy()
    # fewer valid starts than asked for: all of them, sorted
    assert tm.open_loop_windows(starts, 10, 1, 64, seed=1).tolist() == list(range(10))
    assert tm.open_loop_windows(starts, 10, 2, 64, seed=1).tolist() == [0, 1, 3, 5, 7, 8]
    assert tm.open_loop_windows(starts, 10, 3, 64, seed=1).tolist() == [0, 7]
    assert tm.open_loop_windows(starts, 10, 3, 2, seed=1).tolist() == [0, 7]
    # the last rows of the data: a window may reach the last row and never passes it
    assert tm.open_loop_windows(starts, 9, 3, 64, seed=1).tolist() == [0] and tm.open_loop_windows(starts, 9, 2, 64, seed=1).tolist() == [0, 1, 3, 5, 7]
    # enough: `count` distinct valid starts, sorted, the same for the same seed and others for another
    valid = [0, 1, 3, 5, 7, 8]
    picks = [tm.open_loop_windows(starts, 10, 2, 3, seed=s) for s in range(8)]
    for p in picks:
        assert p.shape == (3,) and len(set(p.tolist())) == 3 and set(p.tolist()) <= set(valid) and p.tolist() == sorted(p.tolist())
    assert np.array_equal(picks[1], tm.open_loop_windows(starts, 10, 2, 3, seed=1))
    assert len({tuple(p.tolist()) for p in picks}) > 1
    assert np.array_equal(state, np.random.get_state()[1])                                  # the global stream is not consumed
    # its generator is not model_eval_rows's: the same seed over the same candidates picks differently somewhere
    every = np.arange(400)                           # every row starts an episode: with horizon 1 every row is a candidate
    assert any(not np.array_equal(tm.open_loop_windows(every, 400, 1, 5, seed=s), tm.model_eval_rows(every, 5, seed=s)) for s in range(4))
    # no window at all: the error names the longest run
    with pytest.raises(ValueError) as e:
        tm.open_loop_windows(starts, 10, 4, 64, seed=1)
    assert "longest run of contiguous rows is 3" in str(e.value) and "4" in str(e.value)
    with pytest.raises(ValueError) as e:
        tm.open_loop_windows(np.array([0]), 6, 7, 4, seed=1)
    assert "longest run of contiguous rows is 6" in str(e.value)
    with pytest.raises(ValueError):
        tm.open_loop_windows(starts, 10, 0, 4, seed=1)


# ---- accounting (the restatement the GPU tests compare against) -----------------------------------------------------
def _tables():
    f = np.float32
    n = 6
    data = dict(state=np.arange(n, dtype=f).reshape(n, 1) * np.ones((1, 2), f),
                action=10.0 + np.arange(n, dtype=f).reshape(n, 1),
                next_state=1.0 + np.arange(n, dtype=f).reshape(n, 1) * np.ones((1, 2), f),
                reward=np.arange(n, dtype=f) * f(0.5))
    return data, n


def test_reset_rule_action_hand_over_and_clamp_on_hand_made_tables():
    f = np.float32
    data, n = _tables()
    row0 = np.array([0, 2, 3])                       # the last window reaches row 5, the last one, at t = 2 and is clamped at t = 3
    seen = []

    def step(t, obs, act):
        seen.append((t, obs.copy(), act.copy()))
        return obs + f(0.5), act[:, 0] * f(0.25), np.full(obs.shape[0], f(t)), obs[:, 0] > 3.0

    for K in (0, 1, 2, 3):
        del seen[:]
        tab, obs, act = ref.replay(data, row0, n, 4, K, step)
        assert seen[0][1][:, 0].tolist() == [0.0, 2.0, 3.0] and seen[0][2][:, 0].tolist() == [10.0, 12.0, 13.0]
        for t, o, a in seen:
            # the action of step t is the recorded one of row min(row0 + t, n - 1), whatever the state did
            assert a[:, 0].tolist() == (10.0 + np.minimum(row0 + t, n - 1)).tolist(), (K, t)
            if t > 0:
                r_prev = np.minimum(row0 + t - 1, n - 1)
                was_reset = K > 0 and t % K == 0     # (t - 1 + 1) % K == 0
                want = data["next_state"][r_prev] if was_reset else seen[t - 1][1] + f(0.5)
                assert np.array_equal(o, want), (K, t)
        assert np.array_equal(act[:, 0], 10.0 + np.minimum(row0 + 4, n - 1))        # clamped at the last data row
        assert tab["penalty"].tolist() == [[float(t)] * 3 for t in range(4)]
        r = np.minimum(row0[None, :] + np.arange(4)[:, None], n - 1)
        assert np.array_equal(tab["rew_err"], (10.0 + r) * f(0.25) - r * f(0.5))    # signed, against the clamped row
        assert tab["obs_err"].shape == (4, 3) and tab["term_model"].dtype == bool
    # one-step form: every step starts at the recorded state, so the model's `obs + 0.5` is 0.5 short in both coordinates
    tab, _, _ = ref.replay(data, np.array([0, 1]), n, 4, 1, step)
    assert np.array_equal(tab["obs_err"], np.full((4, 2), np.sqrt(f(0.5)), f))
    # open loop: the deficit compounds by 0.5 per step
    tab, _, _ = ref.replay(data, np.array([0, 1]), n, 4, 0, step)
    assert np.allclose(tab["obs_err"][:, 0], [np.sqrt(2 * (0.5 * (t + 1)) ** 2) for t in range(4)])
    # H == 0: the row state alone
    tab, obs, act = ref.replay(data, row0, n, 0, 0, step)
    assert tab["obs_err"].shape == (0, 3) and obs[:, 0].tolist() == [0.0, 2.0, 3.0] and act[:, 0].tolist() == [10.0, 12.0, 13.0]


def test_error_sum_is_sequential_fp32_with_a_float32_sqrt():
    f = np.float32
    # 1 + 2^-24 + 2^-24 stays 1 when summed left to right in fp32 (a pairwise or fp64 sum would reach 1 + 2^-23)
    a = np.array([[1.0, 2.0 ** -12, 2.0 ** -12]], f)
    b = np.zeros((1, 3), f)
    assert ref.sq_sum32(a, b)[0] == f(1.0) and ref.sq_sum32(a[:, ::-1], b)[0] == f(1.0 + 2.0 ** -23)
    # every product is rounded on its own: (1 + 2^-12)^2 loses its 2^-24 before it is added
    x = np.array([[1.0 + 2.0 ** -12]], f)
    assert ref.sq_sum32(x, np.zeros((1, 1), f))[0] == f(1.0 + 2.0 ** -11)
    rng = np.random.default_rng(0)
    m, r = rng.standard_normal((64, 17)).astype(f), rng.standard_normal((64, 17)).astype(f)
    row, _, _ = ref.account(dict(next_state=r, action=np.zeros((64, 1), f), reward=np.zeros(64, f)), np.arange(64), 64, 0, 0,
                            m, np.zeros(64, f), np.zeros(64, f), np.zeros(64, bool))
    assert row["obs_err"].dtype == f and np.array_equal(row["obs_err"], np.sqrt(ref.sq_sum32(m, r)))
    err = np.abs(row["obs_err"].astype(np.float64) - ref.obs_err_f64(m, r))
    assert (err <= (17 + 4) * 2.0 ** -24 * ref.obs_err_f64(m, r)).all()


# ---- CLI pieces ----------------------------------------------------------------------------------------------------
def test_open_loop_error_is_off_by_default_in_the_merged_config():
    from mobody_amd import train_mobody as tm
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "g10b_config_merge.json")))
    argv = ["--policy", "MOBODY", "--env", "walker2d-friction", "--shift_level", "2.0"]
    cfg = tm.build_config(tm.build_parser().parse_args(argv), 17, 6, 1.0)
    today = {k for k, _ in g["update"]} | set(g["yaml"]["mujoco/mobody/walker2d.yaml"]) | {"rng", "seed"}
    assert set(cfg) == today and not {"model_error_horizon", "model_error_windows"} & set(cfg)
    on = tm.build_config(tm.build_parser().parse_args(argv + ["--params", '{"model_error_horizon": 20, "model_error_windows": 64}']), 17, 6, 1.0)
    assert set(on) == today | {"model_error_horizon", "model_error_windows"} and on["model_error_horizon"] == 20
    assert not [a for a in tm.build_parser()._actions if "model_error" in "".join(a.option_strings)]      # no new flag
    assert tm.OPEN_LOOP_STEPS == (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000)
