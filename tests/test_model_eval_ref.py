"""Policy evaluation in the learned model, the parts that need no GPU: the C ABI of `mobody_ens_evaluate` (declared,
bound, exported, refusals before any runtime call), the NumPy restatement of its per-row accounting on hand-made tables,
the CLI's episode-start helper, and the merged config staying as it is without the two optional keys."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import model_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000          # a non-NULL pointer value: only compared with NULL before the refusal under test
ENTRY = "mobody_ens_evaluate"
POINTERS = ("dyn_blob", "actor_blob", "init_obs", "elites", "obs_state", "alive", "ret", "pen_sum", "disc", "length", "workspace")


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
    assert "int64_t mobody_ens_evaluate_workspace(const MobodyEnsEval* a);" in hdr
    assert "int mobody_ens_evaluate(const MobodyEnsEval* a, void* stream);" in hdr
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7
    assert _lib.PROTOTYPES["mobody_ens_evaluate_workspace"] == (C.c_int64, [C.POINTER(_lib.MobodyEnsEval)])
    assert _lib.PROTOTYPES["mobody_ens_evaluate"] == (C.c_int, [C.POINTER(_lib.MobodyEnsEval), C.c_void_p])
    assert hasattr(lib, "mobody_ens_evaluate") and hasattr(lib, "mobody_ens_evaluate_workspace")


def test_block_fields_match_the_header_in_order_and_size():
    from mobody_amd import _lib
    body = re.search(r"struct MobodyEnsEval \{(.*?)\};", _header(), flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", part).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]
    assert names == [f[0] for f in _lib.MobodyEnsEval._fields_]
    assert names[:2] == ["struct_bytes", "uncertainty_mode"] and names[-1] == "workspace"
    # 2 int32 | 6 pointers | 4 int32 | pointer | int64 | 2 int32 | pointer | 2 uint32 | pointer | 2 float | 2 int32 | 7 pointers
    assert C.sizeof(_lib.MobodyEnsEval) == 8 + 48 + 16 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 8 + 56


# ---- refusals: MOBODY_E_ARG before any runtime call, pointers never dereferenced ------------------------------------
def _good(_lib, **over):
    """A block that passes every check (nothing may be launched with it: its pointers are fake)."""
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    f = dict(struct_bytes=C.sizeof(_lib.MobodyEnsEval), uncertainty_mode=0, precision=0, S=17, A=6, task=4, B=4, H=1, n_elites=5,
             elites=el, seed=1, call0=1, max_action=1.0, discount=1.0, use_trg=1, resume=0)
    f.update({k: PTR for k in POINTERS if k != "elites"})
    f.update(over)
    return _lib.MobodyEnsEval(**f)


def _refused(lib, blk, *words):
    assert lib.mobody_ens_evaluate(C.byref(blk), None) == -1
    msg = lib.mobody_last_error().decode()
    assert msg.startswith(ENTRY + ":"), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


@pytest.mark.parametrize("over,words", [
    (dict(struct_bytes=8), ("struct_bytes", "sizeof(MobodyEnsEval)")),
    (dict(B=-1), ("B < 0",)),
    (dict(H=-1), ("H < 0",)),
    (dict(uncertainty_mode=3), ("uncertainty_mode 3",)),
    (dict(uncertainty_mode=-1), ("uncertainty_mode",)),
    (dict(resume=2), ("resume 2",)),
    (dict(resume=-1), ("resume",)),
    (dict(discount=float("nan")), ("discount",)),
    (dict(discount=0.0), ("discount",)),
    (dict(discount=-0.5), ("discount",)),
    (dict(discount=1.0000001), ("discount",)),
    (dict(precision=5), ("precision 5",)),
    (dict(precision=-1), ("precision",)),
    (dict(precision=4), ("planes",)),                                        # split precision without the ensemble's planes
    (dict(precision=4, dyn_planes=PTR), ("actor_blob_T",)),                  # ... without the actor's T blob
    (dict(precision=4, dyn_planes=PTR, actor_blob_T=PTR, mopo_blob=PTR), ("mopo_blob_T",)),
])
def test_refusals_name_the_field(lib, over, words):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **over), *words)


@pytest.mark.parametrize("field", POINTERS)
def test_every_null_pointer_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **{field: None}), "null pointer", field)


def test_refusal_edges_that_are_not_errors(lib):
    from mobody_amd import _lib
    # B == 0 returns 0 whatever the pointers are; init_obs is read only when resume == 0, so with resume == 1 a null one
    # gets past the pointer checks (and is refused further on, by a field that has nothing to do with it)
    none = {k: None for k in POINTERS}
    assert lib.mobody_ens_evaluate(C.byref(_good(_lib, B=0, **none)), None) == 0
    assert "init_obs" not in _refused(lib, _good(_lib, resume=1, init_obs=None, n_elites=0), "n_elites")
    assert lib.mobody_ens_evaluate(None, None) == -1 and lib.mobody_last_error().decode().startswith(ENTRY + ":")
    assert lib.mobody_ens_evaluate_workspace(C.byref(_good(_lib, struct_bytes=8))) == -1
    assert lib.mobody_last_error().decode().startswith("mobody_ens_evaluate_workspace:")
    # the workspace holds at least the action, the next observation, the penalty and the step's own workspace
    need = lib.mobody_ens_evaluate_workspace(C.byref(_good(_lib, B=33)))
    assert need >= 33 * (6 + 17 + 1) + lib.mobody_dyn_step_workspace(17, 6, 33)


# ---- accounting (the restatement the GPU tests compare against) -----------------------------------------------------
def test_accounting_on_hand_made_tables():
    f = np.float32
    nan = f("nan")
    #            row 0: terminal at step 0   row 1: never terminal   row 2: terminal at step 2, NaN afterwards
    raw = np.array([[1.5, 0.25, 2.0],
                    [9.0, 0.5, -1.0],
                    [9.0, 1.0, 0.125],
                    [9.0, 2.0, nan],
                    [9.0, 4.0, nan]], f)
    pen = np.array([[0.5, 1.0, 1.0], [7.0, 1.0, 2.0], [7.0, 1.0, 4.0], [7.0, 1.0, nan], [7.0, 1.0, nan]], f)
    term = np.array([[1, 0, 0], [0, 0, 0], [1, 0, 1], [0, 0, 1], [0, 0, 0]], bool)
    st = ref.evaluate_tables(raw, pen, term)
    assert st["length"].tolist() == [1, 5, 3] and st["alive"].tolist() == [False, True, False]
    assert st["ret"].tolist() == [1.5, 7.75, 1.125] and np.isfinite(st["ret"]).all()       # the terminating step counts
    assert st["pen_sum"].tolist() == [0.5, 5.0, 7.0] and st["disc"].tolist() == [1.0, 1.0, 1.0]
    # a terminal flag that already has `!alive` folded in (as the fused step reports it) gives the same state
    folded = term.copy()
    folded[1:, 0] = True; folded[3:, 2] = True
    st2 = ref.evaluate_tables(raw, pen, folded)
    assert all(np.array_equal(st[k], st2[k]) for k in st)
    # discount: ret = fma(disc, raw, ret) with disc *= discount after each live step, all in fp32
    d = f(0.5)
    st = ref.evaluate_tables(raw, pen, term, discount=0.5)
    assert st["ret"].tolist() == [1.5, 0.25 + 0.25 + 0.25 + 0.25 + 0.25, 2.0 - 0.5 + 0.125 * 0.25]
    assert st["disc"].tolist() == [0.5, float(d ** 5), 0.125]
    r64, mag = ref.returns_f64(raw, term, 0.5)
    assert np.allclose(r64, st["ret"]) and mag[2] == 2.0 + 0.5 + 0.125 * 0.25


def test_accounting_is_sequential_fp32_and_fma_rounds_once():
    f = np.float32
    # discount 1: the plain left-to-right fp32 sum (1 + 2^-24 twice stays 1 in fp32, a pairwise sum would not)
    raw = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], f)
    st = ref.evaluate_tables(raw, np.zeros_like(raw), np.zeros((3, 1), bool))
    assert st["ret"][0] == f(1.0) and st["length"][0] == 3
    # one rounding: (1 + 2^-12)^2 - 1 = 2^-11 + 2^-24; the separately rounded product would lose the 2^-24
    a = f(1.0 + 2.0 ** -12)
    assert ref.fma32(a, a, f(-1.0)) == f(2.0 ** -11 + 2.0 ** -24) and f(a * a) - f(1.0) == f(2.0 ** -11)
    # resuming a state equals one pass
    rng = np.random.default_rng(0)
    raw, pen = rng.standard_normal((5, 9)).astype(f), rng.random((5, 9)).astype(f)
    term = rng.random((5, 9)) < 0.2
    one = ref.evaluate_tables(raw, pen, term, 0.99)
    two = ref.new_state(9)
    for t in range(5):
        ref.account(two, raw[t], pen[t], term[t], 0.99)
    assert all(np.array_equal(one[k], two[k]) for k in one)


# ---- CLI pieces ----------------------------------------------------------------------------------------------------
def test_episode_starts_on_a_hand_made_dataset():
    from mobody_amd import train_mobody as tm
    obs = np.arange(10, dtype=np.float32).reshape(10, 1) * np.ones((1, 3), np.float32)
    nxt = obs + 1.0                                        # one continuous trajectory ...
    term = np.zeros(10, bool)
    term[2] = term[6] = True                               # ... with two terminals (rows 3 and 7 start episodes)
    obs[5:] += 100.0; nxt[5:] += 100.0                     # ... and one discontinuity (row 5 starts one, no terminal before it)
    assert tm.episode_starts(obs, nxt, term).tolist() == [0, 3, 5, 7]
    assert tm.episode_starts(obs, nxt, term.astype(np.float32).reshape(-1, 1)).tolist() == [0, 3, 5, 7]
    assert tm.episode_starts(obs[:1], nxt[:1], term[:1]).tolist() == [0] and tm.episode_starts(obs[:0], nxt[:0], term[:0]).size == 0
    # a discontinuity in a single coordinate counts
    nxt2 = nxt.copy(); nxt2[8, 2] += 1e-3
    assert tm.episode_starts(obs, nxt2, term).tolist() == [0, 3, 5, 7, 9]
    starts = np.array([0, 3, 5, 7])
    state = np.random.get_state()[1].copy()
    few = tm.model_eval_rows(starts, 3, seed=1)
    assert len(set(few.tolist())) == 3 and set(few.tolist()) <= set(starts.tolist())        # enough starts: distinct ones
    many = tm.model_eval_rows(starts, 64, seed=1)
    assert many.shape == (64,) and set(many.tolist()) == set(starts.tolist())               # fewer starts: with replacement
    assert np.array_equal(many, tm.model_eval_rows(starts, 64, seed=1)) and not np.array_equal(many, tm.model_eval_rows(starts, 64, seed=2))
    assert np.array_equal(state, np.random.get_state()[1])                                  # the global stream is not consumed
    with pytest.raises(ValueError):
        tm.model_eval_rows(np.zeros(0, np.int64), 4, seed=0)


def test_model_evaluation_is_off_by_default_in_the_merged_config():
    from mobody_amd import train_mobody as tm
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "g10b_config_merge.json")))
    argv = ["--policy", "MOBODY", "--env", "walker2d-friction", "--shift_level", "2.0"]
    cfg = tm.build_config(tm.build_parser().parse_args(argv), 17, 6, 1.0)
    today = {k for k, _ in g["update"]} | set(g["yaml"]["mujoco/mobody/walker2d.yaml"]) | {"rng", "seed"}
    assert set(cfg) == today and not {"model_eval_episodes", "model_eval_horizon"} & set(cfg)
    on = tm.build_config(tm.build_parser().parse_args(argv + ["--params", '{"model_eval_episodes": 64, "model_eval_horizon": 5}']), 17, 6, 1.0)
    assert set(on) == today | {"model_eval_episodes", "model_eval_horizon"} and on["model_eval_episodes"] == 64
    assert not [a for a in tm.build_parser()._actions if "model_eval" in "".join(a.option_strings)]      # no new flag
