"""The ensemble step and the rollout, the parts that need no GPU: `mobody_ens_step` and `mobody_ens_rollout` draw their
refusals from the checker the evaluation and the replay use (every required pointer by name, every range rule naming its
field, before any runtime call), empty calls return 0 whatever the pointers are, the positional forms refuse under their
own names, and the four workspace queries keep their closed forms."""
import ctypes as C
import os

import pytest

PTR = 0x1000          # a non-NULL pointer value: only compared with NULL before the refusal under test
STEP_POINTERS = ("dyn_blob", "elites", "obs", "act", "next_obs", "reward", "terminal", "penalty", "workspace")
ROLLOUT_POINTERS = ("dyn_blob", "elites", "actor_blob", "init_obs", "ring", "ptr_size", "workspace")
RING_POINTERS = ("state", "action", "next_state", "reward", "not_done")
SHAPES = [(17, 6, 1), (17, 6, 33), (111, 8, 65)]      # walker: one row, a ragged tile; ant: one row past a 64-row tile


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _step(_lib, **over):
    """A MobodyEnsStep that passes every check (nothing may be launched with it: its device pointers are fake)."""
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    f = dict(struct_bytes=C.sizeof(_lib.MobodyEnsStep), uncertainty_mode=0, precision=0, S=17, A=6, task=4, B=4, n_elites=5, elites=el,
             seed=1, call=1, use_trg=1)
    f.update({k: PTR for k in STEP_POINTERS if k != "elites"})
    f.update(over)
    blk = _lib.MobodyEnsStep(**f)
    blk._keep = el
    return blk


def _rollout(_lib, view=None, **over):
    """A MobodyEnsRollout that passes every check.  `ring` is a real host struct, as the ABI asks; the block keeps it alive."""
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    v = dict(state=PTR, action=PTR, next_state=PTR, reward=PTR, not_done=PTR, pitch=48)
    v.update(view or {})
    view = _lib.MobodyBufferView(**v)
    f = dict(struct_bytes=C.sizeof(_lib.MobodyEnsRollout), uncertainty_mode=0, precision=0, S=17, A=6, task=4, B=4, H=2, n_elites=5,
             elites=el, seed=1, call0=1, max_action=1.0, use_trg=1, ring=C.pointer(view), cap=100)
    f.update({k: PTR for k in ROLLOUT_POINTERS if k not in ("elites", "ring")})
    f.update(over)
    blk = _lib.MobodyEnsRollout(**f)
    blk._keep = (view, el)
    return blk


GOOD = {"mobody_ens_step": _step, "mobody_ens_rollout": _rollout}


def _refused(lib, entry, blk, *words):
    assert getattr(lib, entry)(C.byref(blk), None) == -1
    msg = lib.mobody_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


# ---- the model's range rules: one checker, so both entry points name the same fields ---------------------------------
@pytest.mark.parametrize("entry", sorted(GOOD))
@pytest.mark.parametrize("over,words", [
    (dict(struct_bytes=8), ("struct_bytes", "sizeof(MobodyEns")),
    (dict(B=-1), ("B < 0",)),
    (dict(uncertainty_mode=3), ("uncertainty_mode 3",)),
    (dict(uncertainty_mode=-1), ("uncertainty_mode",)),
    (dict(precision=5), ("precision 5",)),
    (dict(precision=-1), ("precision",)),
    (dict(precision=4), ("planes",)),                                        # split precision without the ensemble's planes
    (dict(precision=4, dyn_planes=PTR, actor_blob_T=PTR, mopo_blob=PTR), ("mopo_blob_T",)),
    (dict(task=7), ("task",)),
    (dict(task=-1), ("task",)),
    (dict(task=6), ("task", "S > 26")),                                     # the pen predicate reads coordinate 26
    (dict(n_elites=0), ("n_elites",)),
    (dict(n_elites=8), ("n_elites",)),
])
def test_range_refusals_name_the_field(lib, entry, over, words):
    from mobody_amd import _lib
    if entry == "mobody_ens_step":
        over = {k: v for k, v in over.items() if k != "actor_blob_T"}
    _refused(lib, entry, GOOD[entry](_lib, **over), *words)


@pytest.mark.parametrize("over,words", [
    (dict(H=-1), ("H < 0",)),
    (dict(B=5, cap=4), ("B > cap", "5", "4")),                              # a step's rows have to fit the ring
    (dict(precision=4, dyn_planes=PTR), ("actor_blob_T",)),                  # split precision without the actor's T blob
])
def test_range_refusals_of_the_rollout_alone(lib, over, words):
    from mobody_amd import _lib
    _refused(lib, "mobody_ens_rollout", _rollout(_lib, **over), *words)


# ---- pointers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", STEP_POINTERS)
def test_every_null_pointer_of_the_step_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, "mobody_ens_step", _step(_lib, **{field: None}), "null pointer", field)


@pytest.mark.parametrize("field", ROLLOUT_POINTERS)
def test_every_null_pointer_of_the_rollout_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, "mobody_ens_rollout", _rollout(_lib, **{field: None}), "null pointer", field)


@pytest.mark.parametrize("field", RING_POINTERS)
def test_every_null_field_of_the_ring_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, "mobody_ens_rollout", _rollout(_lib, view={field: None}), "null pointer", "ring", field)


def test_refusal_edges_that_are_not_errors(lib):
    from mobody_amd import _lib
    # an empty call returns 0 whatever the pointers are: B == 0, and for the rollout H == 0
    assert lib.mobody_ens_step(C.byref(_step(_lib, B=0, **{k: None for k in STEP_POINTERS})), None) == 0
    none = {k: None for k in ROLLOUT_POINTERS}
    assert lib.mobody_ens_rollout(C.byref(_rollout(_lib, B=0, **none)), None) == 0
    assert lib.mobody_ens_rollout(C.byref(_rollout(_lib, H=0, **none)), None) == 0
    assert lib.mobody_ens_rollout(C.byref(_rollout(_lib, B=0, cap=0)), None) == 0          # B <= cap is a rule for rows
    # ... but not whatever the mode is
    _refused(lib, "mobody_ens_step", _step(_lib, B=0, uncertainty_mode=3), "uncertainty_mode 3")
    _refused(lib, "mobody_ens_rollout", _rollout(_lib, H=0, uncertainty_mode=3), "uncertainty_mode 3")
    # per-row picks (elite_idx) stand in for the elites: neither the array nor its length is looked at
    msg = _refused(lib, "mobody_ens_step", _step(_lib, elite_idx=PTR, elites=None, n_elites=0, workspace=None), "workspace")
    assert "elites" not in msg
    # optional fields: noise, elite_idx, alive, raw_reward, mean_out, call_dev, the planes in fp32 -- the good blocks leave
    # them null and are refused only by the field under test
    assert "null pointer" not in _refused(lib, "mobody_ens_step", _step(_lib, task=7), "task")
    assert lib.mobody_ens_step(None, None) == -1 and lib.mobody_last_error().decode().startswith("mobody_ens_step:")
    assert lib.mobody_ens_rollout(None, None) == -1 and lib.mobody_last_error().decode().startswith("mobody_ens_rollout:")


def test_positional_forms_refuse_under_their_own_names(lib):
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    P = PTR

    def dyn_step(task=4, B=4, workspace=P):
        return lib.mobody_dyn_step(P, None, 0, 17, 6, task, P, P, B, None, None, None, el, 5, 1, 1, None, 0.0, 0, 1, P, P, P, P, None,
                                   None, workspace, None)

    def mopo_step(task=4, B=4, mopo=P, workspace=P):
        return lib.mobody_mopo_step(P, None, mopo, None, 0, 17, 6, task, P, P, B, None, None, None, el, 5, 1, 1, 0.0, 0, P, P, P, P,
                                    None, None, workspace, None)

    def rollout(task=4, B=4, H=2, workspace=P):
        from mobody_amd import _lib
        view = _lib.MobodyBufferView(state=P, action=P, next_state=P, reward=P, not_done=P, pitch=48)
        return lib.mobody_rollout(P, None, P, None, 0, 17, 6, task, 1.0, P, B, H, el, 5, 1, 1, 0.0, 0, 1, 0.0, 0, C.byref(view), 100, P,
                                  workspace, None)

    for name, call in (("mobody_dyn_step", dyn_step), ("mobody_mopo_step", mopo_step), ("mobody_rollout", rollout)):
        assert call(B=0, workspace=None) == 0
        for kw, word in ((dict(task=7), "task"), (dict(workspace=None), "null pointer workspace"), (dict(B=-1), "B < 0")):
            assert call(**kw) == -1
            msg = lib.mobody_last_error().decode()
            assert msg.startswith(name + ":") and word in msg, msg
    assert rollout(H=0, workspace=None) == 0
    assert mopo_step(mopo=None) == -1 and lib.mobody_last_error().decode().startswith("mobody_mopo_step:")


# ---- workspaces: the closed forms, written out --------------------------------------------------------------------
def _r4(n):
    return (n + 3) // 4 * 4          # every piece of a workspace is rounded up to 4 floats


@pytest.mark.parametrize("S,A,B", SHAPES)
def test_workspace_sizes_are_the_closed_forms(lib, S, A, B):
    from mobody_amd import _lib
    step = 7 * B * S + 7 * B                                   # ensemble means + per-member reward means
    flags = _r4((B + 3) // 4)                                  # B bytes
    assert lib.mobody_dyn_step_workspace(S, A, B) == step
    # two observation buffers, action, reward, penalty | step | terminal, keep, alive | scan
    want = 2 * _r4(B * S) + _r4(B * A) + 2 * _r4(B) + _r4(step) + 3 * flags + _r4(B + 1040)
    assert lib.mobody_ens_rollout_workspace(C.byref(_rollout(_lib, S=S, A=A, B=B))) == want
    assert lib.mobody_rollout_workspace(S, A, B) == want
    # action, next observation, penalty | step | terminal, alive_next
    blk = _lib.MobodyEnsEval(struct_bytes=C.sizeof(_lib.MobodyEnsEval), S=S, A=A, B=B)
    assert lib.mobody_ens_evaluate_workspace(C.byref(blk)) == _r4(B * A) + _r4(B * S) + _r4(B) + _r4(step) + 2 * flags
    # next observation, penalty | step | terminal
    blk = _lib.MobodyEnsReplay(struct_bytes=C.sizeof(_lib.MobodyEnsReplay), S=S, A=A, B=B)
    assert lib.mobody_ens_replay_workspace(C.byref(blk)) == _r4(B * S) + _r4(B) + _r4(step) + flags
