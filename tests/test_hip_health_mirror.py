"""config['f16_guard'] of the host mirror: a critic weight trained past the f16x2 planes' range is reported at the next check
point ('raise') or the run moves to bf16x3 ('fallback'); either way from the last state computed from healthy planes.

The planted case: W2[k][n] of critic member 0 at 255.8749, the first Adam step has magnitude lr = 3e-4 exactly (zero moments,
|g| >> 1e-8), so a negative gradient lands the weight at 255.8752 >= 255.875.  The gradient's sign is arranged, not hoped for:
with every reward at 1e4 the TD target exceeds Q on every row, so dL/dz2[.][n] has the sign of -W3[n]; n is a hidden unit with
W3[n] > 0 and k the layer-1 unit with the largest bias (active on most rows)."""
import warnings

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

S, A, BS = 17, 6, 64
PLANT = 255.8749


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_words():
    """Faults planted here must not reach later tests through the device's shared block."""
    yield
    from mobody_amd import ops
    torch.cuda.synchronize()
    ops.health_bind(None)


class Writer:
    def add_scalar(self, *a, **k):
        pass


def rows(seed, dev):
    from test_hip_mirror import FixedRows
    r = list(gu.gi.batch(seed, 64, S, A))
    r[3] = np.full_like(r[3], 1e4)
    return FixedRows(tuple(r), S, A, dev).rb


def make(dev, guard, mfma, plant=True):
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    cfg = gu.policy_cfg(S, A, mfma=mfma, f16_guard=guard)
    pol = MOBODY(cfg, dev)
    pa, pq, _ = gu.policy_params(31, S, A)
    where = None
    if plant:
        n = int(np.argmax(pq["network1.network.4.weight"][0]))
        k = int(np.argmax(pq["network1.network.0.bias"]))
        assert pq["network1.network.4.weight"][0, n] > 0
        pq = {kk: v.copy() for kk, v in pq.items()}
        pq["network1.network.2.weight"][n, k] = PLANT          # nn.Linear layout [out][in]
        where = (n, k)
    pol.policy.load_state_dict({k_: torch.from_numpy(v) for k_, v in pa.items()})
    pol.q_funcs.load_state_dict({k_: torch.from_numpy(v) for k_, v in pq.items()})
    pol.target_q_funcs.load_state_dict({k_: torch.from_numpy(v) for k_, v in pq.items()})
    pol.fake_replay_buffer = rows(503, dev)
    return pol, rows(501, dev), rows(502, dev), where


def w_planted(pol, where):
    return float(pol.q_funcs.state_dict()["network1.network.2.weight"][where[0], where[1]])


def test_guard_raise_reports_at_the_next_check_point_and_leaves_a_saveable_state(dev, tmp_path, monkeypatch):
    import mobody_amd.algo.offline_offline.mobody as mob
    monkeypatch.setattr(mob, "REFRESH_EVERY", 4)                  # check points at total_it = 5, 9, ...
    pol, src, tar, where = make(dev, "raise", "f16x2")
    pol.total_it = 1
    calls = 0
    with pytest.raises(FloatingPointError, match="q_funcs") as ei:
        for _ in range(4):                                       # total_it 2 (the fault), 3, 4 (frozen), 5: checked before its refresh
            pol.train(src, tar, BS, None, None)
            calls += 1
    print(ei.value, "| planted weight now", repr(w_planted(pol, where)))
    assert calls == 3 and "F16_RANGE" in str(ei.value) and "bf16x3" in str(ei.value) and "step 1" in str(ei.value)
    assert w_planted(pol, where) >= 255.875                      # the faulting update itself was applied (fp32 exact)
    assert pol.q_optimizer.t == 1 and pol.policy_optimizer.t == 0            # what was applied: one critic step, no actor step
    prefix = str(tmp_path / "model")
    pol.save(prefix)
    for suf in ("_critic", "_critic_optimizer", "_actor", "_actor_optimizer"):
        sd = torch.load(prefix + suf, weights_only=True)
        leaves = sd.values() if suf in ("_critic", "_actor") else [x for st in sd["state"].values() for x in st.values()]
        assert all(bool(torch.isfinite(torch.as_tensor(x)).all()) for x in leaves), suf
    fb = pol.fake_replay_buffer
    assert bool(torch.isfinite(fb.state[:fb.size]).all()) and bool(torch.isfinite(fb.reward[:fb.size]).all())
    assert float(torch.load(prefix + "_critic_optimizer", weights_only=True)["state"][0]["step"]) == 1.0


def test_guard_fallback_continues_in_bf16x3_from_the_frozen_state(dev, tmp_path, monkeypatch):
    import mobody_amd.algo.offline_offline.mobody as mob
    monkeypatch.setattr(mob, "REFRESH_EVERY", 10 ** 9)            # no refresh in this test: the check point is the logging step
    # the frozen state, from a 'raise' twin
    a, src, tar, where = make(dev, "raise", "f16x2")
    a.total_it = 4996
    with pytest.raises(FloatingPointError):
        for _ in range(4):                                       # 4997 (the fault) .. 5000 (logging step: checked)
            a.train(src, tar, BS, Writer(), None)
    prefix = str(tmp_path / "frozen")
    a.save(prefix)
    target = a.target_q_funcs.state_dict()
    from mobody_amd import ops
    ops.health_clear()
    # the run under test
    f, src, tar, _ = make(dev, "fallback", "f16x2")
    f.total_it = 4996
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        losses = []
        for _ in range(4 + 20):
            f.train(src, tar, BS, Writer(), None)
            losses.append(f.losses())
    assert any("bf16x3" in str(w.message) for w in rec)
    assert f.config["mfma"] == "bf16x3" and f.mfma == "bf16x3" and f.q_funcs.precision == 3
    assert np.isfinite(np.asarray(losses[3:])).all()             # the step that fell back and the 20 after it
    assert f.q_optimizer.t == 1 + 21 and f.policy_optimizer.t == 21
    # a fresh bf16x3 object that loads the frozen state and takes the same 21 steps on the same rows
    b, src, tar, _ = make(dev, "raise", "bf16x3", plant=False)
    b.load(prefix)
    b.target_q_funcs.load_state_dict(target)
    b.total_it = 4999
    for _ in range(21):
        b.train(src, tar, BS, Writer(), None)
    torch.cuda.synchronize()
    for name in ("q_funcs", "target_q_funcs", "policy"):
        assert torch.equal(getattr(f, name).blob, getattr(b, name).blob), name
        assert torch.equal(getattr(f, name).blob_T.view(torch.int32), getattr(b, name).blob_T.view(torch.int32)), name
    for name in ("q_optimizer", "policy_optimizer"):
        assert torch.equal(getattr(f, name).m, getattr(b, name).m) and torch.equal(getattr(f, name).v, getattr(b, name).v), name


def test_guard_off_binds_nothing_and_bad_values_are_refused(dev):
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    pol = MOBODY(gu.policy_cfg(S, A, f16_guard="off"), dev)
    assert pol._health is None
    with pytest.raises(ValueError, match="f16_guard"):
        MOBODY(gu.policy_cfg(S, A, f16_guard="warn"), dev)


def test_pretraining_raise_names_the_encoder(dev):
    """learn() batches with a planted encoder W2 (zs2) under f16x2 pre-training: the Adam step of size lr = 1e-3 moves every
    weight by lr in its first step, so a weight planted within lr of the bound on the side its gradient pushes to crosses it.
    Eight elements are planted at +-(255.875 - 5e-4), alternating in sign; each crosses when its gradient points outwards, and
    the test first asserts that at least one did (a stated precondition of the planted case, not a property under test)."""
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    from mobody_amd import ops
    cfg = gu.policy_cfg(S, A, mfma="f16x2", f16_guard="raise")
    p = gu.gi.dyn_params(31, S, A)
    k = int(np.argmax(p["zs1.bias"][0, 0]))
    for j, sign in ((3, 1.0), (40, -1.0), (77, 1.0), (110, -1.0), (150, 1.0), (190, -1.0), (222, 1.0), (250, -1.0)):
        p["zs2.weight"][0, k, j] = sign * (255.875 - 5e-4)       # EnsembleLinear layout [member][in][out]
    m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg)
    m.load_state_dict({kk: torch.from_numpy(v) for kk, v in p.items()}, strict=False)
    dyn = MOBODYEnsembleDynamics(cfg, m, None, None, get_termination_fn("walker2d-medium-v2"), rng="device", seed=5)
    with torch.cuda.device(dev):
        ops.health_clear()
    s, a, s2, r, _ = gu.gi.batch(77, 256, S, A)
    rep = lambda x: np.repeat(x[None], 7, 0)
    dyn.learn(False, rep(s), rep(a), rep(s2), rep(r), 64, 0.0)    # four batches: one of them faults, the later ones are frozen
    st = m.train_state()
    torch.cuda.synchronize()
    from mobody_amd import _lib
    L = _lib.pretrain_layout(S, A)
    assert float(ops._mlp_w2(st["blob"][L.off_enc:], L.enc, 7).abs().max()) >= ops.F16_W_LIMIT, "precondition: no planted weight crossed"
    frozen = [st["blob"].clone(), st["m"].clone(), st["v"].clone()]
    dyn.learn(False, rep(s), rep(a), rep(s2), rep(r), 64, 0.0)
    torch.cuda.synchronize()
    for x, y in zip(frozen, (st["blob"], st["m"], st["v"])):
        assert torch.equal(x, y)                                 # nothing applies any more
    assert bool(torch.isfinite(st["blob"]).all())
    with pytest.raises(FloatingPointError, match="state encoder") as ei:
        dyn.validate(False, s, a, s2, r[:, 0])
    print(ei.value)
    assert "F16_RANGE" in str(ei.value) and "bf16x3" in str(ei.value)


def test_shared_block_is_kept_by_new_objects_and_read_by_guard_off(dev, tmp_path):
    """One block per device: constructing another object does not erase a fault that is not reported yet, and an object
    with f16_guard='off' (which binds nothing itself) still reports a fault in a block somebody else bound -- its optimizer
    launches are frozen by it like everybody's."""
    from mobody_amd import ops, _lib
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    MOBODY(gu.policy_cfg(S, A, f16_guard="raise"), dev)          # binds the device's block
    w = ops.health_bound(dev)
    assert w is not None and int(w[0]) == 0
    w[0] = _lib.HEALTH_NONFINITE
    off = MOBODY(gu.policy_cfg(S, A, f16_guard="off"), dev)
    again = MOBODY(gu.policy_cfg(S, A, f16_guard="raise"), dev)
    torch.cuda.synchronize()
    assert int(w[0]) == _lib.HEALTH_NONFINITE and ops.health_bound(dev) is w
    for pol in (off, again):
        with pytest.raises(FloatingPointError, match="NONFINITE"):
            pol.save(str(tmp_path / "m"))
