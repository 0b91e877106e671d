"""CPU checks of the IQL references (tests/iql_ref.py) and of the parts of the feature that need no GPU:
  * the fp32 restatement reproduces every g24 fixture (the real reference's train() steps) at the tolerances
    tests/test_oracle_golden.py uses for G7 (worst policy-gradient entry: 0.85 of the tolerance, the same on every machine -- the
    restatement's layers are correctly rounded, tests/iql_ref.py mlp3); `short` pins the six learning rates and policy states of a
    T_max = 8 schedule
  * two mutants miss the fixture's policy gradients: max_action inside the policy loss (at max_action = 0.4; the reference's loss
    has no such factor, so the fixture holds at any max_action) and the advantage of AFTER V's update
  * the fp64 closed forms of both seeds (BwdSeed modes 5 and 6) equal fp64 autograd of the losses written out here
  * the learning-rate closed form equals torch's CosineAnnealingLR over a whole T_max = 8 cycle
  * the built-in iql config defaults equal the reference's yaml files (g24_iql_configs.json)
  * call_algo, the header / binding contract of the new entry points and their argument refusals

Without the feature the registry, config, binding and refusal tests fail (call_algo('iql') raises NotImplementedError, the symbols
do not exist); the restatement, autograd and scheduler tests exercise tests/iql_ref.py alone and pass either way.
"""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
import iql_ref as IR
from oracle import mobody_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT, AT = 2e-5, 2e-6


def close(a, b, rtol=RT, atol=AT):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


def run_fixture(tag, mutant=None, check=True, **over):
    """The restatement over the fixture's steps; returns the worst policy-gradient error in units of its tolerance.  over: config
    keys the reference's step does not read (max_action: its loss has no such factor, so the fixture holds at any value)."""
    g = gu.load(f"g24_iql_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = IR.iql_cfg(S, A, **dict(IR.VARIANTS[tag], **over))
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    for p, k in ((pa, "wsum_actor"), (pq, "wsum_q"), (pv, "wsum_v")):
        assert abs(gu.gi.checksum(p) - float(g[k])) <= 1e-9 * abs(float(g[k])), k
    st = O.TrainState(pa, pq, pv)
    batch = IR.g24_batch(bs, S, A)
    worst = 0.0
    short = tag == "short"
    for step in range(1, IR.STEPS[tag] + 1):
        out = IR.train_step(st, batch, cfg, mutant)
        if not short:
            for k, v in out["grads"]["actor"].items():
                want = g[f"s{step}_actor_g::{k}"]
                err = np.abs(gu.sub(v.numpy()).astype(np.float64) - want)
                worst = max(worst, float(np.max(err / (2e-7 + 2e-4 * np.abs(want)))))
        if not check:
            continue
        close(out["lr"], g["lr"][step - 1], rtol=1e-12, atol=0)
        close(out["v_loss"], g["v_loss"][step - 1], rtol=1e-5)
        close(out["q_loss"], g["q_loss"][step - 1], rtol=1e-5)
        close(out["pi_loss"], g["pi_loss"][step - 1], rtol=1e-5)
        close(out["adv"], g[f"s{step}_adv"], rtol=1e-5, atol=1e-5)
        for k, v in st.actor.items():
            close(gu.sub(v.numpy()), g[f"s{step}_actor_p::{k}"], rtol=1e-5, atol=1e-6)
        if short:
            continue
        for nm in ("v", "q", "actor"):
            for k, v in out["grads"][nm].items():
                close(gu.sub(v.numpy()), g[f"s{step}_{nm}_g::{k}"], rtol=2e-4, atol=2e-7)
                v64 = v.numpy().astype(np.float64)
                close([v64.sum(), (v64 ** 2).sum()], g[f"s{step}_{nm}_gsum::{k}"], rtol=2e-4, atol=2e-6)
        for nm, params in (("v", st.v), ("q", st.q), ("qt", st.q_targ)):
            for k, v in params.items():
                close(gu.sub(v.numpy()), g[f"s{step}_{nm}_p::{k}"], rtol=1e-5, atol=1e-6)
    n = IR.STEPS[tag]
    assert list(g["calls_src"]) == [bs] * n and list(g["calls_tar"]) == [bs] * n
    assert [int(x) for x in g["opt_steps"]] == [n, n, n] and int(g["last_epoch"]) == n and int(g["total_it"]) == n
    return worst


@pytest.mark.parametrize("tag", list(IR.VARIANTS))
def test_restatement_reproduces_reference_fixture(tag):
    assert run_fixture(tag) <= 1.0


def test_fixtures_exercise_the_clamp_and_the_schedule():
    for tag in ("default", "lam09_temp10"):
        g = gu.load(f"g24_iql_{tag}")
        x = IR.iql_cfg(17, 6, **IR.VARIANTS[tag])["temp"] * g["s1_adv"]
        assert (x > IR.LN100).any() and (x < IR.LN100).any() and (g["s1_adv"] < 0).any() and (g["s1_adv"] > 0).any()
    lr = gu.load("g24_iql_short")["lr"]
    assert lr[0] == 3e-4 and np.all(np.diff(lr) < -1e-5)                      # the rate moves visibly at T_max = 8
    # the logstd half never moves (zero gradient, zero Adam moments): the reference's own numbers
    g = gu.load("g24_iql_default")
    pa = IR.iql_params(17, 6, int(g["seed"]))[0]
    for k in ("network.network.4.weight", "network.network.4.bias"):
        assert np.array_equal(gu.sub(g[f"s2_actor_g::{k}"].reshape(12, -1)[6:]), np.zeros_like(gu.sub(g[f"s2_actor_g::{k}"].reshape(12, -1)[6:])))
        assert np.array_equal(g[f"s2_actor_p::{k}"].reshape(12, -1)[6:], pa[k].reshape(12, -1)[6:])


def test_post_update_advantage_mutant_misses_the_fixture():
    worst = run_fixture("default", mutant="post_adv", check=False)
    print(f"post-update-adv mutant: worst policy-gradient error = {worst:.3g} x tolerance")
    assert worst > 1.0


# ---- the seeds' closed forms against fp64 autograd ---------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.5, 0.7, 0.9])
@pytest.mark.parametrize("gmul", [1, 2])
def test_expectile_closed_form_equals_fp64_autograd(lam, gmul):
    N = 37
    rng = np.random.default_rng(int(lam * 10) + gmul)
    qt = rng.standard_normal((2, N))
    v = rng.standard_normal(N)
    v[:3] = np.minimum(qt[0, :3], qt[1, :3])                                   # adv exactly 0
    Ng = gmul * N
    cf = IR.expectile_seed(qt, v, lam, Ng)
    assert (cf["adv"] == 0).sum() == 3 and (cf["adv"] < 0).sum() >= 3 and (cf["adv"] > 0).sum() >= 3
    vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    u = torch.min(torch.tensor(qt[0]), torch.tensor(qt[1])) - vt
    loss = (torch.abs(lam - (u < 0).double()) * u ** 2).sum() / Ng              # asymmetric_l2_loss (iql.py:117-118), global mean
    (gz,) = torch.autograd.grad(loss, vt)
    err = np.abs(cf["dz3"] - gz.numpy()).max()
    print(f"lam={lam} gmul={gmul}: max |closed form - autograd| = {err:.3g}")
    assert err <= 1e-15 and abs(cf["L_V"] - float(loss.detach())) <= 1e-15 * max(1.0, abs(float(loss.detach())))
    assert (cf["dz3"][:3] == 0).all()


def awr_case(temp, gmul, mutant=None, ma=1.0):
    N, A = 37, 6
    rng = np.random.default_rng(int(temp) + gmul)
    z = rng.standard_normal((N, 2 * A)) * 1.5
    act = rng.uniform(-1, 1, (N, A)) * ma
    adv = rng.standard_normal(N)
    adv[:6] = np.array([IR.LN100 + 1e-3, IR.LN100 - 1e-3, IR.LN100 + 1, IR.LN100 - 1, 90.0, -90.0]) / temp
    adv[6] = 0.0
    Ng = gmul * N
    cf = IR.awr_seed(z, act, adv, temp, Ng)
    assert (cf["e"] > 100).sum() >= 3 and (cf["e"] < 100).sum() >= 3 and cf["w"][4] == 100.0 and cf["w"][6] == 1.0
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    mu, _ = zt.chunk(2, dim=1)                                                 # bc_loss, iql.py:91-95
    pred = torch.tanh(mu) * (ma if mutant == "max_action" else 1.0)
    w = torch.exp(temp * torch.tensor(adv)).clamp(max=100.0)                   # update_policy :199
    loss = (w[:, None] * (pred - torch.tensor(act)) ** 2).sum() / (Ng * A)
    (gz,) = torch.autograd.grad(loss, zt)
    ref = gz.numpy()
    err = np.abs(cf["dz3"] - ref).max()
    if mutant is None:
        print(f"temp={temp} gmul={gmul}: max |closed form - autograd| = {err:.3g}, max |dz3| = {np.abs(ref).max():.3g}")
        assert err <= 1e-15 * max(1.0, np.abs(ref).max()) and abs(cf["L_pi"] - float(loss.detach())) <= 1e-14 * abs(float(loss.detach()))
        assert np.isfinite(cf["dz3"]).all() and (cf["dz3"][:, A:] == 0).all() and (ref[:, A:] == 0).all()
    return err, np.abs(ref).max()


@pytest.mark.parametrize("temp", [3.0, 10.0])
@pytest.mark.parametrize("gmul", [1, 2])
def test_awr_closed_form_equals_fp64_autograd(temp, gmul):
    awr_case(temp, gmul)


def test_max_action_mutant_misses_the_fixture_at_max_action_04():
    """max_action scales the action in select_action only (iql.py:89): the restatement reproduces the fixture at max_action = 0.4
    too, and with the factor multiplied into tanh(mu) of the loss it does not."""
    assert run_fixture("default", max_action=0.4) <= 1.0
    worst = run_fixture("default", mutant="max_action", check=False, max_action=0.4)
    print(f"max_action mutant: worst policy-gradient error = {worst:.3g} x tolerance")
    assert worst > 1.0
    err, scale = awr_case(3.0, 1, mutant="max_action", ma=0.4)
    assert err > 1e-3 * scale


def test_cosine_closed_form_equals_torch_scheduler():
    T, lr0 = 8, 3e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T)
    for k in range(1, T + 2):                                                  # a whole cycle: k - 1 = 0 .. T
        want = opt.param_groups[0]["lr"]
        assert abs(IR.cosine_lr(lr0, k, T) - want) <= 1e-15 * lr0 + 1e-19, (k, want)
        p.grad = torch.ones(1)
        opt.step(); sched.step()
    assert IR.cosine_lr(lr0, T + 1, T) <= 1e-19
    short = gu.load("g24_iql_short")["lr"]
    for k, want in enumerate(short, 1):
        assert abs(IR.cosine_lr(lr0, k, T) - want) <= 1e-15 * lr0


# ---- registry, config, ABI contract, refusals ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_call_algo_reaches_iql():
    """call_algo('iql' | 'IQL') reaches the class (which needs a GPU device); dara, bosa and igdf still raise."""
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.iql import IQL, step_config
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    assert issubclass(IQL, MOBODY)
    cfg = IR.iql_cfg(17, 6)
    for name in ("iql", "IQL"):
        with pytest.raises(RuntimeError, match="needs a GPU device"):
            call_algo(name, cfg, 3, "cpu")
    for name in ("dara", "bosa", "igdf"):
        with pytest.raises(NotImplementedError):
            call_algo(name, cfg, 3, "cpu")
    for bad, word in ((dict(lam=1.0), "lam"), (dict(lam=0.0), "lam"), (dict(max_step=0), "max_step"), (dict(action_dim=65), "action_dim")):
        with pytest.raises(ValueError, match=word):
            call_algo("iql", dict(cfg, **bad), 3, "cpu")
    with pytest.raises(NotImplementedError, match="max_step"):                  # a MOBODY config is not an IQL config
        call_algo("iql", gu.policy_cfg(17, 6), 3, "cpu")
    for attr in ("train", "select_action", "update_target", "save", "load"):
        assert callable(getattr(IQL, attr)), attr
    st = step_config(cfg)
    assert (st["advantage"], st["fake_batch_scale"], st["src_ratio"], st["trg_ratio"], st["penalty_type"]) == (1, 0, 1, 1, "none")
    assert "advantage" not in cfg                                              # the caller's dict is not touched


def test_mirror_cosine_matches_the_closed_form():
    from mobody_amd import ops
    for T in (8, 40, 500000):
        for k in (1, 2, T // 2, T, T + 1):
            want = np.float32(float(np.float32(3e-4)) * (1.0 + math.cos(math.pi * (k - 1) / T)) * 0.5)
            assert ops.cosine_lr(3e-4, k, T) == float(want)
            assert abs(ops.cosine_lr(3e-4, k, T) - IR.cosine_lr(3e-4, k, T)) <= 2.0 ** -23 * 3e-4


def test_builtin_iql_config_equals_reference_yaml():
    """The CLI's IQL defaults are the reference's four (identical) yaml files; load_yaml itself stays the file lookup it was."""
    from mobody_amd import train_mobody as tm
    want = json.load(open(os.path.join(gu.GOLDEN, "g24_iql_configs.json")))
    assert sorted(want) == ["ant", "halfcheetah", "hopper", "walker2d"]
    for env, cfg in want.items():
        assert tm._BUILTIN_IQL == cfg, env
        args = tm.build_parser().parse_args(["--policy", "IQL", "--env", env + "-friction", "--max_step", "1234"])
        got = tm.build_config(args, 17, 6, 1.0)
        for k, v in cfg.items():
            if k not in ("state_dim", "action_dim", "max_action", "max_step", "eval_freq"):      # (set from the env / the CLI)
                assert got[k] == v, (env, k)
        assert (got["max_step"], got["lam"], got["temp"], got["actor_lr"]) == (1234, 0.7, 3.0, 0.0003)
        got["lam"] = 0                                                        # a copy: the built-in table is not the caller's
    assert tm._BUILTIN_IQL["lam"] == 0.7 and not tm.uses_model("IQL")
    args = tm.build_parser().parse_args(["--policy", "DARA", "--env", "walker2d-friction"])
    with pytest.raises(FileNotFoundError):
        tm.build_config(args, 17, 6, 1.0)


ENTRIES = ("mobody_iql_value", "mobody_iql_critic", "mobody_iql_actor")


def test_new_symbols_declared_bound_and_exported(lib):
    from mobody_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    cites = {e: re.search(r"%s\s+iql\.py:\d+" % e, hdr) for e in ENTRIES}
    assert all(cites.values()), cites                                          # each entry cites the reference lines it replaces
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(const MobodyIql\* a, void\* stream\);" % name, hdr), name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and args[0] is C.POINTER(_lib.MobodyIql) and args[1] is _lib.vp
        assert hasattr(lib, name)
    assert re.search(r"\bint64_t mobody_iql_workspace\(const MobodyTrainDims\* d\);", hdr) and hasattr(lib, "mobody_iql_workspace")
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7
    fields = [f for f, _ in _lib.MobodyIql._fields_]
    decl = re.search(r"\bstruct MobodyIql \{(.*?)\};", hdr, flags=re.S).group(1)
    names = [n.strip(" *") for stmt in decl.split(";") if stmt.strip() for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]
    assert names == fields, (names, fields)
    assert C.sizeof(_lib.MobodyIql) == _lib.BLOCK_BYTES[_lib.MobodyIql] == 288
    assert [f for f, _ in _lib.MobodyHyper._fields_] == ["gamma", "tau", "max_action", "weight", "bc_coef", "q_weighted", "scale_q", "precision"]


PTR = 0x1000


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_name_the_field(lib, entry):
    """Every argument check runs before the first runtime call: the pointers below are never dereferenced."""
    from mobody_amd import _lib
    h = _lib.MobodyHyper(0.99, 0.005, 1.0, 0.0, 0.0, 0, 0, 0)

    def blk(A=6, lam=0.7, T_max=8, **ff):
        d = _lib.MobodyTrainDims(17, A, 64, 64, 128, 128)
        kw = dict(d=d, h=h, lam=lam, temp=3.0, T_max=T_max, v_blob=PTR, v_blob_T=PTR, q_blob=PTR, q_blob_T=PTR, qtarg_blob=PTR,
                  qtarg_blob_T=PTR, pi_blob=PTR, pi_blob_T=PTR, state=PTR, action=PTR, next_state=PTR, reward=PTR, not_done=PTR,
                  adv=PTR, grad=PTR, loss_out=PTR, workspace=PTR)
        kw.update(ff)
        return _lib.block(_lib.MobodyIql, **kw)
    bad = [(blk(A=65), "2 A > 128"), (blk(lam=0.0), "lam 0 outside (0, 1)"), (blk(lam=1.0), "lam 1 outside (0, 1)"),
           (blk(lam=float("nan")), "outside (0, 1)"), (blk(grad=None), "exactly one of grad"), (blk(m=PTR, v=PTR), "exactly one of grad"),
           (blk(grad=None, m=PTR, v=PTR, t=0), "step t must be >= 1")]
    if entry == "mobody_iql_actor":
        bad += [(blk(T_max=0), "T_max 0 < 1"), (blk(T_max=-3), "T_max -3 < 1")]
    for b, word in bad:
        assert getattr(lib, entry)(C.byref(b), None) == -1
        msg = lib.mobody_last_error().decode()
        assert msg.startswith(entry + ":") and word in msg, msg
    cls = _lib.MobodyIql
    assert getattr(lib, entry)(C.byref(cls(struct_bytes=C.sizeof(cls) - 1)), None) == -1
    assert "struct_bytes" in lib.mobody_last_error().decode()
    d = _lib.MobodyTrainDims(17, 65, 64, 64, 64, 64)
    assert lib.mobody_iql_workspace(C.byref(d)) == -1 and "2 A > 128" in lib.mobody_last_error().decode()
