"""Every policy in the learned model, on the device (`mobody_ens_evaluate_policy`, `mobody_eval_summary`,
MOBODYEnsembleDynamics.evaluate_policy(head=, members=), `evaluate_in_model` on the baselines, the CLI's `model_eval_dynamics` /
`model_eval_members` keys).

The reference is again the COMPOSITION of entry points the parent build has, with the same seed and call ids:
`ops.mlp3_forward(out_mode 1)` on the packed policy -- (S, A, 1) at head 0, (S, 2A, 1) and the slice [:, :A] at head 1 --
`mobody_ens_step` under the carried alive mask (with `elite_idx = member` in member mode) and the accounting of
tests/model_eval_ref.py on the host.  With discount 1 the fused call has to give the composition's bits."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import iql_ref as IR
import model_eval_policy_ref as pref
import model_eval_ref as ref
import test_hip_model_eval as E
from test_hip_fqe import cli_args, differing, packed_policy, snapshot

pytestmark = pytest.mark.gpu

SEED, CALL0 = E.SEED, E.CALL0
# The two extra shapes of head 1: A = 1, and A = 64, the largest A both layouts accept -- mobody_dyn_layout stops at A <= 64 and
# the Gaussian policy's 2 A <= 128 columns (mobody_mlp_layout's out_dim) stop at the same A = 64: the two limits coincide.
MODELS = dict(E.MODELS, a1=(17, 1, 4, False, 0.88), a64=(17, 64, 4, False, 0.88))
# Member mode's elites.  Member 6 of the walker weights never terminates within 5 steps (CPU oracle's step on the same Philox
# draws: all rows of length 5), so the evaluation's usual elites (0, 2, 3, 5, 6) would leave one group without a second length;
# with these five the oracle gives every member rows of length 1 and of length 5 (members 0..5 at 64 rows each: 40/15/4/5/0,
# 21/11/5/4/23, 10/9/2/4/39, 40/15/4/5/0, 11/10/2/6/35, 7/6/2/1/48 rows of length 1..5).  The test asserts it from the
# composition's own flags.
MEMBER_ELITES = (0, 1, 2, 4, 5)
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def setup(tag, head, mfma, dev):
    """(model, policy blob, mlp3_forward keywords, policy width) of one (shape, head, MFMA mode), built once."""
    from mobody_amd import packing
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    S, A, _, mopo, shift = MODELS[tag]
    if (tag, mfma) not in _cache:
        m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=gu.policy_cfg(S, A, mopo=int(mopo)))
        p = gu.gi.dyn_params(801, S, A, mopo=mopo)
        p["za_src3.bias" if mopo else "transition3.bias"][:, 0, 0] += np.float32(shift)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
        _cache[(tag, mfma)] = m
    if (tag, head, mfma) not in _cache:
        width = A if head == 0 else 2 * A
        pa = gu.policy_params(301, S, A)[0] if head == 0 else IR.iql_params(S, A, 311)[0]
        blob = packing.pack_mlp([{k[len("network."):]: v for k, v in pa.items()}], S, width, dev)
        _cache[(tag, head, mfma)] = (blob, gu.mlp_kw(blob, S, width, 1, mfma), width)
    return (_cache[(tag, mfma)],) + _cache[(tag, head, mfma)]


def init_obs(tag, B, dev):
    S, _, task = MODELS[tag][:3]
    x = gu.gi.walker_like_obs(np.random.default_rng(4), B, S)
    if task == 3:
        x[:, 0] = 0.6
    return torch.from_numpy(x).to(dev)


def compose(tag, head, mfma, dev, init, H, members=False, elites=E.ELITES, discount=1.0):
    """The composition.  Returns (row state as NumPy, final observation tensor, raw[H][B], terminal[H][B])."""
    from mobody_amd import ops
    S, A, task = MODELS[tag][:3]
    m, blob, akw, width = setup(tag, head, mfma, dev)
    B = init.shape[0]
    member = torch.from_numpy(pref.members(B, elites)).to(dev) if members else None
    st, obs, raws, terms = ref.new_state(B), init, [], []
    for t in range(H):
        out = ops.mlp3_forward(blob, S, width, 1, obs, out_mode=1, max_action=1.0, **akw)[0]
        act = out[:, :A].contiguous()
        alive = torch.from_numpy(st["alive"].astype(np.uint8)).to(dev)
        r = ops.dyn_step(m.packed(), S, A, task, obs, act, alive=alive, elite_idx=member, elites=elites, seed=SEED, call=CALL0 + t,
                         use_penalty=False, use_trg=True, **E.dyn_kw(m, mfma, 0))
        raw, term = r["raw_reward"].cpu().numpy().reshape(-1), r["terminal"].cpu().numpy().reshape(-1) != 0
        raws.append(raw); terms.append(term)
        ref.account(st, raw, r["penalty"].cpu().numpy().reshape(-1), term, discount)
        obs = r["next_obs"]
    return st, obs, np.array(raws), np.array(terms)


def workspace_floats(S, A, B, head):
    r4 = lambda n: (n + 3) // 4 * 4
    return r4(B * A) + r4(B * S) + r4(B) + r4(7 * B * S + 7 * B) + 2 * r4((B + 3) // 4) + head * r4(2 * B * A)


GUARD = 64                                                 # NaN sentinels behind the workspace


def fused(tag, head, mfma, dev, init, H, members=False, elites=E.ELITES, discount=1.0, state=None, resume=False, call0=CALL0,
          call_dev=None):
    """mobody_ens_evaluate_policy on a row state and a workspace pre-filled with a byte pattern; the words behind the workspace's
    closed-form size are NaN sentinels that must come back untouched."""
    from mobody_amd import _lib, ops
    S, A, task = MODELS[tag][:3]
    m, blob, akw, _ = setup(tag, head, mfma, dev)
    B = init.shape[0]
    if state is None:
        state = ops.eval_policy_state(B, S, dev)
        for v in state.values():                          # the first call has to initialise every word it owns
            v.view(torch.uint8).fill_(0xA5)
    need = workspace_floats(S, A, B, head)
    blk = _lib.block(_lib.MobodyEnsEvalPolicy, S=S, A=A, B=B, head=head)
    assert ops.load().mobody_ens_evaluate_policy_workspace(C.byref(blk)) == need, "the closed form is the size the library asks for"
    ws = torch.empty(need + GUARD, dtype=torch.float32, device=dev)
    ws.view(torch.uint8).fill_(0xA5)
    ws[need:] = float("nan")
    guard = ws[need:].clone()
    kw = E.dyn_kw(m, mfma, 0)
    got = ops.ens_evaluate_policy(m.packed(), blob, S, A, task, 1.0, None if resume else init, H, elites, SEED, call0, state, head=head,
                                  members=members, discount=discount, resume=resume, ws=ws, dyn_planes=kw["planes"],
                                  policy_blob_T=akw.get("blob_T"), precision=mfma, mopo=kw["mopo"], call_dev=call_dev)
    assert got is ws
    assert torch.equal(ws[need:].view(torch.int32), guard.view(torch.int32)), "a launch wrote behind the workspace"
    if not members:                                       # `member` is read and written in member mode only
        assert bool((state["member"].view(torch.uint8) == 0xA5).all())
    return state


def same_bytes(a, b, keys=None):
    return [k for k in (keys or a) if not torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))]


# ---- 1. head 0, mode 0 is mobody_ens_evaluate --------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 33, 257])
@pytest.mark.parametrize("tag", list(E.MODELS))
def test_head0_mode0_equals_the_existing_entry_bit_for_bit(tag, B, mfma, dev):
    init = init_obs(tag, B, dev)
    old = E.fused(tag, mfma, dev, init, 5)
    new = fused(tag, 0, mfma, dev, init, 5)
    assert same_bytes(old, new) == [] and set(new) == set(old) | {"member"}
    if B == 33:
        assert len(set(new["length"].tolist())) >= 3


# ---- 2. head 1 against the composition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,B", [(t, b) for t in E.MODELS for b in (1, 33, 257)] + [("a1", 33), ("a64", 33), ("a64", 257)])
def test_head1_equals_the_composition_bit_for_bit(tag, B, mfma, dev):
    init = init_obs(tag, B, dev)
    st, obs, raws, terms = compose(tag, 1, mfma, dev, init, 5)
    E.assert_state_bits(fused(tag, 1, mfma, dev, init, 5), st, obs)
    assert np.array_equal(st["length"], E.lengths_from_flags(terms)) and np.isfinite(st["ret"]).all()
    if tag in E.MODELS and B >= 33:                       # the case exercises the alive mask
        assert len(set(st["length"].tolist())) >= 3
    if tag in E.MODELS and B == 33:                       # and the head: the deterministic actor's run is another one
        assert not np.array_equal(st["ret"], compose(tag, 0, mfma, dev, init, 5)[0]["ret"])


# ---- 3. member mode ---------------------------------------------------------------------------------------------------------
def test_members_are_set_by_the_initialisation(dev):
    for B in (3, 33, 257):                                # B < G, B not a multiple of G
        init = init_obs("walker", B, dev)
        for elites in (E.ELITES, MEMBER_ELITES, (4,)):
            st = fused("walker", 0, "f32", dev, init, 0, members=True, elites=elites)
            assert st["member"].cpu().numpy().tolist() == pref.members(B, elites).tolist()
            E.assert_state_bits(st, ref.new_state(B), init)


@pytest.mark.parametrize("elites", [MEMBER_ELITES, E.ELITES], ids=["e01245", "e02356"])
@pytest.mark.parametrize("head", [0, 1])
@pytest.mark.parametrize("B", [33, 257])
def test_member_mode_equals_the_composition_bit_for_bit(B, head, elites, mfma, dev):
    init = init_obs("walker", B, dev)
    st, obs, raws, terms = compose("walker", head, mfma, dev, init, 5, members=True, elites=elites)
    got = fused("walker", head, mfma, dev, init, 5, members=True, elites=elites)
    E.assert_state_bits(got, st, obs)
    assert got["member"].cpu().numpy().tolist() == pref.members(B, elites).tolist()                  # the steps left it alone
    length = E.lengths_from_flags(terms)
    assert np.array_equal(st["length"], length)
    if B == 257 and elites is MEMBER_ELITES:              # every member group holds rows of at least two different lengths
        for g in range(len(elites)):                      # (the evaluation's usual elites include member 6, which never ends)
            assert len(set(length[np.arange(B) % len(elites) == g].tolist())) >= 2, g
    # the same seed with an elite per row and step is another run: the member reaches the sample kernel
    other = fused("walker", head, mfma, dev, init, 5, members=False, elites=elites)
    assert same_bytes(got, other, ("ret", "obs_state")) == ["ret", "obs_state"]
    assert int((got["ret"] != other["ret"]).sum()) >= 1


# ---- 4. resume and chunking -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,members", [(0, True), (1, False), (1, True)])
def test_resume_continues_the_row_state(head, members, mfma, dev):
    init = init_obs("walker", 33, dev)
    kw = dict(members=members, elites=MEMBER_ELITES)
    one = fused("walker", head, mfma, dev, init, 5, **kw)
    two = fused("walker", head, mfma, dev, init, 2, **kw)
    if members:                                           # `member` has to survive the resume: nothing may re-derive it
        assert two["member"].cpu().numpy().tolist() == pref.members(33, MEMBER_ELITES).tolist()
    fused("walker", head, mfma, dev, init, 3, state=two, resume=True, call0=CALL0 + 2, **kw)
    three = fused("walker", head, mfma, dev, init, 2, call_dev=torch.zeros(1, dtype=torch.int64, device=dev), **kw)
    fused("walker", head, mfma, dev, init, 3, state=three, resume=True, call_dev=torch.tensor([2], dtype=torch.int64, device=dev), **kw)
    for other in (two, three):
        assert same_bytes(one, other) == []
    assert len(set(one["length"].tolist())) >= 3
    if members:                                           # a resumed call reads `member` as it is: another assignment, another run
        swapped = fused("walker", head, mfma, dev, init, 2, **kw)
        swapped["member"].copy_(swapped["member"].flip(0))
        fused("walker", head, mfma, dev, init, 3, state=swapped, resume=True, call0=CALL0 + 2, **kw)
        assert same_bytes(one, swapped, ("ret",)) == ["ret"]


def make_dynamics(dev, **over):
    S, A, task = E.MODELS["walker"][:3]
    cfg = gu.policy_cfg(S, A, rng="device", seed=7, **over)
    return E.make_dynamics(E.dyn_params("walker"), S, A, E.TASKS[task], dev, cfg, rng="device", seed=13)


KEYS = ("returns", "lengths", "penalty_sums", "alive")
FIGURES = ("return_mean", "length_mean", "penalty_mean", "alive_frac", "return_member_means", "return_member_spread", "nan")


@pytest.mark.parametrize("head,members", [(0, True), (1, False), (1, True)])
def test_chunk_graph_equals_one_eager_call(head, members, mfma, dev):
    S, A = E.MODELS["walker"][:2]
    dyn = make_dynamics(dev)
    net, _ = packed_policy(S, A, head, dev, mfma)
    init = init_obs("walker", 33, dev)
    G = len(dyn.model.elites_host()) if members else 1

    def run(h, chunk):
        dyn._eval_calls = 0                                # the same call ids for both forms
        return dyn.evaluate_policy(net, init, h, chunk=chunk, head=head, members=members)

    same = lambda a, b: same_bytes(a, b, KEYS) == [] and all(a[k] == b[k] or a[k] != a[k] for k in FIGURES)
    eager = run(5, 0)
    assert dyn.eval_captures == 0 and eager["returns"].shape == (33 * G,) and len(eager["return_member_means"]) == G
    graph = run(5, 2)
    assert dyn.eval_captures == 1 and same(eager, graph)
    assert same(eager, run(5, 2)) and dyn.eval_captures == 1           # the same key replays
    # the figures are the summary's: one host read of words the kernel formed from the row state
    assert eager["return_mean"] == pytest.approx(float(eager["returns"].double().mean()), rel=1e-5)
    assert eager["length_mean"] == pytest.approx(float(eager["lengths"].double().mean()), rel=1e-6)
    assert eager["alive_frac"] == pytest.approx(float((eager["alive"] != 0).double().mean()), rel=1e-6)
    assert eager["penalty_mean"] == pytest.approx(float(eager["penalty_sums"].double().mean()), rel=1e-5) and eager["nan"] is False
    means = [float(eager["returns"].double()[g::G].mean()) for g in range(G)]
    assert eager["return_member_means"] == pytest.approx(means, rel=1e-5, abs=1e-6)
    assert eager["return_member_spread"] == max(eager["return_member_means"]) - min(eager["return_member_means"])
    if members:                                            # row b is start state b // G under member b % G
        assert dyn._evalp[1]["member"].tolist() == pref.members(33 * G, dyn.model.elites_host()).tolist()
    # the other head / mode is another key: a capture of its own, and the default path keeps its own state
    before = dyn.eval_captures
    if head == 0:
        plain = dyn.evaluate_policy(net, init, 5, chunk=2)
        assert dyn.eval_captures == before + 1 and plain["returns"].shape == (33,) and "nan" not in plain


@pytest.mark.parametrize("members", [False, True])
def test_a_nan_return_raises_the_flag_through_evaluate_policy(members, mfma, dev):
    """A NaN start state goes through the model's Swish layers into the row's reward: `nan` is True and the figures its rows
    reach are NaN (the flag is an int32 word, read through an int32 view); the clean start states give False."""
    S, A = E.MODELS["walker"][:2]
    dyn = make_dynamics(dev)
    net, _ = packed_policy(S, A, 1, dev, mfma)
    init = init_obs("walker", 33, dev)
    clean = dyn.evaluate_policy(net, init, 3, chunk=0, head=1, members=members)
    assert clean["nan"] is False and np.isfinite(clean["return_mean"]) and np.isfinite(clean["return_member_means"]).all()
    bad = init.clone()
    bad[7, 2] = float("nan")
    ev = dyn.evaluate_policy(net, bad, 3, chunk=0, head=1, members=members)
    assert ev["nan"] is True and ev["return_mean"] != ev["return_mean"]
    assert bool(torch.isnan(ev["returns"]).any()) and ev["return_member_spread"] != ev["return_member_spread"]


# ---- 5. discount 0.99 at head 1 against fp64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,B", [("walker", 33), ("walker", 257), ("ant", 33), ("mopo_walker", 33)])
def test_discounted_return_at_head1_against_fp64(tag, B, mfma, dev):
    """The existing bound 2 H 2^-24 sum_t |0.99^t raw_t| per row (test_hip_model_eval.test_discounted_return_against_fp64), over the
    composition's own rewards and flags."""
    H, disc = 5, float(np.float32(0.99))
    init = init_obs(tag, B, dev)
    st, obs, raws, terms = compose(tag, 1, mfma, dev, init, H, discount=disc)
    state = fused(tag, 1, mfma, dev, init, H, discount=disc)
    want, mag = ref.returns_f64(raws, terms, disc)
    err = np.abs(state["ret"].cpu().numpy().astype(np.float64) - want)
    bound = 2 * H * 2.0 ** -24 * mag
    print(f"discounted return head 1 {tag} B={B} H={H} {mfma}: worst err/bound {float(np.max(err / bound)):.4f} (max err {err.max():.3e})")
    assert (mag > 0).all() and (err <= bound).all()
    E.assert_state_bits(state, st, obs)


# ---- 6. mobody_eval_summary -----------------------------------------------------------------------------------------------
def summary_state(B, dev, seed=0):
    from test_model_eval_policy_ref import tables
    ret, pen, length, alive = tables(B, seed)
    host = dict(ret=ret, pen_sum=pen, length=length, alive=alive)
    return host, {k: torch.from_numpy(v).to(dev) for k, v in host.items()}


def run_summary(st, G, dev):
    from mobody_amd import ops
    out = torch.empty(4 * (G + 1) + 1 + 8, dtype=torch.float32, device=dev)
    out.view(torch.uint8).fill_(0xA5)
    ops.eval_summary(st, G, out=out)
    host = out.cpu()
    assert bool((host[4 * (G + 1) + 1:].view(torch.uint8) == 0xA5).all()), "a store behind out[G + 1][4] and the flag"
    return host[:4 * (G + 1)].numpy().reshape(G + 1, 4).copy(), int(host[4 * (G + 1):4 * (G + 1) + 1].view(torch.int32).item())


@pytest.mark.parametrize("G", [1, 5, 7])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1025])
def test_summary_against_fp64(B, G, dev):
    host, st = summary_state(B, dev)
    got, flag = run_summary(st, G, dev)
    want, mag, cnt = pref.summary64(host["ret"], host["pen_sum"], host["length"], host["alive"], G)
    assert flag == 0
    for row in range(G + 1):
        if cnt[row] == 0:                                  # B < G: the groups without rows
            assert np.isnan(got[row]).all()
            continue
        for col, m in ((0, mag[row, 0]), (2, mag[row, 1])):
            err, bound = abs(float(got[row, col]) - want[row, col]), pref.mean_bound(B, m, cnt[row])
            print(f"summary B={B} G={G} row {row} col {col}: err/bound {err / bound if bound else 0.0:.4f}")
            assert err <= bound, (row, col, err, bound)
        assert got[row, 1] == np.float32(want[row, 1]) and got[row, 3] == np.float32(want[row, 3])      # integer sums: exact
    again, _ = run_summary(st, G, dev)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))                                      # two runs, the same bits
    rest, _ = pref.summary32(host["ret"], host["pen_sum"], host["length"], host["alive"], G)
    assert np.array_equal(got.view(np.int32)[~np.isnan(got)], rest.view(np.int32)[~np.isnan(rest)])      # the restated order's bits


def test_summary_nan_rows_and_empty_groups(dev):
    host, st = summary_state(257, dev)
    clean, flag0 = run_summary(st, 5, dev)
    st["ret"][7] = float("nan")                            # group 7 % 5 = 2
    dirty, flag1 = run_summary(st, 5, dev)
    assert (flag0, flag1) == (0, 1) and np.isnan(dirty[2, 0]) and np.isnan(dirty[5, 0])
    keep = np.ones((6, 4), bool)
    keep[2, 0] = keep[5, 0] = False
    assert np.array_equal(clean.view(np.int32)[keep], dirty.view(np.int32)[keep])
    st["ret"][7] = float(host["ret"][7])
    st["pen_sum"][256] = float("nan")                      # group 256 % 5 = 1, thread 0's second row
    dirty, flag2 = run_summary(st, 5, dev)
    keep = np.ones((6, 4), bool)
    keep[1, 2] = keep[5, 2] = False
    assert flag2 == 1 and np.isnan(dirty[1, 2]) and np.isnan(dirty[5, 2]) and np.array_equal(clean.view(np.int32)[keep], dirty.view(np.int32)[keep])
    host, st = summary_state(3, dev)
    got, flag = run_summary(st, 7, dev)
    assert flag == 0 and np.isnan(got[3:7]).all() and not np.isnan(got[:3]).any() and not np.isnan(got[7]).any()
    assert got[:3, 0].tolist() == host["ret"].tolist()     # one row per group: its mean is the row


# ---- 7. training is untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("algo", ["IQL", "TD3_BC"])
def test_an_evaluation_between_train_steps_changes_nothing(algo, graph, mfma, dev):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task = E.MODELS["walker"][:3]
    init = init_obs("walker", 33, dev)

    def run(evaluate):
        torch.manual_seed(3)
        if algo == "IQL":
            cfg = dict(IR.iql_cfg(S, A, max_step=40), rng="device", seed=7, graph=graph)
        else:
            cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, advantage=1, trg_ratio=0.5)
        pol = call_algo(algo, cfg, 3, dev)
        dyn = make_dynamics(dev)
        pol.dynamics = dyn
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, E.TASKS[task], 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, E.TASKS[task], 1)
        ev = None
        for t in range(10):
            pol.train(src, tar, 64, None, None)
            if evaluate and t == 4:
                ev = pol.evaluate_in_model(init, 5, chunk=2, members=True)
        torch.cuda.synchronize()
        losses = pol.losses()
        pol.dynamics = None                                # the model is not training state (and only one run used it)
        state = snapshot(pol)
        state.update({"src." + k: v for k, v in snapshot(src).items()})
        state.update({"tar." + k: v for k, v in snapshot(tar).items()})
        state["torch.cpu_rng"], state["torch.cuda_rng"] = torch.get_rng_state(), torch.cuda.get_rng_state()
        return pol, dyn, state, losses, ev

    a, adyn, sa, la, ev = run(True)
    b, bdyn, sb, lb, _ = run(False)
    assert ev is not None and adyn.eval_captures == 1 and np.isfinite(ev["return_mean"]) and len(ev["return_member_means"]) == 5
    assert ev["returns"].shape == (33 * 5,) and ev["nan"] is False
    if graph:
        assert a._graph is not None and b._graph is not None
    assert a.eval_policy()[1] == (1 if algo == "IQL" else 0) and a.total_it == b.total_it == 10
    assert any(k.endswith("._draws") for k in sa) and any(k.endswith("blob_T") for k in sa) and len(sa) > 20
    bad = differing(sa, sb)
    assert bad == [], " ".join(bad)
    assert la == lb and adyn._calls == bdyn._calls == 0 and adyn._train_calls == bdyn._train_calls


# ---- 8. precision mismatch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,members", [(0, False), (0, True), (1, False), (1, True)])
def test_a_policy_in_another_format_is_evaluated_in_the_models(head, members, dev, monkeypatch):
    """A policy at bf16x3 (where its class's F16_RANGE fallback leaves it) in an f16x2 model: the evaluator builds the policy's T
    blob in the model's format for the evaluation -- the result is that of the same weights packed at f16x2 -- and leaves the
    policy's own planes alone."""
    monkeypatch.setenv("MOBODY_MFMA", "f16x2")
    S, A = E.MODELS["walker"][:2]
    dyn = make_dynamics(dev, mfma="f16x2")
    assert dyn.precision == 4
    init = init_obs("walker", 33, dev)
    fallen, _ = packed_policy(S, A, head, dev, "bf16x3")
    native, _ = packed_policy(S, A, head, dev, "f16x2")
    assert torch.equal(fallen.blob, native.blob) and not torch.equal(fallen.blob_T.view(torch.int32), native.blob_T.view(torch.int32))
    planes = fallen.blob_T.clone()
    out = []
    for net in (fallen, native):
        for chunk in (0, 2):
            dyn._eval_calls = 0
            out.append(dyn.evaluate_policy(net, init, 5, chunk=chunk, head=head, members=members))
    figures = FIGURES if head or members else FIGURES[:4]  # (0, False): the old entry's path, which holds the rule as well
    for o in out[1:]:
        assert same_bytes(out[0], o, KEYS) == [] and all(out[0][k] == o[k] for k in figures)
    if not (head or members):                              # ... with the old entry's bits: the new entry at head 0 agrees
        dyn._eval_calls = 0
        new = dyn.evaluate_policy(fallen, init, 5, chunk=0, entry="policy")
        assert same_bytes(out[0], new, KEYS) == [] and "nan" in new and "nan" not in out[0]
    assert torch.equal(fallen.blob_T.view(torch.int32), planes.view(torch.int32)) and fallen.precision == 3
    assert len(set(out[0]["lengths"].tolist())) >= 3


# ---- 9. CLI ----------------------------------------------------------------------------------------------------------------
TAGS = ["test/model target return", "test/model target normalized score", "test/model episode length", "test/model penalty",
        "test/model alive frac"]
MEMBER_TAGS = ["test/model return member spread"] + [f"test/model return member e{k}" for k in range(5)]


def cli_run(argv, params, out_dir, monkeypatch=None):
    """(policy state with the model detached + the buffers' state, scalar rows) of one CLI run."""
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo import utils
    made = []
    init = utils.ReplayBuffer.__init__
    monkeypatch.setattr(utils.ReplayBuffer, "__init__", lambda self, *a, **k: (init(self, *a, **k), made.append(self))[0])
    try:
        pol = tm.main(argv + ["--dir", str(out_dir), "--params", json.dumps(params)])
    finally:
        monkeypatch.setattr(utils.ReplayBuffer, "__init__", init)
    torch.cuda.synchronize()
    model = pol.dynamics
    if not tm.uses_model(argv[1]):
        pol.dynamics = None                                # the evaluator's model is not the policy's training state
    state = snapshot(pol)
    pol.dynamics = model
    for i, rb in enumerate(made):
        state.update({"buffer%d.%s" % (i, k): v for k, v in snapshot(rb).items()})
    state["torch.cpu_rng"], state["torch.cuda_rng"] = torch.get_rng_state(), torch.cuda.get_rng_state()
    state = {k: v for k, v in state.items() if "model_eval_" not in k}       # (the merged config's keys under test)
    csv = [f for d, _, fs in os.walk(out_dir) for f in (os.path.join(d, x) for x in fs) if f.endswith("scalars.csv")]
    rows = [ln.strip().split(",") for ln in open(csv[0])][1:]
    return pol, state, rows


@pytest.mark.parametrize("policy", ("TD3_BC", "IQL", "DARA", "IGDF", "BOSA"))
def test_cli_evaluates_a_baseline_in_the_model_and_leaves_training_alone(policy, tmp_path, monkeypatch, capsys):
    """12 steps, eval_freq 4 (the sizes of test_hip_fqe's CLI test): model_eval_dynamics = 1 with 8 episodes of 5 steps, without and
    with model_eval_members, against the run without the keys."""
    argv, params = cli_args(policy, tmp_path, monkeypatch)
    argv += ["--train_dynamics", "0"]
    keys = dict(model_eval_dynamics=1, model_eval_episodes=8, model_eval_horizon=5)
    pol0, s0, r0 = cli_run(argv, params, tmp_path / "plain", monkeypatch)
    assert pol0.dynamics is None and not [r for r in r0 if r[0].startswith("test/model ")]
    capsys.readouterr()
    for name, extra, tags in (("on", {}, TAGS), ("members", dict(model_eval_members=1), TAGS + MEMBER_TAGS)):
        pol, s, r = cli_run(argv, dict(params, **keys, **extra), tmp_path / name, monkeypatch)
        assert "ignored" not in capsys.readouterr().out and pol.dynamics is not None
        logged = [x for x in r if x[0].startswith("test/model ")]
        assert sorted(x[0] for x in logged if int(x[1]) == 4) == sorted(tags)              # once per tag ...
        assert sorted(int(x[1]) for x in logged if x[0] == tags[0]) == [4, 8, 12] and len(logged) == 3 * len(tags)   # ... at the cadence
        assert [x for x in r if not x[0].startswith("test/model ")] == r0                    # every other scalar row is what it was
        assert not [x for x in r if x[0] == "test/target return"]                            # the simulator's name stays free
        vals = {(x[0], int(x[1])): float(x[2]) for x in logged}
        assert all(1.0 <= vals[("test/model episode length", t)] <= 5.0 and 0.0 <= vals[("test/model alive frac", t)] <= 1.0 for t in (4, 8, 12))
        if extra:
            mm = [vals[(f"test/model return member e{k}", 12)] for k in range(5)]
            if all(v == v for v in mm):
                assert vals[("test/model return member spread", 12)] == pytest.approx(max(mm) - min(mm), rel=1e-6, abs=1e-12)
        bad = differing(s, s0)                                                               # nets, moments, counts, draws, generators
        assert bad == [], name + ": " + " ".join(bad)
        assert any(k.endswith("._draws") for k in s) and len(s) > 20


def test_cli_old_behaviour_stays(tmp_path, monkeypatch, capsys):
    from mobody_amd import train_mobody as tm
    # a baseline without model_eval_dynamics: the `ignored` line, once (and model_eval_members alone builds nothing)
    argv, params = cli_args("TD3_BC", tmp_path, monkeypatch)
    capsys.readouterr()
    pol, _, rows = cli_run(argv, dict(params, model_eval_episodes=8, model_eval_members=1), tmp_path / "bc", monkeypatch)
    out = capsys.readouterr().out
    assert out.count("model_eval_episodes / model_eval_horizon ignored: TD3_BC has no model to evaluate in") == 1
    assert pol.dynamics is None and not [r for r in rows if r[0].startswith("test/model ")]
    # MOBODY: model_eval_members = 0 logs exactly today's rows; model_eval_dynamics is ignored with one line; = 1 adds the six tags
    argv, params = cli_args("MOBODY", tmp_path, monkeypatch)
    keys = dict(model_eval_episodes=8, model_eval_horizon=5)
    _, _, today = cli_run(argv, dict(params, **keys), tmp_path / "today", monkeypatch)
    capsys.readouterr()
    _, _, zero = cli_run(argv, dict(params, model_eval_members=0, model_eval_dynamics=1, **keys), tmp_path / "zero", monkeypatch)
    assert capsys.readouterr().out.count("model_eval_dynamics ignored: MOBODY builds its own model") == 1
    assert zero == today and sorted({r[0] for r in today if r[0].startswith("test/model ") and "error" not in r[0]}) == sorted(TAGS)
    _, _, mem = cli_run(argv, dict(params, model_eval_members=1, **keys), tmp_path / "mem", monkeypatch)
    skip = set(TAGS + MEMBER_TAGS)                         # member mode is another draw: the five figures are other numbers
    assert [r for r in mem if r[0] not in skip] == [r for r in today if r[0] not in skip]
    assert sorted({r[0] for r in mem if r[0] in skip}) == sorted(skip)
    assert not [r for r in today + mem if r[0] == "test/target return"]
