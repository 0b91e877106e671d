"""GPU checks of fitted Q evaluation.

mobody_fqe_target and mobody_fqe_value against the composition -- ops.mlp3_forward(out_mode 1), a torch slice [:, :A], ops.mlp3_forward
of the twin-Q, (q[0] + q[1]) * 0.5 -- BIT FOR BIT, on NaN-filled outputs and workspaces with guard words behind them; a NaN row kept
to itself; the value words against fp64 means of q_out within R.mean_tolerance.  One FQE step against the same launches issued by the
test on the rows the gather's CPU twin draws; 10 replayed steps against 10 eager ones; 20 steps against the fp64 restatement
(tests/fqe_ref.py); constant rewards; the six algorithms through the CLI with and without the fqe_* keys; warm start, reset, health.

Shapes are the smallest at which these kernels can go wrong (R.TARGET_ROWS, R.VALUE_ROWS): one row short of and past a workgroup, more
than four workgroups, one row per reducer thread and a second trip."""
import json
import os

import numpy as np
import pytest
import torch

import bosa_graph_cases as GC
import fqe_ref as R
from oracle import mobody_oracle as O
from test_hip_bosa import GUARD, NAN, guard_intact

pytestmark = pytest.mark.gpu
TAGS = ("test/fqe value", "test/fqe head gap", "test/fqe td loss", "test/fqe seconds")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


T = lambda p: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()}


def packed_policy(S, A, head, dev, mode="f32", ma=1.0, seed=5):
    from mobody_amd import ops
    from mobody_amd.algo.offline_offline.mobody import _PackedNet
    params = R.policy_params(seed, head, S, A)
    net = _PackedNet(S, A if head == 0 else 2 * A, 1, ("",), dev, out_mode=1, max_action=ma, init=False, precision=ops.prec_id(mode))
    net.load_state_dict(T(GC.state_dict(params, ("",))))
    return net, params


def packed_q(S, A, dev, mode="f32", seed=6):
    from mobody_amd import ops
    from mobody_amd.algo.offline_offline.mobody import _PackedNet
    params = GC.mlp_params(seed, S + A, 1, 2)
    net = _PackedNet(S + A, 1, 2, ("network1.", "network2."), dev, init=False, precision=ops.prec_id(mode))
    net.load_state_dict(T(GC.state_dict(params, ("network1.", "network2."))))
    return net, params


class Nets:
    """A frozen policy of one head form and a twin-Q on the device (fixed seeds), and the two entries on guarded, NaN-filled buffers."""

    def __init__(self, S, A, head, dev, mode="f32", ma=1.0):
        self.policy, self.pp = packed_policy(S, A, head, dev, mode, ma)
        self.q, self.pq = packed_q(S, A, dev, mode)
        self.S, self.A, self.head, self.ma, self.dev = S, A, head, ma, dev

    def composition(self, s):
        """(0.5 (q0 + q1) [N], a [N, A], q [2, N]) with torch ops between the two forwards."""
        from mobody_amd import ops
        p, q, N = self.policy, self.q, s.shape[0]
        z = ops.mlp3_forward(p.blob, self.S, p.out_dim, 1, s, out_mode=1, max_action=self.ma, blob_T=p.blob_T, precision=p.precision)[0]
        a = z[:, :self.A].contiguous()
        qq = ops.mlp3_forward(q.blob, self.S + self.A, 1, 2, s, a, blob_T=q.blob_T, precision=q.precision).reshape(2, N)
        torch.cuda.synchronize()
        return (qq[0] + qq[1]) * 0.5, a, qq

    def target(self, s2, want_action=True):
        from mobody_amd import ops
        N, A = s2.shape[0], self.A
        qbuf = torch.full((N + GUARD,), NAN, device=self.dev)
        abuf = torch.full((N * A + GUARD,), NAN, device=self.dev)
        blk = ops.fqe_target_block(self.policy, self.head, self.q, s2, qbuf[:N], action_out=abuf[:N * A] if want_action else None)
        words = ops.fqe_target_workspace(blk, self.dev).numel()
        assert words == R.workspace_floats(self.head, A, N)
        ws = torch.full((words + GUARD,), NAN, device=self.dev)
        blk.workspace = ws.data_ptr()
        ops.fqe_target(blk)
        torch.cuda.synchronize()
        assert guard_intact(ws) and guard_intact(qbuf) and guard_intact(abuf), "mobody_fqe_target wrote behind a buffer"
        if not want_action:
            assert bool(torch.isnan(abuf).all())
        return qbuf[:N].clone(), abuf[:N * A].reshape(N, A).clone()

    def value(self, s0, want_q=True):
        from mobody_amd import ops
        B = s0.shape[0]
        qbuf = torch.full((2 * B + GUARD,), NAN, device=self.dev)
        out = torch.full((4 + GUARD,), NAN, device=self.dev)
        flag = torch.full((1 + GUARD,), 0x7FC00000, dtype=torch.int32, device=self.dev)
        blk = ops.fqe_value_block(self.policy, self.head, self.q, s0, out[:4], flag[:1], q_out=qbuf[:2 * B] if want_q else None)
        words = ops.fqe_value_workspace(blk, self.dev).numel()
        assert words == R.workspace_floats(self.head, self.A, B)
        ws = torch.full((words + GUARD,), NAN, device=self.dev)
        blk.workspace = ws.data_ptr()
        ops.fqe_value(blk)
        torch.cuda.synchronize()
        assert guard_intact(ws) and guard_intact(qbuf) and guard_intact(out) and bool((flag[1:] == 0x7FC00000).all()), "wrote behind a buffer"
        return out[:4].clone(), int(flag[0]), qbuf[:2 * B].reshape(2, B).clone()


def states(S, N, dev, seed=0):
    return torch.from_numpy(GC.target_inputs(S, 1, N, seed)[0]).to(dev)


# ---- 1. mobody_fqe_target ----------------------------------------------------------------------------------------------------------
def check_target(S, A, N, head, dev, mode, ma):
    k = Nets(S, A, head, dev, mode, ma)
    s2 = states(S, N, dev)
    want, a_want, _ = k.composition(s2)
    got, a_got = k.target(s2)
    assert bits_equal(got, want) and bits_equal(a_got, a_want), (S, A, N, head, mode, ma)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0 and float(a_want.abs().max()) <= ma
    got2, _ = k.target(s2, want_action=False)
    assert bits_equal(got2, want)
    return k, s2, want


@pytest.mark.parametrize("head", R.HEADS)
@pytest.mark.parametrize("S,A", R.TARGET_SHAPES)
def test_target_has_the_bits_of_the_composition(S, A, head, dev):
    for N in R.TARGET_ROWS:
        for ma in R.MAX_ACTIONS:
            check_target(S, A, N, head, dev, "f32", ma)


@pytest.mark.parametrize("head", R.HEADS)
@pytest.mark.parametrize("mode", ("f16x2", "bf16x3"))
def test_target_has_the_bits_of_the_composition_in_the_split_modes(mode, head, dev):
    for N in (33, 257):
        check_target(17, 6, N, head, dev, mode, 1.0)


def test_target_gaussian_head_at_the_128_column_edge(dev):
    for N in (33, 257):
        check_target(17, 64, N, 1, dev, "f32", 1.0)


@pytest.mark.parametrize("mode", ("bf16", "bf16x2"))
def test_target_refuses_the_lower_modes_by_name(mode, dev):
    from mobody_amd import _lib
    k = Nets(17, 6, 0, dev, mode)
    with pytest.raises(_lib.MobodyError, match=r"mobody_fqe_target: precision \d: must be one of 0 \(f32\), 3 \(bf16x3\), 4 \(f16x2\)"):
        k.target(torch.zeros(8, 17, device=dev))


@pytest.mark.parametrize("head", R.HEADS)
def test_target_keeps_a_nan_row_to_itself(head, dev):
    k, s2, want = check_target(17, 6, 257, head, dev, "f32", 1.0)
    for row, col in ((0, 0), (130, 16), (256, 5)):
        bad = s2.clone()
        bad[row, col] = NAN
        got, _ = k.target(bad)
        assert bool(torch.isnan(got[row]))
        keep = torch.ones(257, dtype=torch.bool, device=dev)
        keep[row] = False
        assert bits_equal(got[keep], want[keep]), "every other row keeps its bits"


# ---- 2. mobody_fqe_value -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", R.HEADS)
@pytest.mark.parametrize("B", R.VALUE_ROWS)
def test_value_words(B, head, dev):
    k = Nets(17, 6, head, dev)
    s0 = states(17, B, dev, seed=1)
    _, _, q_want = k.composition(s0)
    out, flag, q = k.value(s0)
    assert bits_equal(q, q_want), "q_out has the composition's bits"
    qn = q.cpu().numpy()
    want, tol = R.value_words(qn), R.mean_tolerance(qn)
    got = out.cpu().numpy().astype(np.float64)
    print("B=%d head %d: means vs fp64, error / tolerance:" % (B, head), np.round(np.abs(got[:3] - want[:3]) / tol, 4))
    assert (np.abs(got[:3] - want[:3]) <= tol).all()
    assert got[3] == float(np.abs(qn[0] - qn[1]).max()), "the gap is exact"          # fp32 subtraction of fp32 values, then a maximum
    assert flag == 0
    out2, flag2, _ = k.value(s0, want_q=False)
    assert bits_equal(out2, out) and flag2 == 0, "two runs give the same bits"
    bad = s0.clone()
    bad[B // 2, 3] = NAN
    outn, flagn, qb = k.value(bad)
    assert flagn == 1 and bool(torch.isnan(outn).all()) and bool(torch.isnan(qb[:, B // 2]).all())
    keep = torch.ones(B, dtype=torch.bool, device=dev)
    keep[B // 2] = False
    assert bits_equal(qb[:, keep], q_want[:, keep])


@pytest.mark.parametrize("mode", ("f16x2", "bf16x3"))
def test_value_in_the_split_modes(mode, dev):
    k = Nets(17, 6, 1, dev, mode)
    s0 = states(17, 257, dev, seed=1)
    _, _, q_want = k.composition(s0)
    out, flag, q = k.value(s0)
    assert bits_equal(q, q_want) and flag == 0 and bool(torch.isfinite(out).all())


# ---- 3. the class --------------------------------------------------------------------------------------------------------------------
def buffer(dev, data):
    from mobody_amd.algo import utils
    s, a, s2, r, nd = data
    rb = utils.ReplayBuffer(s.shape[1], a.shape[1], dev, max_size=s.shape[0], rng="device", seed=2)
    rb.convert_D4RL(dict(observations=s, actions=a, next_observations=s2, rewards=r.reshape(-1), terminals=1.0 - nd.reshape(-1)))
    return rb


def make_fqe(dev, head, mode="f32", bs=33, cfg=R.TRAJ, rng="device", pseed=None):
    from mobody_amd.fqe import FQE
    S, A = cfg["S"], cfg["A"]
    pol, pp = packed_policy(S, A, head, dev, mode, seed=(40 + head) if pseed is None else pseed)
    f = FQE(pol, head, S, A, 1.0, cfg["gamma"], dev, mode, lr=cfg["lr"], tau=cfg["tau"], batch_size=bs, seed=cfg["seed"], rng=rng)
    return f, pp


def fqe_state(f):
    o = f.optimizer
    return dict(q=f.q.blob.clone(), q_T=f.q.blob_T.clone(), targ=f.q_target.blob.clone(), targ_T=f.q_target.blob_T.clone(), m=o.m.clone(),
                v=o.v.clone(), counts=torch.tensor([o.t, f._calls]))


def same_state(a, b):
    return [k for k in a if not (bits_equal(a[k], b[k]) if a[k].dtype == torch.float32 else torch.equal(a[k], b[k]))]


@pytest.mark.parametrize("head", R.HEADS)
@pytest.mark.parametrize("bs", R.STEP_BS)
def test_one_step_is_the_entries_on_the_twins_rows(bs, head, dev):
    """FQE.fit(tar, 1) against ops.fqe_target + the existing critic op called here, on the rows the gather's CPU twin draws."""
    from mobody_amd import _lib, ops
    c = R.TRAJ
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"])
    tar = buffer(dev, data)
    draws0 = tar._draws
    f, _ = make_fqe(dev, head, bs=bs, rng="numpy")
    g, _ = make_fqe(dev, head, bs=bs, rng="numpy")
    assert same_state(fqe_state(f), fqe_state(g)) == [], "two objects of one seed start from the same bits"
    assert f.fit(tar, 1) and f.optimizer.t == 1 and f._calls == 1 and tar._draws == draws0
    idx = R.draw(O.rng_index, c["seed"], 1, bs, c["rows"])
    batch = tuple(torch.from_numpy(np.ascontiguousarray(x[idx])).to(dev) for x in data)
    assert all(bits_equal(x, y) for x, y in zip(f._buf["batch"], batch)), "the step's rows are the twin's"
    qn = torch.empty(bs, device=dev)
    blk = ops.fqe_target_block(g.policy_net, head, g.q_target, batch[2], qn)
    ws = ops.fqe_target_workspace(blk, dev)
    blk.workspace = ws.data_ptr()
    ops.fqe_target(blk)
    dims = ops.train_dims(c["S"], c["A"], bs, bs)
    hyp = _lib.MobodyHyper(c["gamma"], c["tau"], 1.0, 1.0, 0.0, 0, 1, 0)
    o, loss = g.optimizer, torch.zeros(1, device=dev)
    ops.critic_update(dims, hyp, None, g.q.blob, g.q.blob_T, g.q_target.blob, batch, o.m, o.v, 1, o.lr, loss, ops.train_workspace(dims, dev),
                      q_next=qn, qtarg_blob_T=g.q_target.blob_T)
    o.t, g._calls = 1, 1
    torch.cuda.synchronize()
    assert same_state(fqe_state(f), fqe_state(g)) == []
    assert bits_equal(f._loss, loss) and float(loss) > 0
    assert not bits_equal(f.q.blob, f.q_target.blob)


@pytest.mark.parametrize("head", R.HEADS)
def test_replayed_steps_are_eager_steps(head, dev):
    """10 replayed steps == 10 eager steps at bs 8 and then at bs 33, bit for bit: one capture per batch size."""
    c = R.TRAJ
    tar = buffer(dev, R.dataset(c["rows"], c["S"], c["A"], c["seed"]))
    f, _ = make_fqe(dev, head, bs=8, rng="device")
    e, _ = make_fqe(dev, head, bs=8, rng="numpy")
    for n, bs in enumerate(R.STEP_BS, 1):
        f.batch_size = e.batch_size = bs
        assert f.fit(tar, 11) and e.fit(tar, 11)             # the first step at a size is eager: 10 replays
        torch.cuda.synchronize()
        assert f.captures == n and f.replays == 10 * n and e.captures == 0 and e.replays == 0
        assert same_state(fqe_state(f), fqe_state(e)) == []
        assert f._ctr[:2].tolist() == [11 * n, 11 * n] and f.optimizer.t == 11 * n, "the device words are the counts"
    assert f.fit(tar, 3) and e.fit(tar, 3) and f.captures == 2 and f.replays == 23        # the same size again: no new capture
    assert same_state(fqe_state(f), fqe_state(e)) == []


@pytest.mark.parametrize("mode", ("f32", "f16x2"))
@pytest.mark.parametrize("head", R.HEADS)
def test_short_trajectory_against_fp64(head, mode, dev):
    """20 steps at bs 33, (17, 6), rows from the gather's CPU twin: parameters, target parameters and value()'s words against the fp64
    restatement within 4 x what the float32 NumPy restatement differs from it (R.TRAJ_F32_DIFF: head 0 parameters 1.72e-6, target
    1.59e-7, value words 4.9e-8; head 1 3.93e-7, 1.06e-7, 5.2e-8), f32 and f16x2 alike."""
    from mobody_amd import fqe, packing
    c = R.TRAJ
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"])
    tar = buffer(dev, data)
    f, pp = make_fqe(dev, head, mode=mode, bs=c["bs"])
    q0 = R.params_from_state_dict({k: v.numpy() for k, v in fqe.initial_state_dict(c["S"], c["A"], c["seed"]).items()})
    ref = R.Fqe(q0, pp, head, c["A"], 1.0, c["gamma"], c["tau"], c["lr"])
    for k in range(1, c["steps"] + 1):
        ref.step(*[x[R.draw(O.rng_index, c["seed"], k, c["bs"], c["rows"])] for x in data])
    assert f.fit(tar, c["steps"])
    s0 = data[0][::50]
    v = f.value(s0)
    flat = lambda net: np.concatenate([m[f"network.{li}.{wb}"].cpu().numpy().reshape(-1).astype(np.float64)
                                       for m in packing.unpack_mlp(net.blob, net.in_dim, net.out_dim, net.members)
                                       for li in (0, 2, 4) for wb in ("weight", "bias")])
    got = dict(param=np.abs(flat(f.q) - ref.flat()).max(), targ=np.abs(flat(f.q_target) - ref.flat("q_targ")).max(),
               value=np.abs(np.array([v["q1"], v["q2"], v["value"], v["head_gap"]]) - ref.value(s0)).max())
    print("head %d %s: HIP vs fp64 after %d steps:" % (head, mode, c["steps"]), got, "allowed: 4 x", R.TRAJ_F32_DIFF[head])
    assert not v["nan"]
    for k, x in got.items():
        assert x <= 4 * R.TRAJ_F32_DIFF[head][k], (k, x)


def test_constant_rewards(dev):
    """r = 1, not_done = 1, gamma 0.9: the value is 10.  R.CONST['steps'] steps, found on the CPU (the fp64 restatement is within 2 %)."""
    c = R.CONST
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"], const_reward=True)
    tar = buffer(dev, data)
    f, _ = make_fqe(dev, 0, bs=c["bs"], cfg=c, pseed=41)
    assert f.fit(tar, c["steps"])
    v = f.value(data[0][:64])
    print("constant rewards, HIP, %d steps:" % c["steps"], v)
    assert abs(v["value"] - 10.0) <= 0.05 * 10.0 and not v["nan"] and f.replays == c["steps"] - 1


def test_warm_start_and_reset(dev):
    c = R.TRAJ
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"])
    tar = buffer(dev, data)
    f, _ = make_fqe(dev, 1, bs=8)
    s0 = data[0][::50]
    runs = []
    for _ in range(2):                                     # fqe_warm_start = 0: reset() before every evaluation
        f.prepare(warm_start=False)
        assert f.fit(tar, 6)
        runs.append((fqe_state(f), f.value(s0)))
    assert same_state(runs[0][0], runs[1][0]) == [] and runs[0][1] == runs[1][1] and f.optimizer.t == 6
    f.prepare(warm_start=True)                             # 1: the next evaluation starts from the last one's counts
    assert f.optimizer.t == 6 and f._calls == 6 and f.fit(tar, 6) and f.optimizer.t == 12 and f._calls == 12
    assert same_state(fqe_state(f), runs[0][0]) != []
    f.reset()
    assert f.optimizer.t == 0 and f._calls == 0 and float(f.optimizer.m.abs().max()) == 0


def test_health_fault_skips_the_evaluation_and_falls_back(dev):
    """A weight of 300 in FQE's own W2 at f16x2: fit() raises FQE's F16_RANGE bit and returns False with the warning, the words bound
    before (the policy's) stay clear and bound, and the next evaluation runs at bf16x3."""
    from mobody_amd import _lib, ops
    c = R.TRAJ
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"])
    tar = buffer(dev, data)
    policy_words = ops.health_block(dev)
    ops.health_clear()
    f, _ = make_fqe(dev, 0, mode="f16x2", bs=8)
    f.q.blob[f.q.layout.w2 + 5] = 300.0
    with pytest.warns(UserWarning, match="FQE health words F16_RANGE.*skipped.*bf16x3"):
        assert f.fit(tar, 3) is False
    assert f.fault == "F16_RANGE" and int(f._health[0]) == _lib.HEALTH_F16_RANGE
    assert ops.health_bound(dev) is policy_words and ops.health_read(policy_words) == (0, 0)
    f.prepare(warm_start=True)
    assert f.precision == 3 and f.q.precision == 3 and f.q_target.precision == 3 and f.fault is None and int(f._health[0]) == 0
    assert f.fit(tar, 3) and f.optimizer.t == 3
    v = f.value(data[0][::50])
    assert not v["nan"] and np.isfinite(v["value"])
    assert ops.health_read(policy_words) == (0, 0)


# ---- 4. the CLI: isolation -------------------------------------------------------------------------------------------------------------
def is_scratch(name):
    return name in ("ws", "gws", "tws") or name.endswith("_ws")


def snapshot(obj, out=None, path="", seen=None, depth=0):
    """Every tensor and every int / float / bool reachable from `obj` through attributes, lists, tuples and dicts of this package's
    objects: nets, moments, step counts, counter words, noise counts.  Left out: graph keys (device addresses and object ids) and
    scratch workspaces (`ws`, `gws`, `tws`, `*_ws`: torch.empty storage whose padding no launch writes holds what the allocator handed
    out)."""
    out, seen = ({} if out is None else out), (set() if seen is None else seen)
    if isinstance(obj, (bool, int, float)):
        out[path] = obj
        return out
    if id(obj) in seen or depth > 6:
        return out
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        out[path] = obj.detach().cpu().clone()
    elif isinstance(obj, (list, tuple)):
        for i, x in enumerate(obj):
            snapshot(x, out, "%s[%d]" % (path, i), seen, depth + 1)
    elif isinstance(obj, dict):
        for k, x in obj.items():
            if isinstance(k, (str, int)) and not str(k).startswith("fqe_") and not is_scratch(str(k)):   # (fqe_*: the keys under test)
                snapshot(x, out, "%s[%r]" % (path, k), seen, depth + 1)
    elif type(obj).__module__.startswith("mobody_amd") and hasattr(obj, "__dict__"):
        for k, x in vars(obj).items():
            if not k.endswith("_key") and not is_scratch(k):
                snapshot(x, out, path + "." + k, seen, depth + 1)
    return out


def differing(a, b):
    bad = [k for k in sorted(set(a) | set(b)) if k not in a or k not in b]
    for k in set(a) & set(b):
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor):
            same = x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)) if x.numel() else True
        else:
            same = x == y or (x != x and y != y)
        if not same:
            bad.append(k)
    return bad


def cli_args(policy, tmp_path, monkeypatch):
    common = ["--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", "1", "--rng", "device",
              "--src_rows", "600", "--tar_rows", "300", "--max_step", "12", "--eval_freq", "4", "--log_every", "6"]
    params = dict(batch_size=8, graph=1)
    if policy == "MOBODY":
        common += ["--penalty_type", "none", "--src_rollout_batch_size", "400", "--trg_rollout_batch_size", "100"]
    if policy in ("DARA", "IGDF", "BOSA"):
        if policy == "DARA":
            from test_hip_dara import config_tree
            root = config_tree(tmp_path)
        elif policy == "IGDF":
            from test_hip_igdf import config_tree
            root = config_tree(tmp_path)
        else:
            from test_hip_bosa_class import config_tree
            root = config_tree(tmp_path, vae_iteration=5, batch_size=8)
            params.update(critic_actor=1)
            del params["batch_size"]
        monkeypatch.setenv("MOBODY_CONFIG_ROOT", root)
    return ["--policy", policy] + common, params


@pytest.mark.parametrize("policy", ("MOBODY", "TD3_BC", "IQL", "DARA", "IGDF", "BOSA"))
def test_cli_keys_evaluate_and_leave_training_alone(policy, tmp_path, monkeypatch):
    """12 steps at bs 8, eval_freq 4, fqe_steps 5 against the same run without the fqe_* keys: every net, moment, step count, buffer
    draw count and noise count bit for bit, torch's generators where they were; scalars.csv holds the four tags at steps 4, 8, 12."""
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo import utils
    argv, params = cli_args(policy, tmp_path, monkeypatch)
    made = []
    init = utils.ReplayBuffer.__init__
    monkeypatch.setattr(utils.ReplayBuffer, "__init__", lambda self, *a, **k: (init(self, *a, **k), made.append(self))[0])
    runs = {}
    for key in ("fqe", "plain"):
        del made[:]
        p = dict(params, **(dict(fqe_steps=5, fqe_batch_size=8, fqe_episodes=16) if key == "fqe" else {}))
        out_dir = tmp_path / key
        pol = tm.main(argv + ["--dir", str(out_dir), "--params", json.dumps(p)])
        torch.cuda.synchronize()
        state = snapshot(pol)
        for i, rb in enumerate(made):
            state.update({"buffer%d.%s" % (i, k): v for k, v in snapshot(rb).items()})
        state["torch.cpu_rng"], state["torch.cuda_rng"] = torch.get_rng_state(), torch.cuda.get_rng_state()
        csv = [f for d, _, fs in os.walk(out_dir) for f in (os.path.join(d, x) for x in fs) if f.endswith("scalars.csv")]
        rows = [ln.strip().split(",") for ln in open(csv[0])][1:]
        runs[key] = (state, {(r[0], int(r[1])): float(r[2]) for r in rows})
    (sa, ra), (sb, rb_) = runs["fqe"], runs["plain"]
    assert any(k.endswith("._draws") for k in sa) and len(sa) > 20
    bad = differing(sa, sb)
    assert bad == [], " ".join(bad)
    for tag in TAGS:
        assert [s for (t, s) in sorted(ra) if t == tag] == [4, 8, 12], tag
        assert all(np.isfinite(ra[(tag, s)]) for s in (4, 8, 12))
        assert not any(t == tag for (t, _) in rb_)
    assert {k: v for k, v in ra.items() if k[0] not in TAGS} == rb_, "every other scalar is what it was"
