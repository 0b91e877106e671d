"""CPU checks of fitted Q evaluation: the two entries are bound, exported and documented, refuse bad blocks before any
runtime call with the field named and report workspaces of their closed form; eval_policy() of the six algorithm classes; the NumPy
restatement (tests/fqe_ref.py) in float32 stays within HALF of the GPU tests' tolerances against itself in fp64, so those are within
reach of a correct fp32 implementation; and on constant rewards the fp64 restatement reaches 1 / (1 - gamma).  No GPU compute is
launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fqe_ref as R
from test_abi import PTR, _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mobody_fqe_target_workspace", "mobody_fqe_target", "mobody_fqe_value_workspace", "mobody_fqe_value")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def header():
    return open(os.path.join(ROOT, "include", "mobody_hip.h")).read()


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_entries_are_bound_exported_and_documented(lib):
    from mobody_amd import _lib
    hdr = header()
    assert lib.mobody_abi_version() == 7 and "#define MOBODY_ABI_VERSION 7" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", hdr, flags=re.S))
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert name in comments, name + " has no comment"
    for word in ("k_fqe_action", "k_fqe_qnext", "k_fqe_value", "The reference has no counterpart", "no flags, no tickets and no atomics",
                 "head 0 SKIPS it"):
        assert word in comments, word
    block = comments[comments.index("Fitted Q evaluation (DESIGN 5zb)"):]
    assert not re.search(r"\w+\.py:\d+", block), "the FQE block cites no reference lines"


def test_blocks_match_the_header_in_order(lib):
    from mobody_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ("MobodyFqeTarget", "MobodyFqeValue"):
        body = re.search(r"struct %s \{(.*?)\};" % name, code, flags=re.S).group(1)
        decls = [d for d in body.split(";") if d.strip()]
        fields = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", part).group(1) for d in decls for part in d.split(",")]
        cls = getattr(_lib, name)
        assert [f[0] for f in cls._fields_] == fields, name
        assert _lib.BLOCK_BYTES[cls] == C.sizeof(cls)
    assert C.sizeof(_lib.MobodyFqeTarget) == 6 * 4 + 8 + 5 * 8 + 2 * 4 + 3 * 8 == 104
    assert C.sizeof(_lib.MobodyFqeValue) == 6 * 4 + 8 + 5 * 8 + 2 * 4 + 4 * 8 == 112


# ---- refusals: nothing here launches anything, the stream is NULL and every pointer is a made-up address ---------------------------
def target_block(_lib, **over):
    f = dict(precision=0, head=0, S=17, A=6, N=33, policy_blob=PTR, policy_blob_T=PTR, q_blob=PTR, q_blob_T=PTR, next_state=PTR,
             max_action=1.0, q_next=PTR, workspace=PTR)
    f.update(over)
    return _lib.block(_lib.MobodyFqeTarget, **f)


def value_block(_lib, **over):
    f = dict(precision=0, head=0, S=17, A=6, B=33, policy_blob=PTR, policy_blob_T=PTR, q_blob=PTR, q_blob_T=PTR, state=PTR, max_action=1.0,
             out=PTR, nan_flag=PTR, workspace=PTR)
    f.update(over)
    return _lib.block(_lib.MobodyFqeValue, **f)


SHARED_REFUSALS = ((dict(head=2), ("head 2",)), (dict(head=-1), ("head -1",)), (dict(S=0), ("S 0",)), (dict(S=257), ("S 257",)),
                   (dict(A=0), ("A 0",)), (dict(A=129), ("A 129",)), (dict(head=1, A=65), ("A 65", "2 A", "128")), (dict(head=1, A=0), ("A 0",)),
                   (dict(S=200, A=60), ("S + A = 260",)),
                   (dict(precision=1), ("precision 1: must be one of 0 (f32), 3 (bf16x3), 4 (f16x2)",)),
                   (dict(precision=2), ("precision 2: must be one of 0 (f32), 3 (bf16x3), 4 (f16x2)",)),
                   (dict(precision=5), ("precision 5",)), (dict(precision=4, q_blob_T=None), ("T blobs",)),
                   (dict(precision=3, policy_blob_T=None), ("T blobs",)), (dict(policy_blob=None), ("policy_blob is NULL",)),
                   (dict(q_blob=None), ("q_blob is NULL",)), (dict(workspace=None), ("workspace is NULL",)),
                   (dict(max_action=0.0), ("max_action 0",)), (dict(max_action=-1.0), ("max_action -1",)),
                   (dict(max_action=float("nan")), ("max_action",)))


def test_target_refusals_name_the_field(lib):
    from mobody_amd import _lib
    e = "mobody_fqe_target"
    _refused(lib, e, _lib.MobodyFqeTarget(struct_bytes=C.sizeof(_lib.MobodyFqeTarget) - 1), "struct_bytes", "sizeof(MobodyFqeTarget) 104")
    own = ((dict(N=0), ("N 0",)), (dict(N=2 ** 21 + 1), ("N 2097153", "2^21")), (dict(next_state=None), ("next_state is NULL",)),
           (dict(q_next=None), ("q_next is NULL",)))
    for over, words in SHARED_REFUSALS + own:
        _refused(lib, e, target_block(_lib, **over), *words)
    assert lib.mobody_fqe_target(None, None) == -1
    assert lib.mobody_fqe_target_workspace(C.byref(target_block(_lib, S=0))) == -1
    assert lib.mobody_fqe_target_workspace(C.byref(target_block(_lib, head=2))) == -1
    assert lib.mobody_fqe_target_workspace(C.byref(_lib.MobodyFqeTarget(struct_bytes=3, S=17, A=6, N=8))) == -1
    assert lib.mobody_fqe_target_workspace(None) == -1


def test_value_refusals_name_the_field(lib):
    from mobody_amd import _lib
    e = "mobody_fqe_value"
    _refused(lib, e, _lib.MobodyFqeValue(struct_bytes=C.sizeof(_lib.MobodyFqeValue) + 8), "struct_bytes", "sizeof(MobodyFqeValue) 112")
    own = ((dict(B=0), ("B 0",)), (dict(B=2 ** 21 + 1), ("B 2097153", "2^21")), (dict(state=None), ("state is NULL",)),
           (dict(out=None), ("out is NULL",)), (dict(nan_flag=None), ("nan_flag is NULL",)))
    for over, words in SHARED_REFUSALS + own:
        _refused(lib, e, value_block(_lib, **over), *words)
    assert lib.mobody_fqe_value_workspace(C.byref(value_block(_lib, B=0))) == -1
    assert lib.mobody_fqe_value_workspace(None) == -1


# ---- workspaces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", R.HEADS)
def test_workspace_closed_forms(lib, head):
    from mobody_amd import _lib
    for S, A in R.TARGET_SHAPES + ((17, 64),) * head:
        for n in R.TARGET_ROWS + R.VALUE_ROWS:
            want = (n * A + 3) // 4 * 4 + (2 * n + 3) // 4 * 4 + head * ((2 * n * A + 3) // 4 * 4)
            assert R.workspace_floats(head, A, n) == want
            assert lib.mobody_fqe_target_workspace(C.byref(_lib.block(_lib.MobodyFqeTarget, head=head, S=S, A=A, N=n))) == want, (S, A, n)
            assert lib.mobody_fqe_value_workspace(C.byref(_lib.block(_lib.MobodyFqeValue, head=head, S=S, A=A, B=n))) == want, (S, A, n)


# ---- eval_policy ----------------------------------------------------------------------------------------------------------------
def test_eval_policy_of_the_six_classes():
    """(net, head): the deterministic actor with head 0 (MOBODY, TD3_BC: .policy; BOSA: .actor), the Gaussian policy with head 1
    (IQL, DARA, IGDF).  The method reads nothing else, so an object without a device serves."""
    from mobody_amd.algo.offline_offline.bosa import BOSA
    from mobody_amd.algo.offline_offline.dara import DARA
    from mobody_amd.algo.offline_offline.igdf import IGDF
    from mobody_amd.algo.offline_offline.iql import IQL
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    from mobody_amd.algo.offline_offline.td3_bc import TD3BC
    for cls, attr, head in ((MOBODY, "policy", 0), (TD3BC, "policy", 0), (BOSA, "actor", 0), (IQL, "policy", 1), (DARA, "policy", 1),
                            (IGDF, "policy", 1)):
        obj, net = cls.__new__(cls), object()
        setattr(obj, attr, net)
        got = obj.eval_policy()
        assert got[0] is net and got[1] == head and len(got) == 2, cls.__name__


def test_seed_ids_are_fqes_own():
    from mobody_amd import fqe
    from mobody_amd.algo.offline_offline import bosa
    assert (fqe.SEED_FQE_INDEX, fqe.SEED_FQE_INIT) == (111, 112) and R.SEED_FQE_INDEX == fqe.SEED_FQE_INDEX
    assert max(bosa.SEED_POLICY, bosa.SEED_DYNA, bosa.SEED_TARGET) < fqe.SEED_FQE_INDEX      # 101-107 index streams, 108-110 BOSA's


# ---- the restatement in float32 stays within half of the GPU tolerances ------------------------------------------------------------
def kernel_means(q):
    """k_fqe_value's summation in float32: thread t adds rows t, t + 256, ... in order, a tree joins the 256 partial sums."""
    f32 = np.float32
    B = q.shape[1]
    part = np.zeros((2, 256), f32)
    for i in range(B):
        part[:, i % 256] = (part[:, i % 256] + q[:, i]).astype(f32)
    h = 128
    while h >= 1:
        part[:, :h] = (part[:, :h] + part[:, h:2 * h]).astype(f32)
        h //= 2
    s0, s1 = part[0, 0], part[1, 0]
    return np.array([s0 / f32(B), s1 / f32(B), f32(s0 + s1) / f32(2 * B)], f32)


@pytest.mark.parametrize("B", R.VALUE_ROWS + (4099,))
def test_means_in_float32_are_within_half_the_tolerance(B):
    rng = np.random.default_rng(B)
    for offset in (0.0, 7.0):                                   # cancelling values, and values of one sign
        q = (offset + rng.standard_normal((2, B))).astype(np.float32)
        want = R.value_words(q)[:3]
        ratio = np.abs(kernel_means(q).astype(np.float64) - want) / R.mean_tolerance(q)
        print("B=%d offset %g: means fp32 vs fp64, error / tolerance:" % (B, offset), np.round(ratio, 4))
        assert (ratio <= 0.5).all()


def trajectory(dtype, head):
    from oracle import mobody_oracle as O
    from mobody_amd import fqe
    T = R.TRAJ
    data = R.dataset(T["rows"], T["S"], T["A"], T["seed"])
    q0 = R.params_from_state_dict({k: v.numpy() for k, v in fqe.initial_state_dict(T["S"], T["A"], T["seed"]).items()})
    f = R.Fqe(q0, R.policy_params(40 + head, head, T["S"], T["A"]), head, T["A"], 1.0, T["gamma"], T["tau"], T["lr"], dtype)
    for k in range(1, T["steps"] + 1):
        f.step(*[x[R.draw(O.rng_index, T["seed"], k, T["bs"], T["rows"])] for x in data])
    return f, f.value(data[0][::50])


@pytest.mark.parametrize("head", R.HEADS)
def test_trajectory_in_float32_is_within_half_the_tolerance(head):
    """The GPU trajectory test allows 4 x R.TRAJ_F32_DIFF; a float32 NumPy run of the same 20 steps stays within 2 x (measured where
    the constants were recorded: head 0 parameters 1.72e-6, target 1.59e-7, value words 4.9e-8; head 1 3.93e-7, 1.06e-7, 5.2e-8)."""
    (a, va), (b, vb) = trajectory(np.float64, head), trajectory(np.float32, head)
    got = dict(param=np.abs(a.flat() - b.flat()).max(), targ=np.abs(a.flat("q_targ") - b.flat("q_targ")).max(),
               value=np.abs(va - vb.astype(np.float64)).max())
    print("head %d, float32 vs fp64 after %d steps:" % (head, R.TRAJ["steps"]), got)
    for k, v in got.items():
        assert v <= 2 * R.TRAJ_F32_DIFF[head][k], (k, v)
    assert a.t == R.TRAJ["steps"] and np.isfinite(va).all()


def test_constant_rewards_reach_one_over_one_minus_gamma():
    """r = 1, not_done = 1, gamma 0.9: Q = 10 for every state and action.  R.CONST's lr 1e-3, tau 0.05, bs 32: the fp64 restatement is
    within 2 % after R.CONST['steps'] = 1000 steps (measured: 9.926, 0.74 %; 7.33 after 250, 9.26 after 500)."""
    from oracle import mobody_oracle as O
    from mobody_amd import fqe
    c = R.CONST
    data = R.dataset(c["rows"], c["S"], c["A"], c["seed"], const_reward=True)
    q0 = R.params_from_state_dict({k: v.numpy() for k, v in fqe.initial_state_dict(c["S"], c["A"], c["seed"]).items()})
    f = R.Fqe(q0, R.policy_params(41, 0, c["S"], c["A"]), 0, c["A"], 1.0, c["gamma"], c["tau"], c["lr"])
    for k in range(1, c["steps"] + 1):
        f.step(*[x[R.draw(O.rng_index, c["seed"], k, c["bs"], c["rows"])] for x in data])
    v = f.value(data[0][:64])
    print("constant rewards, fp64, %d steps: value words" % c["steps"], v)
    assert abs(v[2] - 10.0) <= 0.02 * 10.0
