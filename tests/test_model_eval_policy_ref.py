"""Every policy in the learned model, the parts that need no GPU: the C ABI of `mobody_ens_evaluate_policy` and
`mobody_eval_summary` (declared, bound, exported, documented, every refusal before any runtime call, the workspace's closed
form), `evaluate_in_model` on the six algorithm classes, and the NumPy restatement of the summary's summation order against fp64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import model_eval_policy_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000          # a non-NULL pointer value: only compared with NULL before the refusal under test
ENTRY = "mobody_ens_evaluate_policy"
POINTERS = ("dyn_blob", "policy_blob", "init_obs", "elites", "obs_state", "alive", "ret", "pen_sum", "disc", "length", "member",
            "workspace")
SUMMARY_POINTERS = ("ret", "pen_sum", "length", "alive", "out", "nan_flag")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def _raw_header():
    return open(os.path.join(ROOT, "include", "mobody_hip.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw_header(), flags=re.S)


# ---- ABI contract --------------------------------------------------------------------------------------------------
def test_abi_declares_binds_and_exports_the_entry_points(lib):
    from mobody_amd import _lib
    hdr = re.sub(r"\s+", " ", _header())
    assert "int64_t mobody_ens_evaluate_policy_workspace(const MobodyEnsEvalPolicy* a);" in hdr
    assert "int mobody_ens_evaluate_policy(const MobodyEnsEvalPolicy* a, void* stream);" in hdr
    assert ("int mobody_eval_summary(const float* ret, const float* pen_sum, const int32_t* length, const uint8_t* alive, int64_t B, "
            "int G, float* out, int32_t* nan_flag, void* stream);") in hdr
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7
    P = C.POINTER(_lib.MobodyEnsEvalPolicy)
    assert _lib.PROTOTYPES["mobody_ens_evaluate_policy_workspace"] == (C.c_int64, [P])
    assert _lib.PROTOTYPES["mobody_ens_evaluate_policy"] == (C.c_int, [P, C.c_void_p])
    vp = C.c_void_p
    assert _lib.PROTOTYPES["mobody_eval_summary"] == (C.c_int, [vp, vp, vp, vp, C.c_int64, C.c_int, vp, vp, vp])
    for name in ("mobody_ens_evaluate_policy", "mobody_ens_evaluate_policy_workspace", "mobody_eval_summary"):
        assert hasattr(lib, name), name


def _fields(block):
    body = re.search(r"struct %s \{(.*?)\};" % block, _header(), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", part).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]


def test_block_fields_match_the_header_in_order_and_size():
    from mobody_amd import _lib
    names = _fields("MobodyEnsEvalPolicy")
    assert names == [f[0] for f in _lib.MobodyEnsEvalPolicy._fields_]
    # MobodyEnsEval's fields under the policy's names, the three new ones in front of the workspace
    old = [{"actor_blob": "policy_blob", "actor_blob_T": "policy_blob_T"}.get(n, n) for n in _fields("MobodyEnsEval")]
    assert names == old[:-1] + ["head", "member_mode", "member", "workspace"]
    assert [f[0] for f in _lib.MobodyEnsEval._fields_] == _fields("MobodyEnsEval")          # the old block keeps its layout
    assert C.sizeof(_lib.MobodyEnsEvalPolicy) == C.sizeof(_lib.MobodyEnsEval) + 8 + 8 == 208
    assert _lib.BLOCK_BYTES[_lib.MobodyEnsEvalPolicy] == 208
    assert _lib.MobodyEnsEvalPolicy.head.offset == 184 and _lib.MobodyEnsEvalPolicy.member.offset == 192


def test_header_comments_say_what_the_entries_do():
    hdr = re.sub(r"\s+", " ", _raw_header().replace("\n *", " "))
    for word in ("mobody_ens_evaluate_policy is mobody_ens_evaluate for both policy head forms", "max_action * tanh(mu)",
                 "member[b] = elites[b % n_elites]", "k_eval_init, then k_eval_members", "k_fqe_action",
                 "5 launches per step at head 0, 6 at head 1", "head outside {0, 1}, member_mode outside {0, 1}",
                 "2 A > 128 at head 1", "a null `member` in mode 1", "B == 0 returns 0",
                 "round4(B A) + round4(B S) + round4(B) + round4(7 B S + 7 B) + 2 round4(ceil(B / 4)) + (head 1: round4(2 B A))",
                 "Row b belongs to group b % G", "ONE workgroup of 256 threads and no atomics",
                 "Thread t adds rows t, t + 256, ... in ascending order", "a fixed tree joins the 256 partial results",
                 "summed as 64-bit integers and are exact", "An empty group", "G outside 1..7, B < 1, any null pointer"):
        assert word in hdr, word


# ---- refusals: MOBODY_E_ARG before any runtime call, pointers never dereferenced ------------------------------------
def _good(_lib, **over):
    """A block that passes every check (nothing may be launched with it: its pointers are fake)."""
    el = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    f = dict(struct_bytes=C.sizeof(_lib.MobodyEnsEvalPolicy), uncertainty_mode=0, precision=0, S=17, A=6, task=4, B=4, H=1,
             n_elites=5, elites=el, seed=1, call0=1, max_action=1.0, discount=1.0, use_trg=1, resume=0, head=1, member_mode=1)
    f.update({k: PTR for k in POINTERS if k != "elites"})
    f.update(over)
    return _lib.MobodyEnsEvalPolicy(**f)


def _refused(lib, blk, *words):
    assert lib.mobody_ens_evaluate_policy(C.byref(blk), None) == -1
    msg = lib.mobody_last_error().decode()
    assert msg.startswith(ENTRY + ":"), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


@pytest.mark.parametrize("over,words", [
    (dict(struct_bytes=8), ("struct_bytes", "sizeof(MobodyEnsEvalPolicy)")),
    (dict(struct_bytes=192), ("struct_bytes",)),                             # MobodyEnsEval's size
    (dict(head=2), ("head 2",)),
    (dict(head=-1), ("head",)),
    (dict(member_mode=2), ("member_mode 2",)),
    (dict(member_mode=-1), ("member_mode",)),
    (dict(A=65, S=17), ("A",)),                                              # 2 A = 130 > 128 (the layout refuses A > 64 by name too)
    (dict(B=-1), ("B < 0",)),
    (dict(H=-1), ("H < 0",)),
    (dict(uncertainty_mode=3), ("uncertainty_mode 3",)),
    (dict(resume=2), ("resume 2",)),
    (dict(discount=float("nan")), ("discount",)),
    (dict(discount=0.0), ("discount",)),
    (dict(discount=1.0000001), ("discount",)),
    (dict(precision=5), ("precision 5",)),
    (dict(precision=4), ("planes",)),
    (dict(precision=4, dyn_planes=PTR), ("policy_blob_T",)),
    (dict(precision=4, dyn_planes=PTR, policy_blob_T=PTR, mopo_blob=PTR), ("mopo_blob_T",)),
    (dict(n_elites=0), ("n_elites",)),
    (dict(n_elites=8), ("n_elites",)),
    (dict(task=7), ("task",)),
])
def test_refusals_name_the_field(lib, over, words):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **over), *words)


def test_the_gaussian_head_is_refused_by_its_own_rule(lib):
    """2 A > 128 at head 1 is the policy's rule, named with the head, before the model's layout sees A; head 0 is not held to it."""
    from mobody_amd import _lib
    assert "head 1" in _refused(lib, _good(_lib, A=65), "2 A")
    assert lib.mobody_ens_evaluate_policy(C.byref(_good(_lib, A=65, head=0)), None) == -1      # ... the model's layout refuses it
    assert lib.mobody_last_error().decode().startswith("mobody_dyn_layout:")


@pytest.mark.parametrize("field", POINTERS)
def test_every_null_pointer_is_refused_by_name(lib, field):
    from mobody_amd import _lib
    _refused(lib, _good(_lib, **{field: None}), "null pointer", field)


def test_refusal_edges_that_are_not_errors(lib):
    from mobody_amd import _lib
    none = {k: None for k in POINTERS}
    assert lib.mobody_ens_evaluate_policy(C.byref(_good(_lib, B=0, **none)), None) == 0
    # `member` is read in mode 1 only, init_obs only when resume == 0: null ones get past the pointer checks otherwise
    assert "member" not in _refused(lib, _good(_lib, member_mode=0, member=None, workspace=None), "workspace")
    assert "init_obs" not in _refused(lib, _good(_lib, resume=1, init_obs=None, workspace=None), "workspace")
    assert lib.mobody_ens_evaluate_policy(None, None) == -1 and lib.mobody_last_error().decode().startswith(ENTRY + ":")
    for bad in (dict(struct_bytes=8), dict(head=2), dict(B=-1)):
        assert lib.mobody_ens_evaluate_policy_workspace(C.byref(_good(_lib, **bad))) == -1
        assert lib.mobody_last_error().decode().startswith("mobody_ens_evaluate_policy_workspace:")


@pytest.mark.parametrize("B", [0, 1, 33, 257, 1025])
@pytest.mark.parametrize("S,A", [(17, 6), (111, 8), (17, 1), (17, 64)])
def test_workspace_closed_form(lib, S, A, B):
    from mobody_amd import _lib
    r4 = lambda n: (n + 3) // 4 * 4
    base = r4(B * A) + r4(B * S) + r4(B) + r4(7 * B * S + 7 * B) + 2 * r4((B + 3) // 4)
    old = _lib.MobodyEnsEval(struct_bytes=C.sizeof(_lib.MobodyEnsEval), S=S, A=A, B=B)
    assert lib.mobody_ens_evaluate_workspace(C.byref(old)) == base
    for head in (0, 1):
        blk = _lib.MobodyEnsEvalPolicy(struct_bytes=C.sizeof(_lib.MobodyEnsEvalPolicy), S=S, A=A, B=B, head=head)
        assert lib.mobody_ens_evaluate_policy_workspace(C.byref(blk)) == base + head * r4(2 * B * A)


def _summary(lib, **over):
    f = dict(ret=PTR, pen_sum=PTR, length=PTR, alive=PTR, B=4, G=5, out=PTR, nan_flag=PTR)
    f.update(over)
    rc = lib.mobody_eval_summary(f["ret"], f["pen_sum"], f["length"], f["alive"], f["B"], f["G"], f["out"], f["nan_flag"], None)
    return rc, lib.mobody_last_error().decode()


@pytest.mark.parametrize("over,word", [(dict(G=0), "G 0"), (dict(G=8), "G 8"), (dict(G=-1), "G"), (dict(B=0), "B 0"), (dict(B=-3), "B")]
                         + [({p: None}, p) for p in SUMMARY_POINTERS])
def test_summary_refusals_name_the_field(lib, over, word):
    rc, msg = _summary(lib, **over)
    assert rc == -1 and msg.startswith("mobody_eval_summary:") and word in msg, msg
    if None in over.values():
        assert "null pointer" in msg


# ---- the class method ------------------------------------------------------------------------------------------------
def test_evaluate_in_model_is_one_function_on_the_six_classes_and_raises_without_a_model():
    from mobody_amd.algo.offline_offline import bosa, dara, igdf, iql, mobody, td3_bc
    classes = [mobody.MOBODY, td3_bc.TD3BC, iql.IQL, dara.DARA, igdf.IGDF, bosa.BOSA]
    for cls in classes:
        assert cls.evaluate_in_model is mobody.evaluate_in_model, cls.__name__

    class Policy(object):
        dynamics = None
        evaluate_in_model = mobody.evaluate_in_model

    with pytest.raises(RuntimeError, match="Policy"):
        Policy().evaluate_in_model(np.zeros((1, 3), np.float32), 1)
    for cls in classes:                                    # each class names itself (no instance needs a device for that)
        obj = object.__new__(cls)
        obj.dynamics = None
        with pytest.raises(RuntimeError, match=cls.__name__):
            obj.evaluate_in_model(np.zeros((1, 3), np.float32), 1)


def test_cli_keys_are_off_by_default():
    from mobody_amd import train_mobody as tm
    argv = ["--policy", "TD3_BC", "--env", "walker2d-friction", "--shift_level", "2.0"]
    cfg = tm.build_config(tm.build_parser().parse_args(argv), 17, 6, 1.0)
    assert not {"model_eval_dynamics", "model_eval_members"} & set(cfg)
    assert not [a for a in tm.build_parser()._actions if "model_eval" in "".join(a.option_strings)]      # no new flag


# ---- the member rule ---------------------------------------------------------------------------------------------------
def test_member_rule():
    el = (0, 2, 3, 5, 6)
    assert pref.members(7, el).tolist() == [0, 2, 3, 5, 6, 0, 2]                   # B not a multiple of G
    assert pref.members(3, el).tolist() == [0, 2, 3]                               # B < G
    assert pref.members(10, el).reshape(2, 5).tolist() == [list(el)] * 2           # row b = episode b // G under member b % G
    assert pref.members(4, (4,)).tolist() == [4] * 4
    for B in (1, 2, 5, 7, 33, 257):
        for G in (1, 5, 7):
            counts = [pref.group_count(B, G, g) for g in range(G)]
            assert counts == np.bincount(np.arange(B) % G, minlength=G).tolist() and sum(counts) == B


# ---- the summary's summation order against fp64 ------------------------------------------------------------------------
def tables(B, seed=0):
    rng = np.random.default_rng(1000 * seed + B)
    ret = (rng.standard_normal(B) * 300.0 + 100.0).astype(np.float32)
    pen = (rng.random(B) * 40.0).astype(np.float32)
    length = rng.integers(1, 1001, B).astype(np.int32)
    alive = (rng.random(B) < 0.4).astype(np.uint8)
    return ret, pen, length, alive


@pytest.mark.parametrize("G", [1, 5, 7])
@pytest.mark.parametrize("B", [1, 2, 5, 255, 256, 257, 1025])
def test_summary_restatement_against_fp64(B, G):
    """The fp32 restatement stays within HALF of the derived bound (ceil(B / 256) + 9) 2^-24 sum|x| / count of each mean; the
    integer columns are the exact quotients rounded to fp32 once."""
    ret, pen, length, alive = tables(B)
    got, flag = pref.summary32(ret, pen, length, alive, G)
    want, mag, cnt = pref.summary64(ret, pen, length, alive, G)
    assert flag == 0 and cnt[G] == B and cnt[:G].sum() == B
    for row in range(G + 1):
        if cnt[row] == 0:
            assert row < G and B <= row and np.isnan(got[row]).all()
            continue
        for col, m in ((0, mag[row, 0]), (2, mag[row, 1])):
            err, bound = abs(float(got[row, col]) - want[row, col]), pref.mean_bound(B, m, cnt[row])
            assert err <= 0.5 * bound, (row, col, err, bound)
        assert got[row, 1] == np.float32(want[row, 1]) and got[row, 3] == np.float32(want[row, 3])
    if G == 1:
        assert np.array_equal(got[0], got[1])              # one group: its accumulators see the rows the overall ones see


def test_summary_restatement_order_and_nan():
    f = np.float32
    # the order is what the header says: thread 0 owns rows 0 and 256, thread 1 row 1.  1 + 2^-24 rounds to 1 in thread 0, and again
    # when the tree adds thread 1's 2^-24: the fp32 sum is 1, where a pairwise or fp64 sum keeps 2^-23
    ret = np.zeros(257, f)
    ret[0], ret[256], ret[1] = 1.0, 2.0 ** -24, 2.0 ** -24
    out, _ = pref.summary32(ret, np.zeros(257, f), np.ones(257, np.int32), np.ones(257, np.uint8), 1)
    assert out[1, 0] == f(f(1.0) + f(2.0 ** -24)) / f(257) == f(1.0) / f(257)        # (1 + 2^-24) rounds to 1, then + 2^-24 again
    # a NaN row: its group and the overall mean are NaN, the flag is raised, the other groups keep their bits
    ret, pen, length, alive = tables(257)
    clean, flag0 = pref.summary32(ret, pen, length, alive, 5)
    ret2 = ret.copy()
    ret2[7] = np.nan                                       # group 7 % 5 = 2
    dirty, flag1 = pref.summary32(ret2, pen, length, alive, 5)
    assert (flag0, flag1) == (0, 1) and np.isnan(dirty[2, 0]) and np.isnan(dirty[5, 0])
    keep = np.ones((6, 4), bool)
    keep[2, 0] = keep[5, 0] = False
    assert np.array_equal(clean.view(np.int32)[keep], dirty.view(np.int32)[keep])
    # B < G: the groups without rows are NaN and raise nothing
    out, flag = pref.summary32(ret[:3], pen[:3], length[:3], alive[:3], 7)
    assert flag == 0 and np.isnan(out[3:7]).all() and not np.isnan(out[:3]).any() and not np.isnan(out[7]).any()
