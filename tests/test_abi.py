"""CPU-side checks of the C-ABI library: it builds, loads, exports every symbol the header declares,
and its layout / argument-validation entry points behave (no GPU compute is launched here)."""
import ctypes as C
import os
import re

import pytest

from dyn_shapes import SHAPES as DYN_SHAPE_EDGES      # the (S, A) edges of the layout, each with the edge it stands for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from mobody_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mobody_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 18
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mobody_abi_version() == 7


def test_struct_sizes_match_header(lib):
    from mobody_amd import _lib
    assert C.sizeof(_lib.MobodyLayer) == 32
    assert C.sizeof(_lib.MobodyDynLayout) == 16 + 13 * 32 + 8
    assert C.sizeof(_lib.MobodyMlpLayout) == 6 * 4 + 15 * 8
    assert C.sizeof(_lib.MobodyTrainDims) == 8 + 4 * 8
    assert C.sizeof(_lib.MobodyHyper) == 8 * 4


@pytest.mark.parametrize("S,A", [(17, 6), (111, 8), (45, 24), (11, 3)] + DYN_SHAPE_EDGES)
def test_dyn_layout(lib, S, A):
    from mobody_amd import _lib
    L = _lib.dyn_layout(S, A)
    assert (L.S, L.A, L.E) == (S, A, 7)
    end = 0
    for i, name in enumerate(_lib.DL_NAMES):
        l = L.layer[i]
        assert l.Kp % 8 == 0 and l.Np % 16 == 0 and l.Kp >= l.in_dim and l.Np >= l.out_dim, name
        assert l.w_off >= end and l.w_off % 4 == 0
        assert l.b_off == l.w_off + 7 * l.Kp * l.Np
        end = l.b_off + 7 * l.Np
    assert L.total_floats >= end
    assert L.layer[0].in_dim == S and L.layer[10].in_dim == 2 * S + A and L.layer[9].out_dim == S


def test_mlp_layout_counts_reference_parameters(lib):
    from mobody_amd import _lib
    L = _lib.mlp_layout(23, 1, 2)          # twin-Q at S=17, A=6: 144 386 parameters
    assert (L.Kp1, L.Np3, L.Np1t) == (24, 16, 32)
    assert 2 * (23 * 256 + 256 + 256 * 256 + 256 + 256 + 1) == 144386
    assert L.member_floats == 24 * 256 + 256 + 65536 + 256 + 256 * 16 + 16 and L.total_floats == 2 * L.member_floats
    La = _lib.mlp_layout(17, 6, 1)
    assert 17 * 256 + 256 + 65536 + 256 + 256 * 6 + 6 == 71942 and La.total_floats >= 71942


def test_argument_validation_reports_errors(lib):
    from mobody_amd import _lib
    L = _lib.MobodyDynLayout()
    assert lib.mobody_dyn_layout(1000, 6, C.byref(L)) == -1
    assert b"unsupported" in lib.mobody_last_error()
    assert lib.mobody_dyn_layout(120, 40, C.byref(L)) == -1      # 2S+A > 256
    # the bound on S that holds is 2S + A <= 256: S <= 127, and 127 only with A <= 2; the message says so
    for S, A in ((1, 1), (127, 3), (128, 1), (17, 65), (17, 0)):
        assert lib.mobody_dyn_layout(S, A, C.byref(L)) == -1, (S, A)
        msg = lib.mobody_last_error().decode()
        assert msg.startswith("mobody_dyn_layout: unsupported S=%d A=%d" % (S, A)) and "256" in msg, msg
    assert "[2,127]" in msg and "240" not in msg
    for S, A in ((127, 2), (96, 64)):
        assert lib.mobody_dyn_layout(S, A, C.byref(L)) == 0 and (L.S, L.A, L.layer[10].Kp) == (S, A, 256)
    M = _lib.MobodyMlpLayout()
    assert lib.mobody_mlp_layout(300, 1, 1, C.byref(M)) == -1
    d = _lib.MobodyTrainDims(17, 6, 0, 0, 0, 0)
    assert lib.mobody_train_workspace(C.byref(d)) == -1
    d = _lib.MobodyTrainDims(17, 6, 640, 512, 640, 512)
    assert lib.mobody_train_workspace(C.byref(d)) > 640 * 256 * 8
    # empty batches are accepted without touching any pointer
    assert lib.mobody_dyn_step(None, None, 0, 17, 6, 4, None, None, 0, None, None, None, None, 0, 0, 0, None, 0.0, 1, 1, None, None,
                               None, None, None, None, None, None) == 0
    assert lib.mobody_dyn_step(None, None, 0, 17, 6, 99, None, None, 5, None, None, None, None, 0, 0, 0, None, 0.0, 1, 1, None, None,
                               None, None, None, None, None, None) == -1


# ---- argument blocks: every entry point that takes one (nothing here launches anything: the refusals come first) ----
BLOCK_ENTRIES = [("mobody_critic", "MobodyCritic"), ("mobody_actor_forward", "MobodyActor"), ("mobody_actor_backward", "MobodyActor"),
                 ("mobody_adam_polyak", "MobodyAdam"), ("mobody_pretrain", "MobodyPretrain"),
                 ("mobody_pretrain_mopo", "MobodyPretrainMopo")]
PTR = 0x1000        # a non-NULL pointer value for fields that are only compared with NULL before the refusal under test


def _header_structs():
    """{struct name: field names in declaration order} of include/mobody_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", hdr, flags=re.S):
        decls = [d for d in body.split(";") if d.strip()]
        out[name] = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", part).group(1) for d in decls for part in d.split(",")]
    return out


def _refused(lib, entry, blk, *words):
    assert getattr(lib, entry)(C.byref(blk), None) == -1, entry          # MOBODY_E_ARG
    msg = lib.mobody_last_error().decode()
    assert msg.startswith((entry + ":", "mobody_mlp_layout:", "mobody_pretrain_layout:", "mobody_pretrain_mopo_layout:")), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def test_block_fields_match_header_in_order(lib):
    from mobody_amd import _lib
    structs = _header_structs()
    blocks = [n for n, f in structs.items() if f[0] == "struct_bytes"]
    assert sorted(blocks) == sorted({b for _, b in BLOCK_ENTRIES} | {"MobodyEnsStep", "MobodyEnsRollout"})
    for n in blocks:
        assert [f[0] for f in getattr(_lib, n)._fields_] == structs[n], n


@pytest.mark.parametrize("entry,block", BLOCK_ENTRIES)
def test_block_struct_bytes_is_checked_first(lib, entry, block):
    from mobody_amd import _lib
    cls = getattr(_lib, block)
    _refused(lib, entry, cls(struct_bytes=C.sizeof(cls) - 1), "struct_bytes", "sizeof(%s) %d" % (block, C.sizeof(cls)))
    # the right size and nothing else: refused further on, so ctypes and the library agree on sizeof
    assert "struct_bytes" not in _refused(lib, entry, _lib.block(cls))


def _choice_blocks(_lib):
    """(entry, block valid up to the choice between gradient blob and optimizer state, name of the gradient field)."""
    d, h = _lib.MobodyTrainDims(17, 6, 64, 32, 64, 32), _lib.MobodyHyper(0.99, 0.005, 1.0, 2.5, 0.1, 1, 1, 0)
    pre = dict(S=17, A=6, b=8, b_global=8)
    return [("mobody_critic", _lib.block(_lib.MobodyCritic, d=d, h=h), "grad_q"),
            ("mobody_actor_backward", _lib.block(_lib.MobodyActor, d=d, h=h), "grad_actor"),
            ("mobody_pretrain", _lib.block(_lib.MobodyPretrain, **pre), "grad"),
            ("mobody_pretrain_mopo", _lib.block(_lib.MobodyPretrainMopo, **pre), "grad")]


def test_block_needs_exactly_one_of_gradient_and_optimizer_state(lib):
    from mobody_amd import _lib
    for entry, blk, g in _choice_blocks(_lib):
        _refused(lib, entry, blk, "exactly one of " + g)                  # neither
        setattr(blk, g, PTR)
        blk.m = blk.v = PTR
        _refused(lib, entry, blk, "exactly one of " + g)                  # both
        blk.v = None
        _refused(lib, entry, blk, "exactly one of " + g)                  # the gradient and half the state
        setattr(blk, g, None)
        _refused(lib, entry, blk, "null pointer")                          # half the state alone
        blk.v = PTR
        assert "exactly one" not in _refused(lib, entry, blk)             # the fused choice is made: refused further on


def test_critic_gather_refusals(lib):
    from mobody_amd import _lib
    gr = _lib.MobodyGatherRng()
    fused = dict(d=_lib.MobodyTrainDims(17, 6, 64, 32, 64, 32), m=PTR, v=PTR, t=1, gather=C.pointer(gr))
    _refused(lib, "mobody_critic", _lib.block(_lib.MobodyCritic, phase=1, **fused),
             "the step cannot be split (phase 1): the first forward launch writes the minibatch the backward reads")
    _refused(lib, "mobody_critic", _lib.block(_lib.MobodyCritic, q_next=PTR, **fused),
             "q_next given: the launch that gathers is the one that evaluates pi(s')")
    _refused(lib, "mobody_critic", _lib.block(_lib.MobodyCritic, phase=3, **{**fused, "gather": None}), "phase is 0")


def test_pretrain_fused_form_refuses_b_global(lib):
    from mobody_amd import _lib
    for entry, cls in (("mobody_pretrain", _lib.MobodyPretrain), ("mobody_pretrain_mopo", _lib.MobodyPretrainMopo)):
        _refused(lib, entry, _lib.block(cls, S=17, A=6, b=8, b_global=16, m=PTR, v=PTR), "b_global 16 != b 8")
        assert "b_global 16" not in _refused(lib, entry, _lib.block(cls, S=17, A=6, b=8, b_global=16, grad=PTR))


def test_missing_library_fails_loudly(monkeypatch, lib):
    from mobody_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libmobody_hip.so")
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()
