"""CPU checks of what replays BOSA's critic / actor stage: the new entries are bound, exported and documented, refuse bad
blocks before any runtime call with the field named, report workspaces of their closed form; the fp64 restatement
(tests/bosa_graph_cases.py) evaluated in float32 on the GPU tests' exact inputs stays within HALF of the GPU tolerances, so those are
within reach of a correct fp32 implementation; the clamp tests' inputs cannot pass vacuously; and the class reads
config['critic_actor_graph'] only with config['critic_actor'].  No GPU compute is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bosa_graph_cases as GC
from test_abi import PTR, _refused
from test_bosa_ref import bosa_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mobody_bosa_target_workspace", "mobody_bosa_target", "mobody_bosa_stage2_rows", "mobody_bosa_stage2_words")


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
def test_new_entries_are_bound_exported_and_documented(lib):
    from mobody_amd import _lib
    hdr = header()
    assert lib.mobody_abi_version() == 7 and "#define MOBODY_ABI_VERSION 7" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", hdr, flags=re.S))
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, code), name + " is not declared"
        assert name in comments, name + " has no comment"
    for word in ("k_bosa_target_action", "k_bosa_qnext", "no flags, no tickets and no atomics", "every loop is bounded by an argument",
                 "LAUNCHES of a stage-2 call"):
        assert word in comments, word


def test_new_blocks_match_the_header_in_order(lib):
    from mobody_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in ("MobodyBosaTarget", "MobodyBosaStage2"):
        body = re.search(r"struct %s \{(.*?)\};" % name, code, flags=re.S).group(1)
        decls = [d for d in body.split(";") if d.strip()]
        fields = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", part).group(1) for d in decls for part in d.split(",")]
        cls = getattr(_lib, name)
        assert [f[0] for f in cls._fields_] == fields, name
        assert _lib.BLOCK_BYTES[cls] == C.sizeof(cls)
    assert C.sizeof(_lib.MobodyBosaTarget) == 4 * 4 + 8 + 6 * 8 + 2 * 4 + 8 + 4 * 4 + 2 * 8 == 120
    assert C.sizeof(_lib.MobodyBosaStage2) == 2 * 4 + 8 + 4 * 8 + 4 * 4 + 6 * 8 + 4 * 8 == 144


# ---- refusals: nothing here launches anything, the stream is NULL and every pointer is a made-up address ---------------------------
def target_block(_lib, **over):
    f = dict(precision=0, S=17, A=6, N=33, actor_blob=PTR, actor_blob_T=PTR, q_blob=PTR, q_blob_T=PTR, next_state=PTR, noise=PTR, seed=1, call=2,
             expl_noise=0.1, noise_clip=0.5, max_action=1.0, q_next=PTR, workspace=PTR)
    f.update(over)
    return _lib.block(_lib.MobodyBosaTarget, **f)


def test_target_refusals_name_the_field(lib):
    from mobody_amd import _lib
    e = "mobody_bosa_target"
    _refused(lib, e, _lib.MobodyBosaTarget(struct_bytes=C.sizeof(_lib.MobodyBosaTarget) - 1), "struct_bytes", "sizeof(MobodyBosaTarget) 120")
    for over, words in ((dict(S=0), ("S 0",)), (dict(S=257), ("S 257",)), (dict(A=0), ("A 0",)), (dict(A=129), ("A 129",)),
                        (dict(S=200, A=60), ("S + A = 260",)), (dict(N=0), ("N 0",)), (dict(N=2 ** 21 + 1), ("N 2097153", "2^21")),
                        (dict(precision=1), ("precision 1: must be one of 0 (f32), 3 (bf16x3), 4 (f16x2)",)),
                        (dict(precision=2), ("precision 2: must be one of 0 (f32), 3 (bf16x3), 4 (f16x2)",)),
                        (dict(precision=5), ("precision 5",)), (dict(precision=4, q_blob_T=None), ("T blobs",)),
                        (dict(precision=3, actor_blob_T=None), ("T blobs",)),
                        (dict(actor_blob=None), ("actor_blob is NULL",)), (dict(q_blob=None), ("q_blob is NULL",)),
                        (dict(next_state=None), ("next_state is NULL",)), (dict(q_next=None), ("q_next is NULL",)),
                        (dict(workspace=None), ("workspace is NULL",)), (dict(noise_clip=-0.5), ("noise_clip -0.5",)),
                        (dict(noise_clip=float("nan")), ("noise_clip",)), (dict(max_action=0.0), ("max_action 0",)),
                        (dict(max_action=-1.0), ("max_action -1",)), (dict(max_action=float("nan")), ("max_action",)),
                        (dict(expl_noise=float("nan")), ("expl_noise",))):
        _refused(lib, e, target_block(_lib, **over), *words)
    assert lib.mobody_bosa_target_workspace(C.byref(target_block(_lib, S=0))) == -1
    assert lib.mobody_bosa_target_workspace(C.byref(_lib.MobodyBosaTarget(struct_bytes=3, S=17, A=6, N=8))) == -1
    assert lib.mobody_bosa_target_workspace(None) == -1


def test_stage2_refusals_name_the_field(lib):
    from mobody_amd import _lib
    B = lambda **f: _lib.block(_lib.MobodyBosaStage2, **f)
    for e in ("mobody_bosa_stage2_rows", "mobody_bosa_stage2_words"):
        _refused(lib, e, _lib.MobodyBosaStage2(struct_bytes=C.sizeof(_lib.MobodyBosaStage2) + 8), "struct_bytes", "sizeof(MobodyBosaStage2) 144")
        _refused(lib, e, B(N=0, mask=PTR, row_weight=PTR, words=PTR, closs=PTR, mask_mean=PTR), "N 0")
        _refused(lib, e, B(N=2 ** 21 + 1, mask=PTR, row_weight=PTR, words=PTR, closs=PTR, mask_mean=PTR), "N 2097153", "2^21")
    e = "mobody_bosa_stage2_rows"
    _refused(lib, e, B(N=8), "neither mask nor dll")
    _refused(lib, e, B(N=8, mask=PTR), "row_weight is NULL")
    _refused(lib, e, B(N=8, dll=PTR, A=6), "dpi is NULL")
    _refused(lib, e, B(N=8, dll=PTR, dpi=PTR, A=0), "A 0")
    _refused(lib, e, B(N=8, dll=PTR, dpi=PTR, A=129), "A 129")
    _refused(lib, e, B(N=8, dll=PTR, dpi=PTR, A=6, dpi_scale=float("nan")), "dpi_scale")
    e = "mobody_bosa_stage2_words"
    _refused(lib, e, B(N=8, closs=PTR, mask_mean=PTR), "words is NULL")
    _refused(lib, e, B(N=8, words=PTR), "neither closs nor ll")
    _refused(lib, e, B(N=8, words=PTR, closs=PTR), "mask_mean is NULL")
    _refused(lib, e, B(N=8, words=PTR, ll=PTR), "aloss is NULL")
    _refused(lib, e, B(N=8, words=PTR, closs=PTR, mask_mean=PTR, nbump=5, bump=PTR), "nbump 5")
    _refused(lib, e, B(N=8, words=PTR, closs=PTR, mask_mean=PTR, nbump=-1, bump=PTR), "nbump -1")
    _refused(lib, e, B(N=8, words=PTR, closs=PTR, mask_mean=PTR, nbump=2), "bump is NULL")


# ---- workspaces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", GC.WS_SHAPES)
def test_target_workspace_closed_form(lib, S, A):
    from mobody_amd import _lib
    for N in GC.WORDS_ROWS:
        got = lib.mobody_bosa_target_workspace(C.byref(_lib.block(_lib.MobodyBosaTarget, S=S, A=A, N=N)))
        assert got == GC.target_workspace_floats(S, A, N) == (N * A + 3) // 4 * 4 + (2 * N + 3) // 4 * 4, (S, A, N)


# ---- the restatement in float32 stays within half of the GPU tolerances ------------------------------------------------------------
@pytest.mark.parametrize("N", GC.WORDS_ROWS)
def test_words_restatement_in_float32_is_within_half_the_tolerance(N):
    mask, closs, ll, aloss, _ = GC.words_inputs(N)
    w64, terms = GC.words(mask, closs, ll, aloss, GC.CONS, GC.LAMDA)
    w32, _ = GC.words(mask, closs, ll, aloss, GC.CONS, GC.LAMDA, np.float32)
    ratio = np.abs(w32.astype(np.float64) - w64) / GC.words_tolerance(w64, terms)
    print("N=%d words fp32 vs fp64, error / tolerance:" % N, np.round(ratio, 4))
    assert (ratio <= 0.5).all()
    assert w64[6] == -np.float64(ll[-1]) and np.argmax(-ll) == N - 1, "max(-ll) sits in the last row"
    # the copies are exact; mask_mean is a count below 2^24 divided once
    assert w32[0] == np.float32(w64[0]) and w32[1] == w64[1] and w32[3] == w64[3] and w32[7] == w64[7]
    nan = ll.copy()
    nan[N // 2] = np.nan
    wn, _ = GC.words(mask, closs, nan, aloss, GC.CONS, GC.LAMDA)
    assert np.isnan(wn[[4, 5, 6]]).all() and not np.isnan(wn[[0, 1, 2, 3, 7]]).any()


@pytest.mark.parametrize("S,A,N", [(17, 6, 257), (3, 1, 1025), (111, 8, 33)])
def test_target_value_restatement_in_float32_is_within_half_the_tolerance(S, A, N):
    """The GPU test holds mobody_bosa_target to the torch composition's BITS; next to that it holds q_next to the fp64 restatement at
    rtol 1e-5 / atol 1e-5 x max |q_next| (f32).  A float32 evaluation reaches half of that."""
    actor, critic = GC.mlp_params(5, S, A, 1), GC.mlp_params(6, S + A, 1, 2)
    s2, noise = GC.target_inputs(S, A, N)
    q64, a64 = GC.target_value(actor, critic, s2, noise, GC.EXPL, GC.CLIP, 1.0)
    q32, a32 = GC.target_value(actor, critic, s2, noise, GC.EXPL, GC.CLIP, 1.0, np.float32)
    tol = GC.RTOL * np.abs(q64) + GC.ATOL * np.abs(q64).max()
    ratio = float((np.abs(q32.astype(np.float64) - q64) / tol).max())
    print("(S, A, N) = (%d, %d, %d): q_next fp32 vs fp64, worst error / tolerance %.4f" % (S, A, N, ratio))
    assert ratio <= 0.5 and np.abs(a64).max() <= 1.0


@pytest.mark.parametrize("ma", (1.0, 2.0))
def test_clamp_edge_inputs_reach_every_branch(ma):
    """Each generated input has an element strictly inside, one beyond each noise clip and one beyond each action bound; and every
    value of the restatement is a float32, so that the GPU test can ask for equality."""
    A = 6
    noise, sign = GC.clamp_edge_inputs(A)
    pi = (sign * np.float32(ma))[:, None].repeat(A, 1)
    scaled = noise.astype(np.float64) * GC.EDGE_EXPL
    clip = np.float64(np.float32(GC.CLIP))
    assert (np.abs(scaled) < clip).any() and (scaled > clip).any() and (scaled < -clip).any() and (scaled == clip).any() and (scaled == -clip).any()
    moved = pi + np.clip(scaled, -clip, clip)
    assert (moved > ma).any() and (moved < -ma).any() and (np.abs(moved) < ma).any()
    a64 = GC.target_action(pi, noise, GC.EDGE_EXPL, GC.CLIP, ma)
    a32 = GC.target_action(pi, noise, GC.EDGE_EXPL, GC.CLIP, ma, np.float32)
    assert (a64.astype(np.float32).astype(np.float64) == a64).all() and (a32 == a64).all()
    assert (moved.astype(np.float32).astype(np.float64) == moved).all()
    just = noise[:, 0] == np.float32(GC.CLIP * (1 + 2.0 ** -20))
    assert just.sum() == 2 and (noise[just, 0] > np.float32(GC.CLIP)).all(), "clip (1 + 2^-20) is a float32 of its own"
    nanrow = GC.target_action(np.array([[np.nan, 0.5]]), np.array([[0.0, np.nan]]), 1.0, GC.CLIP, ma)
    assert np.isnan(nanrow).all(), "both clamps keep a NaN"


# ---- the key --------------------------------------------------------------------------------------------------------------------
def test_critic_actor_graph_is_read_with_critic_actor_only():
    """The constructor checks the key before it touches the device, so on the CPU an accepted config gets as far as the refusal of a
    CPU device and a refused one does not."""
    from mobody_amd.algo.offline_offline.bosa import BOSA
    gpu = "needs a GPU device"
    for value in (0, 1):
        with pytest.raises(RuntimeError, match=gpu):
            BOSA(bosa_config(critic_actor=1, critic_actor_graph=value), "cpu")
    with pytest.raises(RuntimeError, match=gpu):
        BOSA(bosa_config(critic_actor=1), "cpu")                                        # the default is 0
    for value in (2, -1, "1", True, 0.5, None):
        with pytest.raises(ValueError, match=r"config\['critic_actor_graph'\] = .*expected 0 .* or 1"):
            BOSA(bosa_config(critic_actor=1, critic_actor_graph=value), "cpu")
        with pytest.raises(RuntimeError, match=gpu):                                    # without critic_actor the key is not read
            BOSA(bosa_config(critic_actor_graph=value), "cpu")
