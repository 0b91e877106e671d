"""CPU checks of the wide-MLP layer: the layout query, packing round trips to the reference's VAE state_dict keys, the
header against the ctypes mirror, the refusals that come before any runtime call, and the fp64 restatement against finite differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import wide_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    from mobody_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        ge.build()
    return _lib.load()


BLOCKS = {"mobody_wide_mlp3_forward": "MobodyWideFwd", "mobody_wide_mlp3_backward": "MobodyWideBwd", "mobody_wide_adam": "MobodyWideAdam"}


def _fields(hdr, name):
    decl = re.search(r"\bstruct %s \{(.*?)\};" % name, hdr, flags=re.S).group(1)
    return [n.strip(" *") for stmt in decl.split(";") if stmt.strip()
            for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", stmt.strip()).split(",")]


def test_new_symbols_declared_bound_and_exported(lib):
    from mobody_amd import _lib, ops, packing
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    for e in BLOCKS:
        assert re.search(r"%s\s+(what loss\.backward\(\) does to such a stack \()?bosa\.py:\d+" % e, hdr) or \
            re.search(r"%s\s+torch\.optim\.Adam\(lr\) with torch's defaults \(bosa\.py:\d+" % e, hdr), e   # cites the lines it replaces
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for entry, blk in BLOCKS.items():
        assert re.search(r"\bint %s\(const %s\* a, void\* stream\);" % (entry, blk), hdr), entry
        res, args = _lib.PROTOTYPES[entry]
        cls = getattr(_lib, blk)
        assert res is C.c_int and args[0] is C.POINTER(cls) and args[1] is _lib.vp
        assert _fields(hdr, blk) == [f for f, _ in cls._fields_], blk
        assert C.sizeof(cls) == _lib.BLOCK_BYTES[cls]
        assert hasattr(lib, entry)
    lay = re.search(r"typedef struct MobodyWideLayout \{(.*?)\} MobodyWideLayout;", hdr, flags=re.S).group(1)
    names = [n.strip() for stmt in lay.split(";") if stmt.strip() for n in re.sub(r"^\s*\w+\s+", "", stmt.strip()).split(",")]
    assert names == [f for f, _ in _lib.MobodyWideLayout._fields_]
    assert C.sizeof(_lib.MobodyWideLayout) == 8 * 4 + 8 * 8
    for ws in ("mobody_wide_mlp3_forward_workspace", "mobody_wide_mlp3_backward_workspace"):
        assert re.search(r"\bint64_t %s\(const MobodyWideLayout\* L, int64_t rows\);" % ws, hdr) and hasattr(lib, ws)
    assert "#define MOBODY_ABI_VERSION 7" in hdr and lib.mobody_abi_version() == 7          # additions only: the version stays
    for f in ("wide_mlp3_forward", "wide_mlp3_backward", "wide_adam"):
        assert callable(getattr(ops, f)), f
    for f in ("pack_wide", "unpack_wide", "pack_bosa_vae_policy", "unpack_bosa_vae_policy", "pack_bosa_vae_dynamics",
              "unpack_bosa_vae_dynamics"):
        assert callable(getattr(packing, f)), f


@pytest.mark.parametrize("in_dim,hidden,out_dim,members", [(57, 750, 17, 5), (23, 8, 24, 1), (256, 1024, 256, 8), (4, 72, 2, 1), (16, 32, 32, 2)])
def test_layout(lib, in_dim, hidden, out_dim, members):
    from mobody_amd import _lib
    L = _lib.wide_layout(in_dim, hidden, out_dim, members)
    assert (L.in_dim, L.hidden, L.out_dim, L.members) == (in_dim, hidden, out_dim, members)
    assert L.Kp1 % 16 == 0 and L.Hp % 32 == 0 and L.Np3 % 32 == 0
    assert 0 <= L.Kp1 - in_dim < 16 and 0 <= L.Hp - hidden < 32 and 0 <= L.Np3 - out_dim < 32
    assert (L.w1, L.b1, L.w2, L.b2) == (0, L.Kp1 * L.Hp, L.Kp1 * L.Hp + L.Hp, L.Kp1 * L.Hp + L.Hp + L.Hp * L.Hp)
    assert L.w3 == L.b2 + L.Hp and L.b3 == L.w3 + L.Hp * L.Np3 and L.member_floats == L.b3 + L.Np3
    assert L.total_floats == members * L.member_floats
    rows = 129
    assert lib.mobody_wide_mlp3_forward_workspace(C.byref(L), rows) == members * rows * (L.Kp1 + 2 * L.Hp)
    assert lib.mobody_wide_mlp3_backward_workspace(C.byref(L), rows) == 2 * members * rows * L.Hp


@pytest.mark.parametrize("args,word", [((0, 72, 6, 1), "in_dim"), ((257, 72, 6, 1), "in_dim"), ((23, 7, 6, 1), "hidden"),
                                       ((23, 1025, 6, 1), "hidden"), ((23, 72, 0, 1), "out_dim"), ((23, 72, 257, 1), "out_dim"),
                                       ((23, 72, 6, 0), "members"), ((23, 72, 6, 9), "members")])
def test_layout_ranges(lib, args, word):
    from mobody_amd import _lib
    L = _lib.MobodyWideLayout()
    assert lib.mobody_wide_layout(*args, C.byref(L)) == -1
    assert word in lib.mobody_last_error().decode()


def _refused(lib, entry, blk, *words):
    assert getattr(lib, entry)(C.byref(blk), None) == -1, entry
    msg = lib.mobody_last_error().decode()
    assert msg.startswith((entry + ":", "mobody_wide_layout:")), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def test_refusals_come_before_any_runtime_call(lib):
    from mobody_amd import _lib
    L = _lib.wide_layout(23, 72, 24, 1)
    for entry, blk in BLOCKS.items():
        cls = getattr(_lib, blk)
        _refused(lib, entry, cls(struct_bytes=C.sizeof(cls) - 1), "struct_bytes", "sizeof(%s) %d" % (blk, C.sizeof(cls)))
    fwd = dict(layout=L, blob=PTR, src0=PTR, src_width0=23, x_shared=1, rows=8, out=PTR, workspace=PTR)
    for prec in (1, 2, 3, 4, -1):
        _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, precision=prec, **fwd), "precision %d" % prec, "exact fp32")
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "rows": 0}), "rows 0")
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "out_mode": 2}), "out_mode 2")
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "src_width0": 22}), "add up to 22", "in_dim is 23")
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "x_shared": 0}), "x_shared 0")
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "workspace": None}), "a null save needs the workspace")
    bad = _lib.wide_layout(23, 72, 24, 1)
    bad.Hp = 72
    _refused(lib, "mobody_wide_mlp3_forward", _lib.block(_lib.MobodyWideFwd, **{**fwd, "layout": bad}), "not mobody_wide_layout's")
    bwd = dict(layout=L, blob=PTR, dz3=PTR, x=PTR, h1=PTR, h2=PTR, x_shared=1, rows=8, grad=PTR, workspace=PTR)
    _refused(lib, "mobody_wide_mlp3_backward", _lib.block(_lib.MobodyWideBwd, precision=4, **bwd), "precision 4", "exact fp32")
    _refused(lib, "mobody_wide_mlp3_backward", _lib.block(_lib.MobodyWideBwd, **{**bwd, "grad": None}), "null pointer")
    _refused(lib, "mobody_wide_mlp3_backward", _lib.block(_lib.MobodyWideBwd, dx=PTR, dx_col0=17, dx_col1=24, **bwd), "dx columns [17, 24)")
    _refused(lib, "mobody_wide_mlp3_backward", _lib.block(_lib.MobodyWideBwd, dx=PTR, dx_col0=5, dx_col1=5, **bwd), "dx columns [5, 5)")
    adam = dict(blob=PTR, grad=PTR, m=PTR, v=PTR, n=10, lr=1e-3)
    _refused(lib, "mobody_wide_adam", _lib.block(_lib.MobodyWideAdam, **adam), "step t must be >= 1")
    _refused(lib, "mobody_wide_adam", _lib.block(_lib.MobodyWideAdam, t=1, **{**adam, "n": 0}), "n 0")
    _refused(lib, "mobody_wide_adam", _lib.block(_lib.MobodyWideAdam, t=1, **{**adam, "v": None}), "null pointer")


def test_pack_wide_round_trip_and_padding(lib):
    from mobody_amd import _lib, packing
    in_dim, hidden, out_dim, E = 57, 72, 17, 5
    p = WR.params(3, in_dim, hidden, out_dim, E)
    blob = packing.pack_wide(*(p[k] for k in WR.KEYS), "cpu")
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    assert blob.shape == (L.total_floats,)
    for k, t in zip(WR.KEYS, packing.unpack_wide(blob, in_dim, hidden, out_dim, E)):
        assert np.array_equal(t.numpy(), p[k]), k
    pad = packing.wide_padding_mask(in_dim, hidden, out_dim, E)
    n_real = E * (in_dim * hidden + hidden + hidden * hidden + hidden + hidden * out_dim + out_dim)
    assert int((~pad).sum()) == n_real and not blob[pad].any()
    # element (k, n) of member e's W1 sits at e * member_floats + w1 + k * Hp + n: row major, [in][out]
    assert blob[3 * L.member_floats + L.w1 + 5 * L.Hp + 7] == p["W1"][3, 5, 7]
    assert blob[2 * L.member_floats + L.w3 + 9 * L.Np3 + 4] == p["W3"][2, 9, 4]
    assert blob[4 * L.member_floats + L.b2 + 71] == p["b2"][4, 71]


def _policy_sd(S, A, H, seed):
    g = torch.Generator().manual_seed(seed)
    Lz = 2 * A
    shapes = {"encoder_shared.0": (H, S + A), "encoder_shared.2": (H, H), "mean": (Lz, H), "log_std": (Lz, H), "decoder.0": (H, S + Lz),
              "decoder.2": (H, H), "decoder.4": (A, H)}
    sd = {}
    for k, s in shapes.items():
        sd[k + ".weight"], sd[k + ".bias"] = torch.randn(*s, generator=g), torch.randn(s[0], generator=g)
    return sd


def _dynamics_sd(S, A, H, E, seed):
    g = torch.Generator().manual_seed(seed)
    Lz = 2 * S
    shapes = {"encoder_shared.0": (2 * S + A, H), "encoder_shared.2": (H, H), "mean": (H, Lz), "log_std": (H, Lz),
              "decoder.0": (S + A + Lz, H), "decoder.2": (H, H), "decoder.4": (H, S)}
    sd = {}
    for k, s in shapes.items():
        sd[k + ".W"], sd[k + ".b"] = torch.randn(E, *s, generator=g), torch.randn(E, 1, s[1], generator=g)
    return sd


@pytest.mark.parametrize("S,A,H", [(17, 6, 72), (3, 1, 8), (45, 24, 750)])
def test_policy_vae_state_dict_round_trip(lib, S, A, H):
    """VAE_Policy's keys (bosa.py:38-55): nn.Linear orientation; the two heads share the encoder's output layer, mean first."""
    from mobody_amd import _lib, packing
    sd = _policy_sd(S, A, H, 1)
    enc, dec = packing.pack_bosa_vae_policy(sd, "cpu")
    Le, Ld = _lib.wide_layout(S + A, H, 4 * A, 1), _lib.wide_layout(S + 2 * A, H, A, 1)
    assert enc.numel() == Le.total_floats and dec.numel() == Ld.total_floats
    back = packing.unpack_bosa_vae_policy(enc, dec, S, A, H)
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    assert enc[Le.w3 + 5 * Le.Np3 + 0] == sd["mean.weight"][0, 5] and enc[Le.w3 + 5 * Le.Np3 + 2 * A] == sd["log_std.weight"][0, 5]
    assert enc[Le.b3 + 2 * A + 1] == sd["log_std.bias"][1]


@pytest.mark.parametrize("S,A,H,E", [(17, 6, 72, 5), (3, 1, 8, 1), (45, 24, 72, 2)])
def test_dynamics_vae_state_dict_round_trip(lib, S, A, H, E):
    """VAE_Dynamics_Ensemble's keys (bosa.py:218-235): W [E, in, out], b [E, 1, out]."""
    from mobody_amd import _lib, packing
    sd = _dynamics_sd(S, A, H, E, 2)
    enc, dec = packing.pack_bosa_vae_dynamics(sd, "cpu")
    Le, Ld = _lib.wide_layout(2 * S + A, H, 4 * S, E), _lib.wide_layout(3 * S + A, H, S, E)
    assert enc.numel() == Le.total_floats and dec.numel() == Ld.total_floats
    back = packing.unpack_bosa_vae_dynamics(enc, dec, S, A, H, E)
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    e = E - 1
    assert enc[e * Le.member_floats + Le.w3 + 4 * Le.Np3 + 2 * S + 1] == sd["log_std.W"][e, 4, 1]


CORNER_IDS = ["h%d-r%d-e%d-%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1]) for c in WR.CORNER_CASES]


@pytest.mark.parametrize("case", WR.CORNER_CASES, ids=CORNER_IDS)
def test_backward_tolerance_is_reachable_in_fp32_at_the_corner_shapes(case):
    """The precondition of tests/test_hip_wide.py's backward tolerance (rtol 1e-5, atol 1e-5 x the tensor's largest entry), from
    the restatement alone: the same expressions evaluated in float32 NumPy stay within HALF of it of the fp64 ones, on the inputs
    the GPU test uses (its seeds; the activations are the fp64 forward's, rounded, in place of the kernel's saves).  So a correct
    fp32 kernel passes, and the tolerance is not so loose that it is met by accident of the shape: single-entry tensors (dx at
    in_dim = 1 with one row, b3 at out_dim = 1) are compared relative to themselves."""
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    p, srcs, x = WR.case_inputs(case)
    out, h1, h2 = WR.forward(p, x, mode, 1.7)
    assert (h1 > 0).any() and (h2 > 0).any()
    x32, h1, h2 = x.astype(np.float32), h1.astype(np.float32), h2.astype(np.float32)
    dz3 = np.random.default_rng(5).standard_normal((E, rows, out_dim)).astype(np.float32)
    g64, g32 = WR.backward(p, x32, h1, h2, dz3), WR.backward(p, x32, h1, h2, dz3, dtype=np.float32)
    for k in WR.KEYS + ("dx",):
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        tol = 1e-5 * np.abs(g64[k]).max() + 1e-5 * np.abs(g64[k])
        ratio = (np.abs(g32[k] - g64[k]) / tol).max()
        print("%s: fp32 evaluation error / tolerance %.3f" % (k, ratio))
        assert ratio <= 0.5, (k, ratio)


def test_corner_cases_cover_the_layout_domain(lib):
    """Every minimum and maximum of mobody_wide_layout's ranges, a shape with no padding in any dimension, every dimension both
    with and without padding, and row counts of exactly one 16-row chunk and one and two 64-row tiles."""
    from mobody_amd import _lib
    cs = WR.CORNER_CASES
    for idx, lo, hi in ((0, 8, 1024), (2, 1, 8)):
        assert {lo, hi} <= {c[idx] for c in cs}
    assert {1, 256} <= {c[3][0] for c in cs} and {1, 65, 256} <= {c[3][1] for c in cs}
    assert {1, 16, 64, 128} <= {c[1] for c in cs}
    pads = []
    for c in cs:
        L = _lib.wide_layout(c[3][0], c[0], c[3][1], c[2])
        pads.append((L.Kp1 - L.in_dim, L.Hp - L.hidden, L.Np3 - L.out_dim))
        assert sum(c[5]) == c[3][0]
    assert (0, 0, 0) in pads and all(any(p[d] for p in pads) and any(not p[d] for p in pads) for d in range(3))


def test_restatement_gradients_match_finite_differences():
    """The fp64 restatement's backward against central differences of its own forward (loss = sum(out * c))."""
    in_dim, hidden, out_dim, E, rows = 5, 8, 3, 2, 4
    p = WR.f64(WR.params(4, in_dim, hidden, out_dim, E))
    rng = np.random.default_rng(0)
    x, c = rng.standard_normal((E, rows, in_dim)), rng.standard_normal((E, rows, out_dim))
    loss = lambda q, xx: float((WR.forward(q, xx)[0] * c).sum())
    out, h1, h2 = WR.forward(p, x)
    g = WR.backward(p, x, h1, h2, c)
    h = 1e-6
    for k in WR.KEYS:
        for idx in [tuple(rng.integers(0, s) for s in p[k].shape) for _ in range(6)]:
            hi, lo = {kk: v.copy() for kk, v in p.items()}, {kk: v.copy() for kk, v in p.items()}
            hi[k][idx] += h
            lo[k][idx] -= h
            assert abs((loss(hi, x) - loss(lo, x)) / (2 * h) - g[k][idx]) < 1e-6 * max(1.0, abs(g[k][idx])), (k, idx)
    for idx in [tuple(rng.integers(0, s) for s in x.shape) for _ in range(6)]:
        hi, lo = x.copy(), x.copy()
        hi[idx] += h
        lo[idx] -= h
        assert abs((loss(p, hi) - loss(p, lo)) / (2 * h) - g["dx"][idx]) < 1e-6 * max(1.0, abs(g["dx"][idx])), idx
