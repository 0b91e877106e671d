"""mobody_mlp3_backward in isolation: the fp32 forms of k_mlp3_bwd, k_wgrad and k_grad_reduce with no loss kernel in front
(the V function of the `advantage` variant and both DARA classifiers get their gradients from this entry).

(a) Exact.  Small-integer x / h1 / h2 / dz3 and sparse {-1, 0, 1} weights: every partial sum of every output is an integer
    below 2^24, every fp32 summation order gives the same bits, and the kernels must equal the integer reference bit for
    bit at every row geometry of the split-K row loop.  The precondition is asserted from the reference alone.

(b) Real-valued inputs against fp64, per element, nothing normalised by a tensor's maximum (as tests/f64_bounds.py).
    With u = 2^-24 and the fp64 sums of absolute values S(.) = sum |a| |b| of tests/aux_ref.py:

      dz2 = (dz3 W3) [h2 > 0]   one GEMM over K = Np3 <= 112 in K = 2 MFMA steps: at most 56 dependent adds, inside
                                C_LAYER = 128 u (f64_bounds).                      E2 = C_LAYER S(dz2)
      dz1 = (dz2 W2) [h1 > 0]   K = 256, 128 steps, plus dz2's error to first order:  E1 = (C_LAYER S(dz1) + E2 |W2|) [h1 > 0]
      dW  = sum_rows a b        a product passes through: the MFMA chain of its wave's row slice, rows_per_wave adds
                                (v_mfma_f32_32x32x2f32 adds two rows per step); 2 adds of the LDS reduction (waves 2, 3 onto
                                0, 1, then the two buffers); nsplit adds of k_grad_reduce's slab sum; 1 for the product.
                                n_w = rows_per_wave + nsplit + 3:   |dW3 err| <= n_w u S(dW3),
                                |dW2 err| <= n_w u S(dW2) + E2^T |h1|,   |dW1 err| <= n_w u S(dW1) + E1^T |x|
      db  = sum_rows dz         32 rows of a tile (16 per lane + one shuffle for db1 / db2, 32 serial for db3), then
                                k_grad_reduce: ceil(tiles / 64) strided adds per lane + 6 shuffle adds.
                                n_b = 32 + ceil(tiles / 64) + 6:    |db err| <= n_b u S(db) + sum_rows E
    The masks are functions of the h1 / h2 the test supplies, so there is no ReLU-kink ambiguity.  The bounds are worst
    case and take no margin; the measured worst err / bound per tensor and geometry is kept in profiles/aux_grad_bounds.json
    (set MOBODY_AUX_BOUNDS_JSON=<path> to rewrite it).  Random rounding errors grow like sqrt(n), so ratios of a few
    percent are what a correct kernel shows; a dropped row block or slab is an error of order S itself, ratio >> 1.

Padding of the gradient blob (rows k >= in_dim of W1, columns >= out_dim of W3 / b3): k_grad_reduce writes EVERY entry of
the blob; a padding entry is the same contraction as its neighbours over the zero padding of x / dz3, so it is exactly 0
whenever the caller's padding is 0 (what mlp3_forward's saved x and the loss kernels' dz3 provide).  Asserted below with a
NaN sentinel in the gradient blob and the workspace before every call.
"""
import json
import os

import numpy as np
import pytest
import torch

import aux_ref as R
import f64_bounds as FB
import golden_util as gu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SA = [(3, 1), (17, 6), (45, 24), (111, 8)]
KINDS = {  # (in_dim, out_dim, members) of the real nets
    "v": lambda S, A: (S, 1, 1), "cls_sa": lambda S, A: (S + A, 2, 1), "cls_sas": lambda S, A: (2 * S + A, 2, 1),
    "actor": lambda S, A: (S, A, 1), "twin_q": lambda S, A: (S + A, 1, 2), "mopo": lambda S, A: (S + A, S, 7)}
DIMS1 = [(k, sa) for sa in SA for k in ("v", "cls_sa", "cls_sas", "actor")]
DIMS2 = [("twin_q", sa) for sa in SA]
DIMS7 = [("mopo", sa) for sa in SA]

# rows -> the branch of wgrad_tile's row loop (aux_ref.wgrad_geometry names) this count is there for
ROWS1 = [
    (1, "tail_only"),            # one wave with a single row: only the masked pass; three empty waves
    (7, "tail_only"),            # the longest tail-only slice
    (8, "one_block"),            # one whole block, no tail: the `nblk & 1` pass alone
    (9, "one_block_tail"),       # one block + 1-row tail
    (15, "one_block_tail"),      # one block + 7-row tail
    (16, "nblk_even"),           # two blocks: the pipeline runs once and re-loads block 1 unused
    (17, "one_row_wave"),        # wave 0 full (16), wave 1 one row
    (31, "blocks_and_tail"),     # bias tile 1 row short; wave 1 = 8 + 7
    (32, "nblk_even"),           # exactly one bias tile
    (33, "bias_tile_ragged"),    # second bias tile of 1 row; wave 2 one row
    (63, "blocks_and_tail"),     # all four waves busy, the last 8 + 7
    (64, "nblk_even"),           # four full 16-row slices
    (65, "empty_wave"),          # rows_per_wave 17 -> 32: wave 2 has one row, wave 3 none
    (127, "nsplit=1"), (128, "nsplit=1"), (129, "nsplit=1"),      # rows / 128 = 1 still one slab
    (255, "nsplit=1"), (256, "nsplit=2"), (257, "nsplit=2"),      # first slab sum of k_grad_reduce
    (280, "nblk_odd@split"),     # nsplit 2, rows_per_wave 48: wave 5 has 40 rows = 5 blocks (tail pass after the pipeline)
    (283, "nblk_odd@split"),     # same with a 3-row masked tail behind it
    (383, "nsplit=2"), (384, "nsplit=3"), (385, "nsplit=3"),      # odd slab count: the scalar remainder loop of the slab sum
    (512, "nblk_even@split"),    # nsplit 4: one 4-slab group of the unrolled sum, 32-row slices
    (4095, "nsplit=31"), (4096, "nsplit_cap"),                     # 31 -> 32 slabs
    (4097, "empty_slice"),       # cap 32, rows_per_wave 33 -> 48: 86 of 128 waves have work, slices 22..31 are empty
    (10240, "nsplit_cap"),       # the V update's 2.5 * bs rows: 80-row slices
]
ROWS2 = [(33, "nsplit=1"), (511, "nsplit=1"), (512, "nsplit=2"), (513, "nsplit=2"), (767, "nsplit=2"), (768, "nsplit=3"),
         (4095, "nsplit=15"), (4096, "nsplit_cap"), (4097, "empty_slice"), (10240, "nsplit_cap")]      # twin net: 256-row steps, cap 16
ROWS7 = [(65, "empty_wave"), (1023, "nsplit=3"), (1024, "nsplit_cap"), (1025, "empty_wave"), (1280, "nsplit_cap"),
         (10240, "nsplit_cap")]      # 7 members: cap 4 (1025: rows_per_wave 65 -> 80, waves 13..15 empty; no slice is ever wholly empty at cap 4)
# every dim also gets a ragged, an aligned (rows % (64 nsplit) == 0) and a capped-nsplit row count
MUST = {1: (33, 256, 4096), 2: (513, 512, 4096), 7: (1025, 1024, 1280)}


def _cases():
    out = []
    for members, rows_list, dims in ((1, ROWS1, DIMS1), (2, ROWS2, DIMS2), (7, ROWS7, DIMS7)):
        for i, (rows, branch) in enumerate(rows_list):
            for d in {(2 * i) % len(dims), (2 * i + 1) % len(dims)}:         # every row count with two dims
                out.append((dims[d][0], dims[d][1], rows, branch))
        for kind, sa in dims:
            for rows in MUST[members]:
                if not any(c[0] == kind and c[1] == sa and c[2] == rows for c in out):
                    out.append((kind, sa, rows, dict(rows_list)[rows]))
    return out


CASES = _cases()


def case_id(c):
    return f"{c[0]}-S{c[1][0]}A{c[1][1]}-rows{c[2]}-{c[3]}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_AUX_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst |got - fp64| / bound per tensor, tests/test_hip_aux_grad.py part (b)", "cases": RATIOS},
                      f, indent=1, sort_keys=True)


def run_backward(c, in_dim, out_dim, members, dev):
    """pack -> mlp_transpose -> NaN sentinels -> mlp3_backward.  Returns (per-member gradient dicts, dz2, dz1) as numpy and
    asserts what the code promises of the whole blob: every entry written, padding entries exactly 0."""
    from mobody_amd import _lib, ops, packing
    rows = c["x"].shape[0]
    L = _lib.mlp_layout(in_dim, out_dim, members)
    zb = lambda n: np.zeros(n, np.float32)
    blob = packing.pack_mlp([{"network.0.weight": c["W1"][m], "network.0.bias": zb(256), "network.2.weight": c["W2"][m],
                              "network.2.bias": zb(256), "network.4.weight": c["W3"][m], "network.4.bias": zb(out_dim)}
                             for m in range(members)], in_dim, out_dim, dev)
    blob_T = ops.mlp_transpose(blob, in_dim, out_dim, members, precision=0)
    x = torch.zeros(rows, L.Kp1, device=dev); x[:, :in_dim] = torch.from_numpy(c["x"]).to(dev)
    dz3 = torch.zeros(members, rows, L.Np3, device=dev); dz3[:, :, :out_dim] = torch.from_numpy(c["dz3"]).to(dev)
    h1, h2 = torch.from_numpy(c["h1"]).to(dev), torch.from_numpy(c["h2"]).to(dev)
    grad = torch.full((L.total_floats,), float("nan"), device=dev)
    need = _lib.load().mobody_mlp3_backward_workspace(in_dim, out_dim, members, rows)
    ws = torch.full((need,), float("nan"), device=dev)
    got_ws = ops.mlp3_backward(blob_T, in_dim, out_dim, members, dz3, x, h1, h2, grad, ws)
    assert got_ws is ws
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad).all()), f"{int((~torch.isfinite(grad)).sum())} entries of the gradient blob unwritten / non-finite"
    for m in range(members):
        base = m * L.member_floats
        w1 = packing.wide_unpack(grad[base + L.w1:base + L.w1 + L.Kp1 * 256], L.Kp1)
        w3 = grad[base + L.w3:base + L.w3 + 256 * L.Np3].view(256, L.Np3)
        b3 = grad[base + L.b3:base + L.b3 + L.Np3]
        assert bool((w1[in_dim:] == 0).all()), "dW1 padding rows k >= in_dim are not exactly 0"
        assert bool((w3[:, out_dim:] == 0).all()) and bool((b3[out_dim:] == 0).all()), "dW3 / db3 padding columns are not exactly 0"
    g = [{k: v.cpu().numpy() for k, v in d.items()} for d in packing.unpack_mlp(grad, in_dim, out_dim, members)]
    n = members * rows * 256                            # carve_bwd (csrc/dara.hip): dz2 | dz1 | dbp | slabs
    dz2 = ws[:n].view(members, rows, 256).cpu().numpy()
    dz1 = ws[n:2 * n].view(members, rows, 256).cpu().numpy()
    return g, dz2, dz1


def same_bits(got, want, what):
    """Bit equality of fp32 `got` with the integer-valued fp64 `want` (a zero's sign is not a bit of the sum: +0 + -0)."""
    got = np.asarray(got, np.float32) + np.float32(0)
    want = np.asarray(want, np.float64).astype(np.float32) + np.float32(0)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first {i}: got {got[i]!r} want {want[i]!r}")


def check_case_table():
    """(Also run without a GPU by tests/test_aux_ref.py.)  Every row count hits the branch its comment names (from the formulas of train.h / launch_wgrad), with two dims;
    every dim has a ragged, an aligned and a capped-nsplit row count; the named branches are all there."""
    seen = set()
    per_rows, per_dim = {}, {}
    for kind, sa, rows, branch in CASES:
        members = KINDS[kind](*sa)[2]
        geo = R.wgrad_geometry(rows, members)
        assert branch in geo["branches"], (kind, sa, rows, branch, sorted(geo["branches"]))
        seen |= geo["branches"]
        per_rows.setdefault((members, rows), set()).add((kind, sa))
        f = per_dim.setdefault((kind, sa), set())
        f.add("ragged" if rows % 32 else "whole_tiles")
        if rows % (64 * geo["nsplit"]) == 0:
            f.add("aligned")
        if "nsplit_cap" in geo["branches"]:
            f.add("capped")
    assert all(len(v) >= 2 for v in per_rows.values()), {k: v for k, v in per_rows.items() if len(v) < 2}
    assert len(per_dim) == 24 and all({"ragged", "aligned", "capped"} <= f for f in per_dim.values()), per_dim
    for b in ("tail_only", "one_block", "one_block_tail", "blocks_and_tail", "pipeline", "nblk_even", "nblk_odd",
              "nblk_even@split", "nblk_odd@split", "empty_wave", "empty_slice", "one_row_wave", "rpw_rounded",
              "nsplit=1", "nsplit=2", "nsplit=3", "nsplit_cap", "bias_tile_ragged"):
        assert b in seen, b
    for members, cap, rows in ((1, 32, 4096), (2, 16, 4096), (7, 4, 1280)):
        assert R.wgrad_nsplit(rows, members) == cap


def test_case_table_covers_what_it_claims():
    check_case_table()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_integer_gradients(case, dev):
    kind, (S, A), rows, branch = case
    in_dim, out_dim, members = KINDS[kind](S, A)
    assert branch in R.wgrad_geometry(rows, members)["branches"]
    c = R.int_case(1000 + rows + 7 * in_dim, in_dim, out_dim, members, rows)
    ref = R.mlp3_backward_ref(c["W1"], c["W2"], c["W3"], c["x"], c["h1"], c["h2"], c["dz3"])
    worst, ok = R.int_exact_ok(ref)
    assert ok, f"precondition of bit equality fails: max sum |a||b| = {worst} (needs < 2^24, integers)"
    assert (c["h1"] <= 0).any() and (c["h2"] <= 0).any() and np.abs(ref["dz1"]).max() > 0
    g, dz2, dz1 = run_backward(c, in_dim, out_dim, members, dev)
    same_bits(dz2, ref["dz2"], "dz2")
    same_bits(dz1, ref["dz1"], "dz1")
    for m in range(members):
        for rk, pk in R.GRAD_KEYS:
            same_bits(g[m][pk], ref[rk][m], f"{rk}[member {m}] rows={rows}")


def real_case(seed, kind, S, A, rows, mix):
    """gen_inputs' parameters and batch; h1 / h2 are the fp32 forward activations of that net.  mix: "plain", "row_scale"
    (every row of x, h1, h2 times 2^k, k uniform in [-20, 20]), "dominant" (one row of dz3 2^12 above the rest)."""
    in_dim, out_dim, members = KINDS[kind](S, A)
    s, a, s2, _, _ = gu.gi.batch(seed, rows, S, A)
    x = {"v": s, "actor": s, "cls_sas": np.concatenate([s, a, s2], 1)}.get(kind)
    if x is None:
        x = np.concatenate([s, a], 1)
    rng = np.random.default_rng(seed + 1)
    P = [gu.gi.mlp_params(seed + 10 + m, in_dim, out_dim) for m in range(members)]
    W1, W2, W3 = (np.stack([p[f"network.{l}.weight"] for p in P]) for l in (0, 2, 4))
    h1 = np.stack([np.maximum(x @ p["network.0.weight"].T + p["network.0.bias"], 0) for p in P]).astype(np.float32)
    h2 = np.stack([np.maximum(h1[m] @ p["network.2.weight"].T + p["network.2.bias"], 0) for m, p in enumerate(P)]).astype(np.float32)
    dz3 = (rng.standard_normal((members, rows, out_dim)) / rows).astype(np.float32)
    if mix == "row_scale":
        sc = np.exp2(rng.integers(-20, 21, rows)).astype(np.float32)[:, None]
        x, h1, h2 = x * sc, h1 * sc, h2 * sc
    elif mix == "dominant":
        dz3[:, rows // 3] *= np.float32(2.0 ** 12)
    return {"W1": W1, "W2": W2, "W3": W3, "x": x.astype(np.float32), "h1": h1, "h2": h2, "dz3": dz3}


REAL = [("v", (17, 6), 10240), ("twin_q", (17, 6), 10240), ("cls_sas", (45, 24), 257), ("cls_sa", (111, 8), 65),
        ("actor", (111, 8), 385), ("twin_q", (45, 24), 4097), ("mopo", (3, 1), 1025), ("actor", (17, 6), 283)]


@pytest.mark.parametrize("mix", ["plain", "row_scale", "dominant"])
@pytest.mark.parametrize("kind,sa,rows", REAL, ids=lambda v: str(v).replace(" ", ""))
def test_gradients_vs_fp64_bounds(kind, sa, rows, mix, dev):
    S, A = sa
    in_dim, out_dim, members = KINDS[kind](S, A)
    c = real_case(31 + rows, kind, S, A, rows, mix)
    ref = R.mlp3_backward_ref(c["W1"], c["W2"], c["W3"], c["x"], c["h1"], c["h2"], c["dz3"])
    geo = R.wgrad_geometry(rows, members)
    n_w = geo["rows_per_wave"] + geo["nsplit"] + 3
    n_b = 32 + -(-geo["ntiles"] // 64) + 6
    aW2, ah1, ax = np.abs(c["W2"].astype(np.float64)), np.abs(c["h1"].astype(np.float64)), np.abs(c["x"].astype(np.float64))
    E2 = FB.C_LAYER * ref["abs_dz2"]
    E1 = FB.C_LAYER * ref["abs_dz1"] + np.stack([(E2[m] @ aW2[m]) * (c["h1"][m] > 0) for m in range(members)])
    bound = {"dz2": E2, "dz1": E1,
             "dW3": n_w * U * ref["abs_dW3"], "db3": n_b * U * ref["abs_db3"],
             "dW2": n_w * U * ref["abs_dW2"] + np.stack([E2[m].T @ ah1[m] for m in range(members)]),
             "db2": n_b * U * ref["abs_db2"] + E2.sum(1),
             "dW1": n_w * U * ref["abs_dW1"] + np.stack([E1[m].T @ ax for m in range(members)]),
             "db1": n_b * U * ref["abs_db1"] + E1.sum(1)}
    g, dz2, dz1 = run_backward(c, in_dim, out_dim, members, dev)
    got = {"dz2": dz2, "dz1": dz1}
    for rk, pk in R.GRAD_KEYS:
        got[rk] = np.stack([g[m][pk] for m in range(members)])
    ratios, fails = {}, []
    for k in ("dz2", "dz1", "dW3", "db3", "dW2", "db2", "dW1", "db1"):
        err = np.abs(got[k].astype(np.float64) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound[k] > 0, err / bound[k], np.where(err == 0, 0.0, np.inf))
        ratios[k] = float(r.max())
    name = f"{kind}-S{S}A{A}-rows{rows}-{mix}"
    RATIOS[name] = dict(ratios, nsplit=geo["nsplit"], rows_per_wave=geo["rows_per_wave"], n_w=n_w, n_b=n_b)
    print(name, {k: f"{v:.3g}" for k, v in ratios.items()})
    for k in ratios:
        FB.check(got[k], ref[k], bound[k], f"{name} {k}")
