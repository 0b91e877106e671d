"""GPU checks of the packed wide MLP (csrc/wide.hip) against the fp64 restatement tests/wide_ref.py.

Forward, per element and per layer, each layer fed the kernel's OWN saved input (x, h1, h2 as the kernel wrote them): a layer's
output is a sequential fp32 sum of Kp products (v_mfma_f32_32x32x2_f32 is a k-ordered fma chain, Kp the padded contraction
length) plus the bias, so with u = 2^-24 its error is at most (Kp + 2) u (|x| |W| + |b|) -- the standard sequential-sum bound; ReLU
is 1-Lipschitz and keeps it.  In the tanh output mode max_action * tanh(z) moves by at most max_action per unit of z, and tanhf
(two units in the last place: 4 u of a value below 1) and the product with max_action cost another 6 u max_action.
Backward: the issue's rtol 1e-5 / atol 1e-5 x the tensor's largest entry, ReLU masks taken from the kernel's saves on both sides.
Adam over three steps: an update is lr m_hat / (sqrt(v_hat) + eps); m, v, the root and the quotient are a dozen roundings of
operands whose ratio |g| / sqrt(v_hat) stays below 4 in the first steps, so each step is within 64 u lr + 2 u |p|.

Row counts: the kernel's row tile is 64, so 1, 63, 65 and 129 rows; wide_ref.CORNER_CASES adds the corners of the layout's domain
(every minimum and maximum, the shapes without padding, rows of exactly 16, 64 and 128, out_dim 65), whose backward tolerance
tests/test_wide_ref.py shows reachable in fp32.  Periodic sources (src_rows) and the workspace path of the forward have tests of
their own below: both are copies or the same launches on other memory, so they are compared bit for bit.
"""
import numpy as np
import pytest
import torch

import wide_ref as WR

pytestmark = pytest.mark.gpu
U = WR.U
NAN = float("nan")
ROW_TILE = 64
W, P = WR.NET_SHAPES["walker"], WR.NET_SHAPES["pen"]

# (hidden, rows, members, (in, out), output mode, source widths, index of the per-member source or None)
FWD_CASES = [
    (8, 1, 1, W["pol_enc"], "raw", (17, 6), None),
    (8, ROW_TILE - 1, 5, P["dyn_dec"], "raw", (45, 24, 90), 2),
    (72, ROW_TILE + 1, 1, W["pol_dec"], "tanh", (17, 12), None),
    (72, ROW_TILE - 1, 5, W["dyn_enc"], "raw", (17, 6, 17), None),
    (72, 2 * ROW_TILE + 1, 5, P["dyn_enc"], "raw", (45, 24, 45), None),
    (256, 2 * ROW_TILE + 1, 5, W["dyn_dec"], "raw", (17, 6, 34), 2),
    (256, 1, 5, P["pol_enc"], "tanh", (69,), None),
    (750, ROW_TILE + 1, 5, W["dyn_dec"], "raw", (17, 6, 34), 2),
    (750, 1, 1, P["pol_dec"], "tanh", (45, 48), None),
    (750, ROW_TILE - 1, 1, P["pol_enc"], "raw", (45, 24), None),
]
BWD_CASES = [FWD_CASES[i] for i in (0, 1, 2, 4, 5, 7, 8)] + WR.CORNER_CASES
FWD_CASES = FWD_CASES + WR.CORNER_CASES
IDS = lambda cases: ["h%d-r%d-e%d-%dx%d-%s" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4]) for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def setup(case, dev, seed=11):
    from mobody_amd import _lib, packing
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    p, srcs, x = WR.case_inputs(case, seed)
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    blob = packing.pack_wide(*(p[k] for k in WR.KEYS), dev)
    return p, L, blob, [torch.from_numpy(s).to(dev) for s in srcs], x


def run_forward(case, dev, ma=1.7):
    from mobody_amd import ops
    p, L, blob, srcs, x = setup(case, dev)
    out, xs, h1, h2 = ops.wide_mlp3_forward(blob, L, srcs, out_mode=case[4], max_action=ma, save=True)
    torch.cuda.synchronize()
    return p, L, blob, x, out, xs, h1, h2


def check_padding_dims(L, pad):
    """wide_padding_mask dimension by dimension: W1's rows past in_dim, b1 past hidden, b3 past out_dim hold exactly the layout's
    padding, so in a dimension without padding the mask is EMPTY there (asserted, not skipped)."""
    m = pad.view(L.members, L.member_floats)
    dims = {"in": (m[:, L.w1:L.b1].view(L.members, L.Kp1, L.Hp)[:, :, 0], L.Kp1 - L.in_dim, L.in_dim % 16 == 0),
            "hidden": (m[:, L.b1:L.w2], L.Hp - L.hidden, L.hidden % 32 == 0),
            "out": (m[:, L.b3:], L.Np3 - L.out_dim, L.out_dim % 32 == 0)}
    for name, (part, n, exact) in dims.items():
        assert int(part.sum()) == L.members * n and (n == 0) == exact, name
        if exact:
            assert not part.any(), "%s has no padding, but the mask marks some" % name
    n_real = L.in_dim * L.hidden + L.hidden * L.hidden + L.hidden * L.out_dim + 2 * L.hidden + L.out_dim
    assert int(pad.sum()) == L.total_floats - L.members * n_real


@pytest.mark.parametrize("case", FWD_CASES, ids=IDS(FWD_CASES))
def test_forward_per_element_vs_fp64(dev, case):
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    ma = 1.7
    p, L, blob, x, out, xs, h1, h2 = run_forward(case, dev, ma)
    p64 = WR.f64(p)
    xs, h1, h2, out = (t.cpu().numpy() for t in (xs, h1, h2, out))
    assert xs.shape == ((1 if per_member is None else E), rows, L.Kp1) and h1.shape == h2.shape == (E, rows, L.Hp)
    # the concatenated input is a copy, its padding and the hidden padding are exactly zero
    assert np.array_equal(xs[:, :, :in_dim], (x if per_member is not None else x[:1]).astype(np.float32))
    assert not xs[:, :, in_dim:].any() and not h1[:, :, hidden:].any() and not h2[:, :, hidden:].any()
    from mobody_amd import packing
    check_padding_dims(L, packing.wide_padding_mask(in_dim, hidden, out_dim, E))
    xk = WR.bcast(xs[:, :, :in_dim], E)
    worst = 0.0
    for inp, Wk, bk, Kp, got, relu in ((xk, "W1", "b1", L.Kp1, h1[:, :, :hidden], True),
                                       (h1[:, :, :hidden].astype(np.float64), "W2", "b2", L.Hp, h2[:, :, :hidden], True),
                                       (h2[:, :, :hidden].astype(np.float64), "W3", "b3", L.Hp, out, False)):
        z, mag = WR.layer(inp, p64[Wk], p64[bk])
        bound = (Kp + 2) * U * mag
        if relu:
            want = np.maximum(z, 0.0)
        elif mode == "tanh":
            want, bound = ma * np.tanh(z), ma * (bound + 6 * U)
        else:
            want = z
        ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
        worst = max(worst, float(ratio.max()))
        print("%s: worst error / bound %.3f" % (Wk, ratio.max()))
        assert (np.abs(got - want) <= bound).all(), (Wk, float(ratio.max()))
    # end to end too, loosely: the three layers chained in fp64 (catches a layer wired to the wrong input)
    want = WR.forward(p, x, mode, ma)[0]
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * np.abs(want).max())


def ref_grads(p, xs, h1, h2, dz3, L, hidden, in_dim, E):
    return WR.backward(p, WR.bcast(xs[:, :, :in_dim], E), h1[:, :, :hidden], h2[:, :, :hidden], dz3)


@pytest.mark.parametrize("case", BWD_CASES, ids=IDS(BWD_CASES))
def test_backward_vs_fp64_padding_zero_and_bit_identical(dev, case):
    from mobody_amd import ops, packing
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    p, L, blob, x, out, xs, h1, h2 = run_forward(case, dev)
    rng = np.random.default_rng(5)
    dz3 = rng.standard_normal((E, rows, out_dim)).astype(np.float32)
    dz3_d = torch.from_numpy(dz3).to(dev)
    corner = case in WR.CORNER_CASES
    c0 = 0 if corner else in_dim - widths[-1]                       # dX for the last source only (the decoder's latent) | all of it
    runs = []
    for _ in range(2):
        gbuf = torch.full((L.total_floats + 1,), NAN, device=dev)    # a sentinel float behind the blob
        grad, dx = ops.wide_mlp3_backward(blob, L, dz3_d, xs, h1, h2, grad=gbuf[:-1], dx_cols=(c0, in_dim))
        assert dx.shape == (E, rows, in_dim - c0)
        torch.cuda.synchronize()
        assert torch.isnan(gbuf[-1])
        runs.append((grad.clone(), dx.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "the weight gradient is not bit-identical"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    grad, dx = runs[0]
    pad = packing.wide_padding_mask(in_dim, hidden, out_dim, E, dev)
    assert pad.any() or (hidden % 32 == 0 and in_dim % 16 == 0 and out_dim % 32 == 0)
    check_padding_dims(L, pad)
    assert not grad[pad].view(torch.int32).any(), "gradient padding is not exactly zero"
    want = ref_grads(p, xs.cpu().numpy(), h1.cpu().numpy(), h2.cpu().numpy(), dz3, L, hidden, in_dim, E)
    got = dict(zip(WR.KEYS, (t.cpu().numpy() for t in packing.unpack_wide(grad, in_dim, hidden, out_dim, E))))
    full_dx = want["dx"]
    got["dx"], want["dx"] = dx.cpu().numpy(), full_dx[:, :, c0:]
    keys = WR.KEYS + ("dx",)
    if (in_dim, out_dim) == (256, 256):                              # a middle column range too, across the sources' seams
        mid = ops.wide_mlp3_backward(blob, L, dz3_d, xs, h1, h2, dx_cols=(99, 201))[1]
        assert torch.equal(mid.view(torch.int32), dx[:, :, 99:201].contiguous().view(torch.int32))
        got["dx[99:201]"], want["dx[99:201]"] = mid.cpu().numpy(), full_dx[:, :, 99:201]
        keys += ("dx[99:201]",)
    for k in keys:
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]) / (1e-5 * scale + 1e-5 * np.abs(want[k]))
        print("%s: worst error / tolerance %.3f" % (k, err.max()))
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=1e-5 * scale, err_msg=k)


def test_dx_column_ranges(dev):
    """Every column range of dX is the matching slice of the full one, bit for bit (the range only offsets W1's rows)."""
    from mobody_amd import ops
    case = (72, 33, 2, W["dyn_dec"], "raw", (17, 6, 34), 2)
    p, L, blob, x, out, xs, h1, h2 = run_forward(case, dev)
    dz3 = torch.from_numpy(np.random.default_rng(2).standard_normal((2, 33, 17)).astype(np.float32)).to(dev)
    full = ops.wide_mlp3_backward(blob, L, dz3, xs, h1, h2, dx_cols=(0, 57))[1]
    for c0, c1 in ((0, 1), (17, 23), (23, 57), (56, 57)):
        part = ops.wide_mlp3_backward(blob, L, dz3, xs, h1, h2, dx_cols=(c0, c1))[1]
        assert torch.equal(part, full[:, :, c0:c1].contiguous()), (c0, c1)
    assert ops.wide_mlp3_backward(blob, L, dz3, xs, h1, h2)[1] is None


@pytest.mark.parametrize("hidden,E,shape", [(72, 5, W["dyn_enc"]), (750, 1, W["pol_dec"])], ids=["h72-e5", "h750-e1"])
def test_adam_vs_fp64_device_count_and_padding(dev, hidden, E, shape):
    from mobody_amd import ops, packing
    in_dim, out_dim = shape
    case = (hidden, 33, E, shape, "raw", (in_dim,), None)
    p, L, blob, srcs, x = setup(case, dev)
    lr, steps = 3e-4, 3
    pad = packing.wide_padding_mask(in_dim, hidden, out_dim, E, dev)
    rng = np.random.default_rng(9)
    blob_dev = blob.clone()
    m, v, m2, v2 = (torch.zeros_like(blob) for _ in range(4))
    t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    p64, m64, v64 = blob.cpu().numpy().astype(np.float64), 0.0, 0.0
    bound = np.zeros_like(p64)
    for t in range(1, steps + 1):
        g = rng.standard_normal(blob.numel()).astype(np.float32) * (rng.random(blob.numel()) < 0.9)     # some exact zeros
        g[pad.cpu().numpy()] = 0.0                                   # what mobody_wide_mlp3_backward writes there
        gd = torch.from_numpy(g).to(dev)
        ops.wide_adam(blob, gd, m, v, lr, t=t)
        t_dev += 1
        ops.wide_adam(blob_dev, gd, m2, v2, lr, t_dev=t_dev)
        p64, m64, v64 = WR.adam(p64, g.astype(np.float64), m64, v64, t, lr)
        bound += 64 * U * lr + 2 * U * np.abs(p64)
        err = np.abs(blob.cpu().numpy() - p64)
        print("step %d: worst error / bound %.3f" % (t, (err / bound).max()))
        assert (err <= bound).all(), t
    for a, b in ((blob, blob_dev), (m, m2), (v, v2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "host and device step counts differ"
    for tns in (blob, m, v):
        assert not tns[pad].view(torch.int32).any(), "padding moved"


def test_training_keeps_padding_zero_through_real_gradients(dev):
    """Three forward / backward / Adam rounds at a shape with padding in every dimension: blob, gradient and moments stay 0 there."""
    from mobody_amd import ops, packing
    case = (72, 33, 2, W["dyn_dec"], "raw", (17, 6, 34), 2)
    p, L, blob, srcs, x = setup(case, dev)
    pad = packing.wide_padding_mask(57, 72, 17, 2, dev)
    assert int(pad.sum()) > 0
    m, v = torch.zeros_like(blob), torch.zeros_like(blob)
    before = blob.clone()
    for t in (1, 2, 3):
        out, xs, h1, h2 = ops.wide_mlp3_forward(blob, L, srcs, save=True)
        grad, _ = ops.wide_mlp3_backward(blob, L, (out * (2.0 / out.numel())).contiguous(), xs, h1, h2)
        ops.wide_adam(blob, grad, m, v, 1e-3, t=t)
        for tns in (blob, grad, m, v):
            assert not tns[pad].view(torch.int32).any(), t
    assert not torch.equal(before, blob) and torch.isfinite(blob).all()


# ---- periodic sources (src_rows: row r of x reads row r % period of the source) ---------------------------------------------------
PERIODIC_ROWS, PERIODIC_E = 70, 3
# name -> per source (width, per member?, periodic?): a periodic source next to a full shared one (x shared between members) and
# periodic sources, shared and per member, next to a full per-member one (the estimator's decoder: states | actions | latents)
PERIODIC_MIXES = {"shared": ((5, False, True), (18, False, False)),
                  "member": ((5, False, True), (9, True, True), (9, True, False))}


@pytest.mark.parametrize("mix", list(PERIODIC_MIXES))
@pytest.mark.parametrize("period", [1, 7, 11, 35, 70])        # 7 and 35 divide the 70 rows, 11 does not, 70 is the full source
def test_periodic_sources_are_the_tiled_sources_bit_for_bit(dev, period, mix):
    from mobody_amd import _lib, ops, packing
    rows, E, hidden = PERIODIC_ROWS, PERIODIC_E, 72
    in_dim, out_dim = W["pol_enc"]
    spec = PERIODIC_MIXES[mix]
    assert sum(w for w, _, _ in spec) == in_dim
    p = WR.params(3, in_dim, hidden, out_dim, E)
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    blob = packing.pack_wide(*(p[k] for k in WR.KEYS), dev)
    rng = np.random.default_rng(period)
    given, tiled = [], []
    for w, member, periodic in spec:
        n = period if periodic else rows
        s = rng.standard_normal(((E, n, w) if member else (n, w))).astype(np.float32)
        given.append(s)
        tiled.append(np.ascontiguousarray(s[..., np.arange(rows) % n, :]))             # NumPy's tiling: row r <- row r % period
    td = lambda a: torch.from_numpy(a).to(dev)
    got = ops.wide_mlp3_forward(blob, L, [td(s) for s in given], save=True, source_rows=[period if s[2] else None for s in spec])
    want = ops.wide_mlp3_forward(blob, L, [td(s) for s in tiled], save=True)
    torch.cuda.synchronize()
    xs = got[1].cpu().numpy()
    shared = not any(member for _, member, _ in spec)
    assert xs.shape == (1 if shared else E, rows, L.Kp1) and L.Kp1 > in_dim
    x_np = np.concatenate([np.broadcast_to(t, (xs.shape[0], rows, t.shape[-1])) for t in tiled], axis=2)
    assert np.array_equal(xs[:, :, :in_dim].view(np.int32), x_np.view(np.int32)), "x is not the tiling of the sources"
    assert not xs[:, :, in_dim:].view(np.int32).any(), "x's padding is not exactly zero"
    for name, a, b in zip(("out", "x", "h1", "h2"), got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert torch.isfinite(got[0]).all() and got[0].abs().max() > 0


def test_period_beyond_rows_is_refused(dev):
    from mobody_amd import _lib, ops, packing
    rows, E = PERIODIC_ROWS, PERIODIC_E
    in_dim, out_dim = W["pol_enc"]
    L = _lib.wide_layout(in_dim, 72, out_dim, E)
    blob = torch.zeros(L.total_floats, device=dev)
    full, over = torch.zeros(rows, 18, device=dev), torch.zeros(rows + 1, 5, device=dev)
    with pytest.raises(_lib.MobodyError, match=r"source 0: src_rows 71 outside \[0, rows\]"):
        ops.wide_mlp3_forward(blob, L, [over, full], source_rows=[rows + 1, None])
    ops.wide_mlp3_forward(blob, L, [over[:rows], full], source_rows=[rows, None])        # the largest period passes


# ---- the workspace path: saves the caller does not want are carved from `workspace` ------------------------------------------------
@pytest.mark.parametrize("case", [(72, ROW_TILE + 1, 3, W["dyn_enc"], "raw", (17, 6, 17), None),
                                  (72, ROW_TILE + 1, 3, W["dyn_dec"], "tanh", (17, 6, 34), 2)], ids=["shared-x", "per-member-x"])
def test_forward_without_saves_runs_in_the_workspace(dev, case):
    import ctypes as C
    from mobody_amd import _lib, ops
    from mobody_amd.ops import check, cur_stream, load, ptr
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    p, L, blob, srcs, x = setup(case, dev)
    want, xs, h1, h2 = ops.wide_mlp3_forward(blob, L, srcs, out_mode=mode, max_action=1.7, save=True)
    need = load().mobody_wide_mlp3_forward_workspace(C.byref(L), rows)
    assert need == E * rows * (L.Kp1 + 2 * L.Hp)
    guard = 64
    ws = torch.full((need + guard,), NAN, device=dev)                                 # NaN sentinels behind the workspace
    out = torch.full((E, rows, out_dim), NAN, device=dev)
    fields = dict(layout=L, blob=ptr(blob), x_shared=int(per_member is None), rows=rows, out_mode=_lib.WIDE_OUT_MODES[mode],
                  max_action=1.7, out=ptr(out))
    for i, s in enumerate(srcs):
        fields.update({"src%d" % i: ptr(s), "src_width%d" % i: s.shape[-1], "src_member_stride%d" % i: 0 if s.dim() == 2 else rows * s.shape[-1]})
    a = _lib.block(_lib.MobodyWideFwd, workspace=ptr(ws), **fields)
    assert not a.save_x and not a.save_h1 and not a.save_h2
    check(load().mobody_wide_mlp3_forward(C.byref(a), cur_stream()), "mobody_wide_mlp3_forward")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)), "the workspace path's output differs from the saving call's"
    assert (ws[need:].view(torch.int32) == 0x7FC00000).all(), "the forward wrote behind its workspace"
    # the carving the header states: x [members rows Kp1] (a shared x fills the first member's part), then h1, then h2
    nx, nh = E * rows * L.Kp1, E * rows * L.Hp
    assert torch.equal(ws[:xs.numel()].view(torch.int32), xs.reshape(-1).view(torch.int32))
    assert torch.equal(ws[nx:nx + nh].view(torch.int32), h1.reshape(-1).view(torch.int32))
    assert torch.equal(ws[nx + nh:need].view(torch.int32), h2.reshape(-1).view(torch.int32))
    # one save given, two carved: the same output again
    out.fill_(NAN)
    h1b = torch.full_like(h1, NAN)
    b = _lib.block(_lib.MobodyWideFwd, workspace=ptr(ws), save_h1=ptr(h1b), **fields)
    check(load().mobody_wide_mlp3_forward(C.byref(b), cur_stream()), "mobody_wide_mlp3_forward")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(h1b.view(torch.int32), h1.view(torch.int32))
    assert (ws[need:].view(torch.int32) == 0x7FC00000).all()
    # a null save without a workspace is refused
    c = _lib.block(_lib.MobodyWideFwd, save_x=ptr(xs), save_h1=ptr(h1), **fields)
    assert load().mobody_wide_mlp3_forward(C.byref(c), cur_stream()) == -1
    assert "a null save needs the workspace" in load().mobody_last_error().decode()


def test_refusals_name_the_argument(dev):
    from mobody_amd import _lib, ops
    case = (72, 8, 2, W["dyn_enc"], "raw", (17, 6, 17), None)
    p, L, blob, srcs, x = setup(case, dev)
    with pytest.raises(_lib.MobodyError, match="exact fp32"):
        ops.wide_mlp3_forward(blob, L, srcs, precision="f16x2")
    with pytest.raises(_lib.MobodyError, match="add up to 23"):
        ops.wide_mlp3_forward(blob, L, srcs[:2])
    out, xs, h1, h2 = ops.wide_mlp3_forward(blob, L, srcs, save=True)
    dz3 = torch.zeros_like(out)
    with pytest.raises(_lib.MobodyError, match="exact fp32"):
        ops.wide_mlp3_backward(blob, L, dz3, xs, h1, h2, precision=4)
    with pytest.raises(_lib.MobodyError, match="step t must be >= 1"):
        ops.wide_adam(blob, torch.zeros_like(blob), torch.zeros_like(blob), torch.zeros_like(blob), 1e-3, t=0)
