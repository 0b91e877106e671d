"""GPU checks of the packed wide MLP (csrc/wide.hip) against the fp64 restatement tests/wide_ref.py.

Forward, per element and per layer, each layer fed the kernel's OWN saved input (x, h1, h2 as the kernel wrote them): a layer's
output is a sequential fp32 sum of Kp products (v_mfma_f32_32x32x2_f32 is a k-ordered fma chain, Kp the padded contraction
length) plus the bias, so with u = 2^-24 its error is at most (Kp + 2) u (|x| |W| + |b|) -- the standard sequential-sum bound; ReLU
is 1-Lipschitz and keeps it.  In the tanh output mode max_action * tanh(z) moves by at most max_action per unit of z, and tanhf
(two units in the last place: 4 u of a value below 1) and the product with max_action cost another 6 u max_action.
Backward: the issue's rtol 1e-5 / atol 1e-5 x the tensor's largest entry, ReLU masks taken from the kernel's saves on both sides.
Adam over three steps: an update is lr m_hat / (sqrt(v_hat) + eps); m, v, the root and the quotient are a dozen roundings of
operands whose ratio |g| / sqrt(v_hat) stays below 4 in the first steps, so each step is within 64 u lr + 2 u |p|.

Row counts: the kernel's row tile is 64, so 1, 63, 65 and 129 rows.
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
BWD_CASES = [FWD_CASES[i] for i in (0, 1, 2, 4, 5, 7, 8)]
IDS = lambda cases: ["h%d-r%d-e%d-%dx%d-%s" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4]) for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def setup(case, dev, seed=11):
    from mobody_amd import _lib, packing
    hidden, rows, E, (in_dim, out_dim), mode, widths, per_member = case
    assert sum(widths) == in_dim
    p = WR.params(seed, in_dim, hidden, out_dim, E)
    rng = np.random.default_rng(seed + 1)
    srcs = [rng.standard_normal(((E, rows, w) if i == per_member else (rows, w))).astype(np.float32) for i, w in enumerate(widths)]
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    blob = packing.pack_wide(*(p[k] for k in WR.KEYS), dev)
    x = np.concatenate([WR.bcast(s, E) for s in srcs], axis=2)
    return p, L, blob, [torch.from_numpy(s).to(dev) for s in srcs], x


def run_forward(case, dev, ma=1.7):
    from mobody_amd import ops
    p, L, blob, srcs, x = setup(case, dev)
    out, xs, h1, h2 = ops.wide_mlp3_forward(blob, L, srcs, out_mode=case[4], max_action=ma, save=True)
    torch.cuda.synchronize()
    return p, L, blob, x, out, xs, h1, h2


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
    c0 = in_dim - widths[-1]                                        # dX for the last source only (the decoder's latent)
    runs = []
    for _ in range(2):
        gbuf = torch.full((L.total_floats + 1,), NAN, device=dev)    # a sentinel float behind the blob
        grad, dx = ops.wide_mlp3_backward(blob, L, dz3_d, xs, h1, h2, grad=gbuf[:-1], dx_cols=(c0, in_dim))
        torch.cuda.synchronize()
        assert torch.isnan(gbuf[-1])
        runs.append((grad.clone(), dx.clone()))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)), "the weight gradient is not bit-identical"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    grad, dx = runs[0]
    pad = packing.wide_padding_mask(in_dim, hidden, out_dim, E, dev)
    assert pad.any() or (hidden % 32 == 0 and in_dim % 16 == 0 and out_dim % 32 == 0)
    assert not grad[pad].view(torch.int32).any(), "gradient padding is not exactly zero"
    want = ref_grads(p, xs.cpu().numpy(), h1.cpu().numpy(), h2.cpu().numpy(), dz3, L, hidden, in_dim, E)
    got = dict(zip(WR.KEYS, (t.cpu().numpy() for t in packing.unpack_wide(grad, in_dim, hidden, out_dim, E))))
    got["dx"], want["dx"] = dx.cpu().numpy(), want["dx"][:, :, c0:]
    for k in WR.KEYS + ("dx",):
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
