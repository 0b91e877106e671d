"""Per-element error bounds of the split-precision GEMMs against an fp64 reference (tests/test_hip_f16_scaling.py).

For C = A B the standard rounding bound of element (i, j) is  c * sum_k |A_ik| |B_kj|;  nothing here is normalised by the
largest element of a tensor, so a small row, tile or column is held to its own scale.

c:  C_LAYER = 2^-17 for one GEMM fed the kernel's own inputs.  "f16x2" carries 22 significand bits (two fp16 terms; the
    dropped x1 y1 product and the residuals' rounding are ~3 * 2^-22 ~ 2^-20.4 per product), and the fp32 accumulation of
    a K = 256 contraction runs through ~50 dependent MFMA adds (16 k-steps x 3 products), <= ~2^-18.3: together ~2^-17.9.
    The exact fp32 mode ("f32", the control) accumulates 128 K = 2 steps: <= 2^-17.  The worst case of a sequential fp32
    sum over K = 256, 256 * 2^-24 = 2^-16, is C_E2E, used where the split forward's error also reaches the operands
    (end-to-end gradients of Engine.step / pretrain_grads, the forward of a whole net).
    C_BF16X3 = C_LAYER for one "bf16x3" GEMM (tests/test_hip_bf16x3.py).  Three bf16 terms hold all 24 significand bits
    (|t1| <= 2^-8 |x|, |t2| <= 2^-17 |x|, nothing left over), so the only operand error is the three dropped pairs:
    x1 y2 + x2 y1 + x2 y2 <= 2 * 2^-25 + 2^-34 ~ 2^-24 per product.  The fp32 accumulation of K = 256 runs through
    16 k-steps x 6 products = 96 dependent MFMA adds (bf_gemm; the weight gradient's 16-row blocks give fewer per wave),
    <= 96 * 2^-24 = 2^-17.4: together ~2^-17.4 < 2^-17.  bf16 keeps fp32's exponent range: no scaling, hence no
    subnormal term and no slice floor (split=False).  tests/test_bf16x3_ref.py shows that a product without the pair
    (1, 1), without (0, 2) and (2, 0), or with two planes only misses this c.
tiny_abs:
  * SUBNORMAL = 2^-39: "f16x2" scales each 32-row tile so that its largest magnitude m lands in [2^13, 2^14); the residual
    term of a value far below m falls into fp16 subnormals, an absolute error of ~2^-39 m per operand (csrc/tile_bf.h).
  * the weight-gradient slice floor: the plane-fed weight-gradient GEMM drops a tile whose scale is more than 2^24 below the
    dominant tile of its wave's row slice; such a tile t contributes at most 32 * max|A_t| * max|B_t| per element and can
    only be dropped if that product is below ~2^-23 of the largest tile's.
"""
import numpy as np
import torch

C_LAYER = 2.0 ** -17
C_E2E = 2.0 ** -16
C_BF16X3 = C_LAYER
SUBNORMAL = 2.0 ** -39
SWISH_LIP = 1.1                     # max |d swish / dz| = 1.0998


def f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, np.float64)


def tile_max(x, tb=32, pad=0.0):
    """Largest finite |x| of each `tb`-row tile (rows on axis -2, over every column), broadcast back to the rows [..., rows, 1].
    `pad`: magnitude of the padding rows of a ragged last tile (the kernels' padding rows hold act(bias))."""
    a = np.abs(f64(x))
    a = np.where(np.isfinite(a), a, 0.0)
    rows = a.shape[-2]
    nt = -(-rows // tb)
    full = np.zeros(a.shape[:-2] + (nt * tb, a.shape[-1]))
    full[..., :rows, :] = a
    if rows % tb:
        full[..., rows:, :] = pad
    m = full.reshape(a.shape[:-2] + (nt, tb * a.shape[-1])).max(-1)
    return np.repeat(m, tb, axis=-1)[..., :rows, None]


def layer_bound(x, W, b, c=C_LAYER, split=False, tb=32, pad=0.0):
    """fp64 z = x W + b (x [.., rows, K], W [.., K, N]) and its bound c (|x| |W| + |b|) (+ the subnormal floor
    2^-39 * tile max |x| * sum_k |W_kj| when the layer runs on the "f16x2" core)."""
    x, W, b = f64(x), f64(W), f64(b)
    z = x @ W + b
    bnd = c * (np.abs(x) @ np.abs(W) + np.abs(b))
    if split:
        bnd = bnd + SUBNORMAL * tile_max(x, tb, pad) * np.abs(W).sum(-2, keepdims=True)
    return z, bnd


def wgrad_floor(A, Bz, tb=32):
    """tiny_abs of the plane-fed weight gradient A^T Bz (A [.., rows, K], Bz [.., rows, N]): the subnormal floor of every
    tile plus the slice floor (see the module docstring).  Returns [.., K, N]."""
    A, Bz = np.abs(f64(A)), np.abs(f64(Bz))
    ta, tbz = tile_max(A, tb)[..., 0], tile_max(Bz, tb)[..., 0]          # [.., rows]
    # a product a b of one row carries (2^-39 max|A_tile|) |b| + |a| (2^-39 max|Bz_tile|)
    sub = SUBNORMAL * (ta[..., None, :] @ Bz + np.swapaxes(A, -1, -2) @ tbz[..., :, None])
    p = (ta * tbz)[..., ::tb]                                            # per-tile product of the maxima
    pmax = p.max(-1, keepdims=True)
    small = np.where(p < 2.0 ** -22 * pmax, p, 0.0).sum(-1)
    return sub + 32.0 * small[..., None, None]


def check(got, ref, bound, what):
    """Assert |got - ref| <= bound element by element (NaN / Inf in `got` fail)."""
    got, ref, bound = f64(got), f64(ref), np.broadcast_to(f64(bound), np.shape(ref))
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        ratio = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.inf)
        w = np.unravel_index(np.nanargmax(np.where(np.isfinite(ratio), ratio, np.inf)), ratio.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound; first {i}: got {got[i]!r} "
                             f"ref {ref[i]!r} bound {bound[i]!r}; worst {w}: err / bound = {ratio[w]:.3g}")


def net_weights(p, pre):
    return [(p[pre + f"network.{i}.weight"].T.astype(np.float64), p[pre + f"network.{i}.bias"].astype(np.float64)) for i in (0, 2, 4)]


def e2e_bound(x, layers, c, split_mode, pad1, lip=1.0, act=lambda z: np.maximum(z, 0.0), E0=None):
    """fp64 forward of a 3-layer net and a bound on the error of its pre-output, propagated layer by layer:
    E_l = lip |W_l|^T E_(l-1) + c (|h||W_l| + |b_l|) (+ subnormal floor of the split layer 2); E0: error of the input."""
    h, E = f64(x), (0.0 if E0 is None else E0)
    for li, (W, b) in enumerate(layers):
        z, bnd = layer_bound(h, W, b, c, split=split_mode and li == 1, pad=pad1 if li == 1 else 0.0)
        E = (lip if li else 1.0) * (E @ np.abs(W) if (li or E0 is not None) else 0.0) + bnd
        h = act(z) if li < 2 else z
    return h, E


def grad_bounds(tape, c, split, which, edz3=None, ex=None):
    """Per-element bounds of every gradient tensor of the nets whose layers were recorded under the prefix `which` (nn.Linear
    layout): c (sum_calls |dz|^T |x| + the error the split GEMM dz_(l+1) W_(l+1)^T passes into dz_l) + the floors of the
    plane-fed layer-2 weight gradient (+ |x|^T Edz, edz3 = a bound on the error of the output gradient that the forward's
    error carries in: a TD error q - y far below |q| amplifies it; + |dz|^T Ex, ex = the forward error of each layer's input,
    which a large dz amplifies where the input itself is small)."""
    out = {}
    E = {4: edz3}
    if edz3 is not None:
        for i in (2, 0):
            W = tape["_W"][which + f"network.{i + 2}.weight"]
            E[i] = (E[i + 2] @ np.abs(W)) * (f64(tape[which + f"network.{i}"][0]["z"]) > 0)
    for i in (0, 2, 4):
        name = which + f"network.{i}"
        recs = tape[name]
        gW = sum(np.abs(f64(r["dz"])).T @ np.abs(f64(r["x"])) for r in recs)
        gb = sum(np.abs(f64(r["dz"])).sum(0) for r in recs)
        if i < 4:                                              # dz_l = (dz_(l+1) W_(l+1)^T) [z_l > 0] carries c |dz_(l+1)| |W_(l+1)|
            W = tape["_W"][which + f"network.{i + 2}.weight"]
            for r, rn in zip(recs, tape[which + f"network.{i + 2}"]):
                prop = (np.abs(f64(rn["dz"])) @ np.abs(W)) * (f64(r["z"]) > 0)
                gW = gW + prop.T @ np.abs(f64(r["x"]))
                gb = gb + prop.sum(0)
        bW, bb = c * gW, c * gb
        if edz3 is not None:
            bW = bW + E[i].T @ np.abs(f64(recs[0]["x"]))
            bb = bb + E[i].sum(0)
        if ex is not None and i in ex:
            bW = bW + (np.abs(f64(recs[0]["dz"])) + (E[i] if edz3 is not None else 0.0)).T @ ex[i]
        if split and i == 2:
            bW = bW + sum(wgrad_floor(r["x"], r["dz"]).T for r in recs)
        out[name + ".weight"], out[name + ".bias"] = bW, bb
    return out


def input_gradient(layers, x):
    """fp64 z3 [rows, out] of a 3-layer ReLU net and d z3[:, 0] / d x [rows, in] (the net is piecewise linear in x)."""
    (W1, b1), (W2, b2), (W3, b3) = layers
    z1 = x @ W1 + b1
    z2 = np.maximum(z1, 0) @ W2 + b2
    g = ((W3[:, 0] * (z2 > 0)) @ W2.T * (z1 > 0)) @ W1.T
    return np.maximum(z2, 0) @ W3 + b3, g


def robust_rows(pa, pq, s, a, thr=2.0 ** -18, max_action=1.0):
    """Rows whose fp64 hidden pre-activations (both Q nets at (s, a) and (s, pi(s)), the actor at s) all keep |z| above thr of
    their own rounding scale |W||h| + |b|: a ReLU mask there cannot flip under the kernels' error.  And rows whose
    |q0 - q1| at (s, pi(s)) is above the forward bound of q0 - q1, so that the branch of min(q0, q1) -- and the 1/2 split of
    a tie -- cannot differ between an fp32 and the fp64 evaluation.  That bound is, per member, the forward bound of q at the
    exact pi (C_E2E, split layer 2) plus |dq/da| E_pi: with its masks fixed q is linear in a, so the policy's own forward
    error E_pi reaches q through the gradient itself, not through products of |W|."""
    ok = np.ones(len(s), bool)

    def scan(layers, x):
        nonlocal ok
        h = x
        for (W, b) in layers[:2]:
            z = h @ W + b
            ok &= (np.abs(z) >= thr * (np.abs(h) @ np.abs(W) + np.abs(b))).all(1)
            h = np.maximum(z, 0)
        return h @ layers[2][0] + layers[2][1]
    s64, a64 = s.astype(np.float64), a.astype(np.float64)
    la = net_weights(pa, "network.")
    pi = max_action * np.tanh(scan(la, s64))
    Epi = max_action * e2e_bound(s64, la, C_E2E, True, np.maximum(la[0][1], 0).max())[1]       # tanh is 1-Lipschitz
    qs, Eq = [], 0.0
    for pre in ("network1.", "network2."):
        lq = net_weights(pq, pre)
        scan(lq, np.concatenate([s64, a64], 1))
        x = np.concatenate([s64, pi], 1)
        scan(lq, x)
        q, g = input_gradient(lq, x)
        qs.append(q[:, 0])
        Eq = Eq + e2e_bound(x, lq, C_E2E, True, np.maximum(lq[0][1], 0).max())[1][:, 0] + (np.abs(g[:, s.shape[1]:]) * Epi).sum(1)
    ok &= np.abs(qs[0] - qs[1]) > Eq
    return ok
