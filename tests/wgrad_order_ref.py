"""The documented summation order of the weight-gradient launches (csrc/mlp_bwd.hip k_wgrad*, k_grad_reduce), emulated in
NumPy on inputs chosen so that the order is all there is to emulate.

Order (the comment block above the weight-gradient GEMM):
  * wave (slice, w) accumulates rows [(4 slice + w) rows_per_wave, ...) in increasing order, one fp32 fma chain per output
    element starting from zero;
  * the four waves of a slice meet as (w0 + w2) + (w1 + w3);
  * k_grad_reduce adds the slabs to 0 in slab order.
Geometry (nsplit, rows_per_wave) is aux_ref.wgrad_geometry's.

Inputs (order_case): every operand of a weight-gradient product is +-m 2^e with an integer 1024 <= m < 2048 (11 significant
bits) and e spread over -10 .. 10, or zero.  A product then has at most 22 significant bits and an exponent far inside the
normal range: it is exact in fp32, so fma(a, b, acc) == round(acc + a b) and the chain is a chain of rounded adds.  The
partial sums do round -- terms 2^40 apart meet in one chain -- so the result depends on the order.  dz1, the operand of dW1,
is made by the backward kernel; W3 and W2 are scaled selection / permutation matrices (one power of two per column), so that
dz2 = dz3[:, sel] 2^p [h2 > 0] and dz1 = dz2[:, perm] 2^q [h1 > 0] are exact copies of dz3 entries with moved exponents.
"""
import numpy as np

import aux_ref as R

HID = 256
F32 = np.float32


def _vals(rng, shape, spread=10):
    m = rng.integers(1024, 2048, shape).astype(np.float64)
    e = rng.integers(-spread, spread + 1, shape)
    s = rng.choice([-1.0, 1.0], shape)
    return (s * np.ldexp(m, e - 10)).astype(F32)


def order_case(seed, in_dim, out_dim, members, rows):
    """x, h1, h2, dz3 and the W1 / W2 / W3 of mobody_mlp3_backward (nn.Linear shapes, aux_ref's conventions), plus the dz2 / dz1
    the backward kernel has to form from them (exact, see the module docstring)."""
    rng = np.random.default_rng(seed)
    x = _vals(rng, (rows, in_dim))
    dz3 = _vals(rng, (members, rows, out_dim))
    h1 = _vals(rng, (members, rows, HID))
    h2 = _vals(rng, (members, rows, HID))
    h1 = np.where(rng.random(h1.shape) < 0.9, np.abs(h1), -np.abs(h1)).astype(F32)      # the ReLU masks drop a tenth
    h2 = np.where(rng.random(h2.shape) < 0.9, np.abs(h2), -np.abs(h2)).astype(F32)
    sel = rng.integers(0, out_dim, (members, HID))                  # dz2[:, j] <- dz3[:, sel[j]]
    p3 = rng.integers(-3, 4, (members, HID))
    perm = np.stack([rng.permutation(HID) for _ in range(members)])  # dz1[:, i] <- dz2[:, perm[i]]
    p2 = rng.integers(-3, 4, (members, HID))
    W3 = np.zeros((members, out_dim, HID), F32)
    W2 = np.zeros((members, HID, HID), F32)                          # [out j][in i]: dh1[i] = sum_j dz2[j] W2[j][i]
    dz2 = np.zeros((members, rows, HID), F32)
    dz1 = np.zeros((members, rows, HID), F32)
    cols = np.arange(HID)
    for m in range(members):
        W3[m, sel[m], cols] = np.ldexp(1.0, p3[m])
        W2[m, perm[m], cols] = np.ldexp(1.0, p2[m])
        dz2[m] = dz3[m][:, sel[m]] * np.ldexp(1.0, p3[m]).astype(F32) * (h2[m] > 0)
        dz1[m] = dz2[m][:, perm[m]] * np.ldexp(1.0, p2[m]).astype(F32) * (h1[m] > 0)
    W1 = np.zeros((members, HID, in_dim), F32)                      # takes no part in any gradient
    return {"W1": W1, "W2": W2, "W3": W3, "x": x, "h1": h1, "h2": h2, "dz3": dz3, "dz2": dz2, "dz1": dz1}


def significand_bits(a):
    """Largest number of significant bits of any entry (0 for zeros)."""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a > 0]
    if a.size == 0:
        return 0
    m, _ = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    return int(53 - np.log2((mi & -mi).astype(np.float64)).min())


def products_exact(c):
    """From the inputs alone: both factors of every weight-gradient product keep at most 11 bits (exact 22-bit product) and
    every product stays in the normal fp32 range -- and, redundantly, one row's products really are equal in fp32 and fp64."""
    ok = True
    for a, b in (("x", "dz1"), ("dz3", "h2")):
        A, B = c[a].reshape(-1, c[a].shape[-1]), c[b].reshape(-1, c[b].shape[-1])
        ok &= significand_bits(A) <= 11 and significand_bits(B) <= 11
        nz = lambda v: np.abs(v[v != 0]).astype(np.float64)
        if nz(A).size and nz(B).size:
            ok &= nz(A).min() * nz(B).min() > 2.0 ** -100 and nz(A).max() * nz(B).max() < 2.0 ** 100
        p64 = np.multiply.outer(A[0].astype(np.float64), B[0].astype(np.float64))
        ok &= bool(np.array_equal(np.multiply.outer(A[0], B[0]).astype(np.float64), p64))
    return bool(ok)


def _chain(A, B, r0, r1):
    """sum over rows r0 .. r1 - 1 of outer(A[r], B[r]) as one sequential fp32 chain per element, from zero."""
    acc = np.zeros((A.shape[1], B.shape[1]), F32)
    for r in range(r0, r1):
        acc += np.multiply.outer(A[r], B[r])            # the product is exact (products_exact): one rounding, the add's
    return acc


def ordered_sum(A, B, rows, members):
    """sum_rows outer(A[row], B[row]) in the launch's order; A [rows][ka], B [rows][nb] fp32."""
    geo = R.wgrad_geometry(rows, members)
    rpw, ns = geo["rows_per_wave"], geo["nsplit"]
    total = np.zeros((A.shape[1], B.shape[1]), F32)
    for s in range(ns):
        w = [_chain(A, B, min(rows, (4 * s + k) * rpw), min(rows, (4 * s + k + 1) * rpw)) for k in range(4)]
        total = total + ((w[0] + w[2]) + (w[1] + w[3]))
    return total


def emulate(c, reverse=False):
    """dW1 [M][256][in] and dW3 [M][out][256] (nn.Linear shapes) in the documented order; reverse: the same launch over the
    rows in reverse order."""
    x, dz1, dz3, h2 = c["x"], c["dz1"], c["dz3"], c["h2"]
    members, rows = dz3.shape[0], x.shape[0]
    if reverse:
        x, dz1, dz3, h2 = x[::-1], dz1[:, ::-1], dz3[:, ::-1], h2[:, ::-1]
    dW1 = np.stack([ordered_sum(x, dz1[m], rows, members).T for m in range(members)])       # xᵀ dz1 -> [in][256] -> [256][in]
    dW3 = np.stack([ordered_sum(dz3[m], h2[m], rows, members) for m in range(members)])     # dz3ᵀ h2 -> [out][256]
    return {"dW1": dW1, "dW3": dW3}
