"""The documented summation order of the K-split output layer of the fused MLP forward (csrc/tile.h narrow_run and, for a
one-output net, narrow_run_one), emulated in NumPy float32.  This is the statement of what the layer's
v_mfma_f32_16x16x4_f32 sequence does; tests/wgrad_order_ref.py holds the one for v_mfma_f32_32x32x2_f32.

Order, for output element (row, col) of a 256 -> Np layer:
  * wave w contracts k in [64 w, 64 w + 64): one fp32 fma chain from zero.  Step s = 0 .. 15 is one MFMA; the instruction adds
    its four k-blocks q = 0 .. 3 in that order onto the accumulator, and block q of step s holds k = 64 w + 16 q + s.  So the
    chain runs s outer, q inner;
  * the four waves' partial sums meet as ((p0 + p1) + p2) + p3;
  * then + bias.
fma32 is a correctly rounded fp32 fma: the product of two floats is exact in float64, the float64 sum is brought to round-to-odd
with the exact error of the addition (TwoSum), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the single rounding
of the exact a * b + c.
"""
import numpy as np

HID = 256
F32 = np.float32
F64 = np.float64

K_ORDER = [[64 * w + 16 * q + s for s in range(16) for q in range(4)] for w in range(4)]      # per wave, in chain order


def fma32(a, b, c):
    """round_to_float32(a * b + c), elementwise, one rounding."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)          # exact: 24 + 24 bits
    c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)                                                 # s + err == p + c exactly
    bits = s.copy().view(np.int64)
    odd = (err != 0) & ((bits & 1) == 0)                                          # inexact and even: take the odd neighbour on err's side
    step = np.where((err > 0) == (s > 0), 1, -1)
    bits += np.where(odd, step, 0)
    return bits.view(F64).astype(F32)


def out_layer(h2, w3col, bias, order=K_ORDER):
    """h2 [rows][256] fp32, w3col [256], bias scalar -> the layer's column in the documented order; `order`: the k sequence of each wave."""
    h2 = np.asarray(h2, F32)
    w3col = np.asarray(w3col, F32)
    parts = []
    for ks in order:
        acc = np.zeros(h2.shape[0], F32)
        for k in ks:
            acc = fma32(h2[:, k], w3col[k], acc)
        parts.append(acc)
    return (((parts[0] + parts[1]) + parts[2]) + parts[3]) + F32(bias)


def reversed_order():
    return [ks[::-1] for ks in K_ORDER]


def q_outer_order():
    """the other sequential reading of one wave's 64 k: lane quarter outer, step inner (plain increasing k)"""
    return [[64 * w + k for k in range(64)] for w in range(4)]
