"""Per-element error bounds of the split-precision GEMMs against an fp64 reference (tests/test_hip_f16_scaling.py).

For C = A B the standard rounding bound of element (i, j) is  c * sum_k |A_ik| |B_kj|;  nothing here is normalised by the
largest element of a tensor, so a small row, tile or column is held to its own scale.

c:  C_LAYER = 2^-17 for one GEMM fed the kernel's own inputs.  "f16x2" carries 22 significand bits (two fp16 terms; the
    dropped x1 y1 product and the residuals' rounding are ~3 * 2^-22 ~ 2^-20.4 per product), and the fp32 accumulation of
    a K = 256 contraction runs through ~50 dependent MFMA adds (16 k-steps x 3 products), <= ~2^-18.3: together ~2^-17.9.
    The exact fp32 mode ("f32", the control) accumulates 128 K = 2 steps: <= 2^-17.  The worst case of a sequential fp32
    sum over K = 256, 256 * 2^-24 = 2^-16, is C_E2E, used where the split forward's error also reaches the operands
    (end-to-end gradients of Engine.step / pretrain_grads, the forward of a whole net).
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
