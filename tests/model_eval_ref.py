"""Restatement of the per-row accounting of `mobody_ens_evaluate` (include/mobody_hip.h; eval_policy_batch's
`reward_all[i, :done_index[i] + 1]` sums, train_mobody.py:60-98) in NumPy fp32, and an fp64 return for the discounted
bound.  Shared by the CPU tests (hand-made tables) and the GPU tests (the composition's own rewards and flags)."""
import numpy as np


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64 (48 bits), the sum of it and an fp32
    value is rounded once to fp64 and once more to fp32.  The double rounding can differ from a true fma only when the
    fp64 sum lands exactly on an fp32 rounding boundary, which needs more than 53 significant bits in the exact sum: the
    tests' discount-1 sums (a = 1: the product is b itself, the sum of two fp32 values, one rounding) never do."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def new_state(B):
    return dict(alive=np.ones(B, bool), ret=np.zeros(B, np.float32), pen_sum=np.zeros(B, np.float32),
                disc=np.ones(B, np.float32), length=np.zeros(B, np.int32))


def account(st, raw, pen, term, discount):
    """One step (3 and 4 of the semantics) on the row state `st`, in place.  raw / pen: fp32 [B]; term: bool [B] (with or
    without the step's own `!alive` folded in: `alive && !term` is the same).  Dead rows read nothing."""
    a = st["alive"]
    raw, pen = np.asarray(raw, np.float32).reshape(-1), np.asarray(pen, np.float32).reshape(-1)
    st["ret"][a] = fma32(st["disc"][a], raw[a], st["ret"][a])
    st["pen_sum"][a] = (st["pen_sum"][a] + pen[a]).astype(np.float32)
    st["length"][a] += 1
    st["disc"][a] = (st["disc"][a] * np.float32(discount)).astype(np.float32)
    st["alive"] = a & ~np.asarray(term).reshape(-1).astype(bool)
    return st


def evaluate_tables(raw, pen, term, discount=1.0):
    """raw, pen, term: [H][B] tables -> the row state after H steps."""
    st = new_state(np.asarray(raw).shape[1])
    for t in range(np.asarray(raw).shape[0]):
        account(st, raw[t], pen[t], term[t], discount)
    return st


def returns_f64(raw, term, discount):
    """(fp64 discounted return, sum_t |discount^t raw_t|) per row over the steps the row was alive at, from [H][B] tables."""
    raw = np.asarray(raw, np.float64)
    H, B = raw.shape
    alive, ret, mag = np.ones(B, bool), np.zeros(B), np.zeros(B)
    for t in range(H):
        term_t = float(discount) ** t * np.where(alive, raw[t], 0.0)
        ret += term_t
        mag += np.abs(term_t)
        alive = alive & ~np.asarray(term[t]).reshape(-1).astype(bool)
    return ret, mag
