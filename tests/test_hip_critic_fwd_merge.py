"""The critic step's forwards merged into one launch (csrc/critic_fwd_bf.hip): mobody_critic with a `gather` block evaluates
pi(s') inside the target-Q workgroups where the merged kernel applies (f16x2, an s' tile that fits behind the LDS image).

Everything is bit-for-bit against the path every other caller takes -- mobody_gather_batch_rng, then mobody_critic without
`gather` (the two forward launches): same draws, same loads, same arithmetic per output element, so there is no tolerance.
Shapes the merged kernel does not take ((111, 8) and (45, 24): a tile's [s' | a'] rows do not fit behind the image at four
workgroups per CU; every shape in the f32 mode) run the same cases through the launches they keep."""
import functools

import pytest
import torch

import golden_util as gu
from mobody_amd import ops

SHAPES = [(17, 6), (11, 3), (23, 17),            # (23, 17): an actor output layer of 32 columns in the merged launch
          (45, 24), (111, 8)]                    # S + A > 59: these stay on two launches
ROWS = [1, 31, 32, 33, 65, 257, 4097,            # one tile, a ragged last tile, 2, 3, 9 and 129 tiles
        3264, 3265]                              # 102 | 103 tiles: the last launch of the two-chain form, the first of the one-chain form
RING_ROWS = (1000, 7, 300)                       # src | tar | fake, of different sizes: every role of a row tile must draw the same rows
PAD = 5                                          # sentinel rows behind the minibatch arrays


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _rings(S, A):
    """Three packed rings with every float (padding included) random, and their {ptr, size} words."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(2000 * S + A)
    pitch = ops.ring_pitch(S, A)
    out = []
    for rows in RING_ROWS:
        store = torch.randn(rows, pitch, generator=g).to(dev)
        out.append((ops.RingView(store, S, A), torch.tensor([0, rows], dtype=torch.int64, device=dev)))
    return out


@functools.lru_cache(maxsize=None)
def _nets(S, A, mfma):
    from mobody_amd import engine
    pa, pq, _ = gu.policy_params(5, S, A)
    return engine.Engine(S, A, pa, pq, torch.device("cuda:0"))        # built under MOBODY_MFMA = mfma (the fixture set it)


def _counts(N, Nt):
    """Rows per ring (src, tar, fake): the Nt true rows from the two source rings, the rest from the fake ring."""
    return (Nt - Nt // 2, Nt // 2, N - Nt)


def _critic_call(S, A, mfma, N, Nt, policy_forward, merged):
    """One critic update from a fixed state; returns every tensor it can have written."""
    dev = torch.device("cuda:0")
    eng = _nets(S, A, mfma)
    cfg = gu.policy_cfg(S, A, mfma=mfma)
    used = [(r, c) for r, c in zip(_rings(S, A), _counts(N, Nt)) if c > 0]
    dims, hyp = ops.train_dims(S, A, N, Nt), ops.hyper(cfg)
    full = [torch.empty((N + PAD, w), device=dev) for w in (S, A, S, 1, 1)]
    for t in full:
        _bits(t).fill_(-1)                                            # 0xFF bytes: a word nobody wrote is NaN
    b = tuple(t[:N] for t in full)
    ws = ops.train_workspace(dims, dev)
    _bits(ws).fill_(-1)
    st = {k: getattr(eng, k).clone() for k in ("actor", "actor_T", "q", "q_T", "qt", "qt_T", "mq", "vq")}
    loss = torch.zeros(1, device=dev)
    ctr = torch.tensor([7, 3, 11, 13], dtype=torch.int64, device=dev)  # call counter | the three words the gather advances
    gather = dict(buffers=[r[0] for r, _ in used], counts=[c for _, c in used], seeds=[101, 102, 103][:len(used)],
                  call_offsets=[1, 2, 3][:len(used)], counter=ctr[0:1], sizes=[r[1][1:2] for r, _ in used],
                  bump=(ctr[1:2], ctr[2:3], ctr[3:4]))
    kw = dict(t_dev=ctr[1:2], policy_forward=policy_forward, actor_blob_T=st["actor_T"], qtarg_blob_T=st["qt_T"], bump=ctr[0:1])
    if merged:
        kw["gather"] = gather
    else:
        ops.gather_batch_rng(S=S, A=A, out=b, **gather)
    ops.critic_update(dims, hyp, st["actor"], st["q"], st["q_T"], st["qt"], b, st["mq"], st["vq"], 0, cfg["critic_lr"], loss, ws, **kw)
    torch.cuda.synchronize()
    out = dict(st, ws=ws, loss=loss, ctr=ctr)
    out.update({"batch%d" % k: t for k, t in enumerate(full)})
    return out


def _same(ref, got, what):
    for k in ref:
        assert torch.equal(_bits(ref[k]) if ref[k].dtype == torch.float32 else ref[k],
                           _bits(got[k]) if got[k].dtype == torch.float32 else got[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("S,A", SHAPES)
def test_merged_launch_bitwise(mfma, S, A):
    for N in ROWS:
        for Nt in sorted({0, N // 2, N}):
            for pf in (True, False):
                what = (N, Nt, pf)
                ref = _critic_call(S, A, mfma, N, Nt, pf, merged=False)
                got = _critic_call(S, A, mfma, N, Nt, pf, merged=True)
                _same(ref, got, what)                                  # minibatch, workspace, blobs, moments, loss, counters
                for k in range(5):
                    t = got["batch%d" % k]
                    assert not torch.isnan(t[:N]).any(), (what, k)     # every row written ...
                    assert (_bits(t[N:]) == -1).all(), (what, k)       # ... and none past them
                assert got["ctr"].tolist() == [8, 4, 12, 14], what     # the optimizer launch advanced [0], the gather the rest


@pytest.mark.gpu
@pytest.mark.parametrize("S,A", SHAPES)
def test_merged_launch_repeats(mfma, S, A):
    """Ten merged launches of the largest case: identical bits (no tile depends on which workgroup got there first)."""
    N = max(ROWS)
    first = _critic_call(S, A, mfma, N, N // 2, True, merged=True)
    for rep in range(9):
        _same(first, _critic_call(S, A, mfma, N, N // 2, True, merged=True), rep)
