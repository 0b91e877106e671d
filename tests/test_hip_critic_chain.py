"""The critic backward chained onto the merged critic forward (csrc/critic_fwd_bf.hip k_critic_chain_bf): where mobody_critic with a
`gather` block takes the one-chain form of the merged forward launch (f16x2, more than 102 row tiles), the workgroup that finishes
a (row tile, member)'s forward rows last runs that tile's backward in the same launch, and the separate k_mlp3_bwd launch is gone.

Everything is bit-for-bit against the plain launches -- mobody_gather_batch_rng, then mobody_critic without `gather`: the same
draws, the same arithmetic per output element, so there is no tolerance.  The workspace is 0xFF before the first call: a word the
launch should have published and did not is NaN in the seed, and every ticket starts from bytes no launch wrote.  Each case calls
the same entry three times on the same state, workspace and tickets: twice at one value of the draw counter (the ticket epoch),
then once with it advanced.  Sizes on both sides of the size rule (3264 | 3265 rows) and at the row-tile edges; below the rule,
in f32 and at (45, 24) the step keeps its separate backward launch and must agree all the same.  Nothing here steers which
producer of a ticket arrives last: both orders occur across these sizes.

Figures (MI355X): see DESIGN 5z."""
import functools

import pytest
import torch

import golden_util as gu
from mobody_amd import ops

SHAPES = [(17, 6), (11, 3), (23, 17)]            # (23, 17): an actor output layer of 32 columns in the chained launch
ROWS = [1, 31, 32, 33, 65, 257, 3264, 3265, 4097]  # row-tile edges; 102 | 103 tiles: the last launch without, the first with the backward tiles
RING_ROWS = (1000, 7, 300)                       # src | tar | fake, of different sizes
PAD = 5                                          # sentinel rows behind the minibatch arrays
IDLE = -1                                        # a ticket no producer is waiting on (0xFFFFFFFF)


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _rings(S, A):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3000 * S + A)
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
    return engine.Engine(S, A, pa, pq, torch.device("cuda:0"))        # built under MOBODY_MFMA = mfma (the caller set it)


def _ticket_slice(N, ws):
    """The ticket words of the chained launch: two per 32-row tile, at the head of the workspace's last piece (four words per tile,
    rounded up to four: csrc/train.hip carve)."""
    tiles = -(-N // 32)
    start = ws.numel() - ((4 * tiles + 3) & ~3)
    return slice(start, start + 2 * tiles)


def _critic_calls(S, A, mfma, N, Nt, policy_forward, chained, calls=3):
    """`calls` critic updates in a row on one state, workspace and counter block; a snapshot of every tensor they can have written
    after each.  The optimizer launch advances the draw counter in the second call only."""
    dev = torch.device("cuda:0")
    eng = _nets(S, A, mfma)
    cfg = gu.policy_cfg(S, A, mfma=mfma)
    counts = (Nt - Nt // 2, Nt // 2, N - Nt)
    used = [(r, c) for r, c in zip(_rings(S, A), counts) if c > 0]
    dims, hyp = ops.train_dims(S, A, N, Nt), ops.hyper(cfg)
    full = [torch.empty((N + PAD, w), device=dev) for w in (S, A, S, 1, 1)]
    for t in full:
        _bits(t).fill_(-1)                                            # 0xFF bytes: a word nobody wrote is NaN
    b = tuple(t[:N] for t in full)
    ws = ops.train_workspace(dims, dev)
    _bits(ws).fill_(-1)
    st = {k: getattr(eng, k).clone() for k in ("actor", "actor_T", "q", "q_T", "qt", "qt_T", "mq", "vq")}
    loss = torch.zeros(1, device=dev)
    ctr = torch.tensor([7, 3, 11, 13], dtype=torch.int64, device=dev)  # draw counter | the three words the gather advances
    gather = dict(buffers=[r[0] for r, _ in used], counts=[c for _, c in used], seeds=[101, 102, 103][:len(used)],
                  call_offsets=[1, 2, 3][:len(used)], counter=ctr[0:1], sizes=[r[1][1:2] for r, _ in used],
                  bump=(ctr[1:2], ctr[2:3], ctr[3:4]))
    snaps = []
    for k in range(calls):
        kw = dict(t_dev=ctr[1:2], policy_forward=policy_forward, actor_blob_T=st["actor_T"], qtarg_blob_T=st["qt_T"],
                  bump=ctr[0:1] if k == 1 else None)
        if chained:
            kw["gather"] = gather
        else:
            ops.gather_batch_rng(S=S, A=A, out=b, **gather)
        ops.critic_update(dims, hyp, st["actor"], st["q"], st["q_T"], st["qt"], b, st["mq"], st["vq"], 0, cfg["critic_lr"], loss, ws, **kw)
        torch.cuda.synchronize()
        out = dict(st, ws=ws, loss=loss, ctr=ctr)
        out.update({"batch%d" % j: t for j, t in enumerate(full)})
        snaps.append({key: t.clone() for key, t in out.items()})
    return snaps


def _same(ref, got, N, what, tickets_idle):
    tk = _ticket_slice(N, ref["ws"])
    for k in ref:
        r = _bits(ref[k]) if ref[k].dtype == torch.float32 else ref[k]
        g = _bits(got[k]) if got[k].dtype == torch.float32 else got[k]
        if k == "ws":                                                  # the whole workspace except the ticket words
            assert torch.equal(r[:tk.start], g[:tk.start]), (what, k, "in front of the tickets")
            assert torch.equal(r[tk.stop:], g[tk.stop:]), (what, k, "behind the tickets")
            if tickets_idle:                                           # every ticket was completed: none is left at "one arrived"
                assert (g[tk] == IDLE).all(), (what, "a ticket is not idle after the launch")
        else:
            assert torch.equal(r, g), (what, k)


def _check(S, A, mfma, rows, nts=lambda N: (0, N), pfs=(True, False)):
    for N in rows:
        for Nt in nts(N):
            for pf in pfs:
                ref = _critic_calls(S, A, mfma, N, Nt, pf, chained=False)
                got = _critic_calls(S, A, mfma, N, Nt, pf, chained=True)
                for call, (r, g) in enumerate(zip(ref, got)):
                    what = (N, Nt, pf, call)
                    _same(r, g, N, what, tickets_idle=True)
                    for k in range(5):
                        t = g["batch%d" % k]
                        assert not torch.isnan(t[:N]).any(), (what, k)     # every row written ...
                        assert (_bits(t[N:]) == -1).all(), (what, k)       # ... and none past them
                    assert not torch.isnan(g["loss"]).any(), what
                # the second call's optimizer launch advanced the draw counter, every call's gather the other three words
                assert [s["ctr"].tolist() for s in got] == [[7, 4, 12, 14], [8, 5, 13, 15], [8, 6, 14, 16]], (N, Nt, pf)


@pytest.mark.gpu
@pytest.mark.parametrize("S,A", SHAPES)
def test_chained_launch_bitwise(monkeypatch, S, A):
    monkeypatch.setenv("MOBODY_MFMA", "f16x2")
    _check(S, A, "f16x2", ROWS)


@pytest.mark.gpu
def test_f32_keeps_its_separate_backward(monkeypatch):
    """Exact fp32 has no merged forward launch: the gathering entry runs the plain backward launch and agrees with it."""
    monkeypatch.setenv("MOBODY_MFMA", "f32")
    _check(17, 6, "f32", [33, 3265, 4097])


@pytest.mark.gpu
def test_wide_rows_keep_their_separate_backward(monkeypatch):
    """(45, 24): a tile's [s' | a'] rows do not fit behind the image, the step stays on its launches -- same bits."""
    monkeypatch.setenv("MOBODY_MFMA", "f16x2")
    _check(45, 24, "f16x2", [33, 3265, 4097])


@pytest.mark.gpu
def test_chained_launch_repeats(monkeypatch):
    """Ten chained launches of the largest case: identical bits, whichever producer of a ticket got there last."""
    monkeypatch.setenv("MOBODY_MFMA", "f16x2")
    N = max(ROWS)
    first = _critic_calls(17, 6, "f16x2", N, N, True, chained=True, calls=1)[0]
    for rep in range(9):
        again = _critic_calls(17, 6, "f16x2", N, N, True, chained=True, calls=1)[0]
        _same(first, again, N, rep, tickets_idle=True)
