"""The chained actor backward (csrc/mlp_bwd.hip k_actor_bwd_chain): the frozen twin-Q input-gradient pass and the actor's own
backward in one launch, handed over tile by tile through a ticket word per 32-row tile.  What the hand-over can get wrong is
not arithmetic but ORDER and STATE, so every check here is bit for bit against the fp64 closed form of the exact probes
(actor_ref.int_probe / int_probe_expected; see tests/test_hip_actor_fp64.py part (a) for why those are exact in f32 and f16x2):

(i)   poisoned workspace: every byte of the workspace is 0xFF before the first launch that writes into it.  A ticket word nobody
      zeroed then never reads 1, the actor tile never runs and the NaN sentinels of the gradient blob stay; a dxa / bcw word read
      before its writer published it is NaN.  Either way the comparison fails -- nothing waits, so nothing can hang.
(ii)  repeated backward: two actor_backward calls after one actor_forward on the same workspace, a fresh NaN-filled gradient
      blob each time (the last arriver re-arms its ticket).
(iii) row counts 1, 33, 65, 257, 4097 = 1, 2, 3, 9, 129 tiles (all but one odd: a tile's two member workgroups then sit on different
      XCDs under round-robin dispatch), the Nt edge inside a tile and at a tile boundary, at the (S, A) that select the
      input-gradient instances NT = 1, 2 and 0.
(iv)  repeat identity: the largest case ten times on one workspace gives the same bits every time.
"""
import functools

import numpy as np
import pytest
import torch

import actor_ref as AR

ROWS = [(1, 0), (33, 32), (65, 33), (257, 129), (4097, 31)]
TILES = {1: 1, 33: 2, 65: 3, 257: 9, 4097: 129}
SA = [(11, 3), (17, 6), (111, 8)]
EXPECT_NT = {(11, 3): 1, (17, 6): 2, (111, 8): 0}
# (N, Nt), (S, A), N_global / pow2ceil(N), BC-weight variant, pi(s) rides with critic_step
CASES = [(n_nt, sa, 1 + (i + k) % 2, ("stats", "adv")[(i + k // 2) % 2], (i + k) % 2 == 1 and n_nt[0] > 1)
         for i, n_nt in enumerate(ROWS) for k, sa in enumerate(SA)]
LARGEST = next(c for c in CASES if c[0][0] == 4097 and c[1] == (111, 8))


def case_id(c):
    return f"N{c[0][0]}-Nt{c[0][1]}-S{c[1][0]}A{c[1][1]}-g{c[2]}-{c[3]}{'-ride' if c[4] else ''}"


@functools.lru_cache(maxsize=None)
def probe(c):
    """The probe and its fp64 closed form, computed once and shared by every test and both modes (read only)."""
    (N, Nt), (S, A), gmul, variant, _ = c
    p = AR.int_probe(S, A, N, Nt, gmul, 100 + N + 7 * S + gmul, variant)
    return p, AR.int_probe_expected(p)


def test_case_table_is_exact_and_complete():
    """CPU only: every case of the table meets the precondition of bit equality -- fp32 sums and the fp16 split of the f16x2 mode --
    and the table has what the module claims."""
    assert len(CASES) == len(ROWS) * len(SA) == len(set(CASES))
    for n_nt in ROWS:
        assert {c[1] for c in CASES if c[0] == n_nt} == set(SA)
    assert {AR.bwd_dx_nt(*sa) for sa in SA} == {0, 1, 2}
    for sa, nt in EXPECT_NT.items():
        assert AR.bwd_dx_nt(*sa) == nt
    assert [-(-n // 32) for n, _ in ROWS] == [TILES[n] for n, _ in ROWS] == [1, 2, 3, 9, 129]
    assert {AR.nt_place(*r) for r in ROWS} == {"none", "tile_edge", "inside_tile"}
    assert {c[4] for c in CASES} == {False, True} and {c[2] for c in CASES} == {1, 2} and {c[3] for c in CASES} == {"stats", "adv"}
    for c in CASES:
        _, (exp, ok, detail) = probe(c)
        assert ok, f"{case_id(c)}: precondition of bit equality fails: {detail}"
        assert AR.f16_bits_ok(probe(c)[0], exp), f"{case_id(c)}: an fp16-core operand needs more than 11 bits below its tile maximum"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Run:
    """pack -> transposes -> workspace with every byte 0xFF -> forward(); backward() may then be called any number of times, each
    with a fresh NaN-filled gradient blob and loss.  The pattern of test_hip_actor_fp64.run_actor, split at the backward."""

    def __init__(self, c, mode, dev):
        from mobody_amd import _lib, ops, packing
        self.ops, self.packing, self.dev = ops, packing, dev
        p = self.p = probe(c)[0]
        S, A = self.S, self.A = p["s"].shape[1], p["act"].shape[1]
        cfg = dict(gamma=0.99, tau=0.005, mfma=mode, **{k: p["h"][k] for k in ("max_action", "weight", "bc_coef", "q_weighted", "scale_Q")})
        self.actor = packing.pack_mlp([{k[len("network."):]: v for k, v in p["pa"].items()}], S, A, dev)
        self.q = packing.pack_mlp(p["pq"], S + A, 1, dev, prefixes=["network1.", "network2."])
        self.actor_T = ops.mlp_transpose(self.actor, S, A, 1, precision=mode)
        self.q_T = ops.mlp_transpose(self.q, S + A, 1, 2, precision=mode)
        self.dims, self.hyp = ops.train_dims(S, A, p["N"], p["Nt"], p["Ng"], p["Ntg"]), ops.hyper(cfg)
        self.ws = ops.train_workspace(self.dims, dev)
        self.ws.view(torch.uint8).fill_(0xFF)                   # before the first launch that writes into it
        self.s, self.a = torch.from_numpy(p["s"]).to(dev).contiguous(), torch.from_numpy(p["act"]).to(dev).contiguous()
        self.L = _lib.mlp_layout(S, A, 1)
        self.ride = c[4]

    def nan(self, n):
        return torch.full((n,), float("nan"), device=self.dev)

    def forward(self):
        ops, p = self.ops, self.p
        stats = self.nan(2)
        if self.ride:
            z = torch.zeros(p["N"], 1, device=self.dev)
            ops.critic_step(self.dims, self.hyp, self.actor, self.q, self.q_T, self.q.clone(), (self.s, self.a, self.s, z, z),
                            torch.empty_like(self.q), self.nan(1), self.ws, policy_forward=True, actor_blob_T=self.actor_T,
                            qtarg_blob_T=self.q_T.clone())
        ops.actor_forward(self.dims, self.hyp, self.actor, self.q, self.s, self.a, stats, self.ws, policy_ready=self.ride,
                          actor_blob_T=self.actor_T, q_blob_T=self.q_T)
        self.handed = torch.tensor(p["stats_in"], dtype=torch.float32, device=self.dev)
        self.v_true = torch.from_numpy(p["v_true"]).to(self.dev) if p["v_true"] is not None else None
        return stats

    def backward(self):
        """-> (gradient blob, loss_out[0:2]) on the device"""
        grad, loss = self.nan(self.L.total_floats), self.nan(2)
        self.ops.actor_backward(self.dims, self.hyp, self.actor, self.actor_T, self.q, self.q_T, self.s, self.a, self.handed, grad,
                                loss, self.ws, v_true=self.v_true)
        return grad, loss

    def tensors(self, grad):
        return {"network." + k: v.cpu().numpy() for k, v in self.packing.unpack_mlp(grad, self.S, self.A, 1)[0].items()}


def same_bits(got, want, what):
    """Bit equality of fp32 `got` with the fp64 `want` rounded once (a zero's sign is not a bit of the sum: +0 + -0)."""
    got = np.asarray(got, np.float32) + np.float32(0)
    want = np.asarray(want, np.float64).astype(np.float32) + np.float32(0)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first {i}: got {got[i]!r} want {want[i]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_poisoned_workspace_then_repeated_backward(case, mfma, dev):
    (N, Nt), (S, A) = case[0], case[1]
    assert AR.bwd_dx_nt(S, A) == EXPECT_NT[(S, A)] and -(-N // 32) == TILES[N]
    exp, ok, detail = probe(case)[1]
    assert ok, detail
    cf = exp["cf"]
    r = Run(case, mfma, dev)
    stats = r.forward()
    outs = [r.backward(), r.backward()]                         # (i) the first call on the poisoned workspace, (ii) the second
    torch.cuda.synchronize()
    same_bits(stats.cpu().numpy(), cf["stats"], "stats of actor_forward")
    for call, (grad, loss) in enumerate(outs):
        what = f"{case_id(case)} {mfma} backward {call + 1}"
        nbad = int((~torch.isfinite(grad)).sum())
        assert nbad == 0, f"{what}: {nbad} entries of the gradient blob unwritten / non-finite"
        g = r.tensors(grad)
        for k, v in exp["grads"].items():
            same_bits(g[k], v, f"{what} {k}")
        same_bits(loss.cpu().numpy(), [cf["L_pi"], cf["L_BC"]], f"{what} loss_out[0:2]")


@pytest.mark.gpu
def test_repeat_identity_largest_case(mfma, dev):
    exp, ok, detail = probe(LARGEST)[1]
    assert ok, detail
    r = Run(LARGEST, mfma, dev)
    r.forward()
    outs = [r.backward() for _ in range(10)]
    torch.cuda.synchronize()
    g0, l0 = outs[0]
    for k, v in exp["grads"].items():
        same_bits(r.tensors(g0)[k], v, f"{case_id(LARGEST)} {mfma} launch 1 {k}")
    for n, (g, l) in enumerate(outs[1:], 2):
        assert torch.equal(g.view(torch.int32), g0.view(torch.int32)), f"launch {n}: gradient bits differ from launch 1"
        assert torch.equal(l.view(torch.int32), l0.view(torch.int32)), f"launch {n}: loss bits differ from launch 1"
