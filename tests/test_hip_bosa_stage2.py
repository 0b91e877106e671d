"""GPU checks of the critic seed with a conservative term (seed mode 9, mobody_bosa_critic; csrc/mlp_bwd.hip) in exact
fp32 against an fp64 autograd evaluation of the same loss,

    mean_rows(w (q1 - y)^2) + mean_rows(w (q2 - y)^2) + sum_rows c (q1 + q2),        y = r + not_done * gamma * q_next,

whose derivative with respect to q_m is the seed 2 w (q_m - y) / N + c.  Tolerances: losses rtol 1e-5, gradients rtol 1e-5 / atol
1e-5 x the largest gradient entry (tests/test_hip_igdf.py's, for mode 8).  rows = 33 and 257 are one row past one and past eight
32-row tiles.  With c all zero the seed and every gradient carry mode 8's bits (mobody_igdf_critic on the same rows); the loss is
the same sum divided by N where mode 8 multiplies by the rounded 1 / N, so it may differ in the last place.
tests/test_bosa2_ref.py holds the precondition of the normalised tolerance: a float32 evaluation of tests/bosa2_ref.critic_step on
these inputs stays within half of it (measured 0.009 to 0.083).  The fp64 reference is that restatement, checked here against torch
autograd of the loss above.  bosa2_ref.MODE9_EDGE_CASES adds the row edges at walker shapes -- N = 2 (one target and one source row),
32, 64, the product's 256, 1024 and 1025 -- and N = 65 at (S, A) = (11, 3), (45, 24) and (111, 8), with the same check; their float32
precondition is tests/test_bosa_actor_ref.py's.  The c = 0 and the fused-form checks also run at 256 rows.

The split-precision instances of the kernel run once each against the same fp64 reference at the bounds the project already holds
those modes to: f16x2 and bf16x3 (fp32-grade) at the exact-fp32 tolerance, as every `mfma`-parametrised suite does
(tests/test_hip_igdf.py::test_weighted_critic_vs_fp64_and_null_weight for mode 8); bf16x2 and bf16 at
tests/test_hip_precision.py::test_train_step_lower_modes_vs_oracle's: the loss within tol, gradients within 10 tol x the largest
entry, tol = 2e-4 and 5e-2.  f16x2 and bf16x3 run again at 256 rows and at pen's widths with 65 rows, at the exact-fp32 tolerance.
"""
import numpy as np
import pytest
import torch

import bosa2_ref as B2
import golden_util as gu
import igdf_ref as GR
import iql_ref as IR
from test_hip_igdf import WStep
from test_hip_iql import Net, hyper_of, to_dev
from test_hip_train import close

pytestmark = pytest.mark.gpu
NAN = float("nan")
S, A, MODE = B2.MODE9_S, B2.MODE9_A, "f32"
COEF = B2.MODE9_COEF


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Critic:
    """The twin-Q net on the device and one mobody_bosa_critic call in either form."""

    def __init__(self, pq, N, dev, gamma=0.99, mode=MODE, SA=(S, A)):
        from mobody_amd import ops
        S, A = SA
        self.q = Net(pq, S + A, 1, 2, dev, mode)
        self.q.gbuf = torch.full((self.q.blob.numel() + 1,), NAN, device=dev)
        self.q.grad = self.q.gbuf[:-1]
        self.dims = ops.train_dims(S, A, N, N)
        self.hyp = hyper_of(dict(gamma=gamma, tau=0.005, max_action=1.0), mode)
        self.ws = ops.train_workspace(self.dims, dev)
        self.loss = torch.full((3,), NAN, device=dev)

    def run(self, b, q_next, w, c, cons_rows, **opt):
        from mobody_amd import ops
        kw = opt or dict(grad_q=self.q.grad)
        ops.bosa_critic(self.dims, self.hyp, self.q.blob, self.q.blob_T, b, q_next, w, c, COEF, cons_rows, self.loss[:2], self.ws, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.loss[2])) and bool(torch.isnan(self.q.gbuf[-1]))
        return self.loss[:2].cpu().numpy()


def case(N, dev, seed=501, SA=(S, A)):
    return B2.mode9_case(N, gu.gi.batch(seed, max(N, 64), *SA))


def restated(pq, rows, q_next, w, c, gamma=0.99):
    """(critic_loss, cons_loss, {state-dict name: gradient}) of tests/bosa2_ref.critic_step in fp64."""
    s, a, _, r, nd = rows
    y = np.asarray(r, np.float64).reshape(-1) + np.asarray(nd, np.float64).reshape(-1) * gamma * q_next.astype(np.float64)
    logs, seed, g = B2.critic_step(B2.twin_from_state_dict(pq), s, a, y, 2.0 * w, COEF, c=c)      # the float32 c the kernel reads
    assert c[len(c) // 2] == np.float32(COEF / (len(c) - len(c) // 2)) and not c[:len(c) // 2].any()
    return logs["critic_loss"], logs["critic_cons_loss"], B2.to_state_dict(g)


def fp64(pq, rows, q_next, w, c, gamma=0.99):
    """(critic_loss, cons_loss, {name: gradient}) by autograd in fp64."""
    q64 = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in pq.items()}
    s, ac, s2, r, nd = [torch.tensor(np.asarray(x, np.float64)) for x in rows]

    def mlp(pre, x):
        h = torch.relu(x @ q64[pre + "network.0.weight"].T + q64[pre + "network.0.bias"])
        h = torch.relu(h @ q64[pre + "network.2.weight"].T + q64[pre + "network.2.bias"])
        return h @ q64[pre + "network.4.weight"].T + q64[pre + "network.4.bias"]
    y = r + nd * gamma * torch.tensor(q_next.astype(np.float64)).reshape(-1, 1)
    x = torch.cat([s, ac], 1)
    q1, q2 = mlp("network1.", x), mlp("network2.", x)
    wt, ct = (torch.tensor(t.astype(np.float64)).reshape(-1, 1) for t in (w, c))
    td = (wt * (q1 - y) ** 2).mean() + (wt * (q2 - y) ** 2).mean()
    src = ct[:, 0] != 0
    n_src = max(int(src.sum()), 1)
    cons = (q1[src].sum() + q2[src].sum()) / n_src
    loss = td + (ct * (q1 + q2)).sum()
    g = torch.autograd.grad(loss, list(q64.values()))
    return float((td + COEF * cons).detach()), float(cons.detach()), dict(zip(q64, (t.numpy() for t in g)))


def check(cr, rows, q_next, w, c, pq, dev, tag):
    N = len(w)
    n_src = max(int((c != 0).sum()), 1)
    got = cr.run(to_dev(rows, dev), torch.as_tensor(q_next).to(dev), torch.as_tensor(w).to(dev), torch.as_tensor(c).to(dev), n_src)
    want_loss, want_cons, want = restated(pq, rows, q_next, w, c)
    auto = fp64(pq, rows, q_next, w, c)                          # the restatement is the loss's derivative: torch autograd agrees
    assert abs(auto[0] - want_loss) <= 1e-12 * abs(want_loss) and abs(auto[1] - want_cons) <= 1e-12 * abs(want_cons)
    for name, g64 in want.items():
        np.testing.assert_allclose(auto[2][name], g64, rtol=1e-9, atol=1e-12 * max(float(np.abs(v).max()) for v in want.values()))
    print("%s: critic_loss %.7g / %.7g, cons %.7g / %.7g" % (tag, got[0], want_loss, got[1], want_cons))
    close(float(got[0]), want_loss, rtol=1e-5, atol=0)
    close(float(got[1]), want_cons, rtol=1e-5, atol=0)
    grads = cr.q.unpack(cr.q.grad)
    scale = max(float(np.abs(v).max()) for v in want.values())
    for name, g64 in want.items():
        print("  %s: worst error / tolerance %.3f" % (name, (np.abs(grads[name] - g64) / (1e-5 * scale + 1e-5 * np.abs(g64))).max()))
        close(grads[name], g64, rtol=1e-5, atol=1e-5 * scale)
    return got, grads


@pytest.mark.parametrize("N", [33, 257])
def test_mode9_vs_fp64(N, dev):
    mode9_vs_fp64(N, (S, A), dev)


@pytest.mark.parametrize("c", B2.MODE9_EDGE_CASES, ids=lambda c: "N%d-s%da%d" % (c[0], c[1][0], c[1][1]))
def test_mode9_vs_fp64_at_row_edges_and_other_widths(c, dev):
    """B2.MODE9_EDGE_CASES: at (17, 6) the smallest N (one target and one source row), one and two exact 32-row tiles, the product's
    256, 1024 and one past it; at N = 65 a narrow net (11, 3), pen's A = 24 and ant's S = 111.  tests/test_bosa_actor_ref.py holds
    the float32 precondition of each."""
    mode9_vs_fp64(c[0], c[1], dev)


def mode9_vs_fp64(N, SA, dev):
    pq = B2.mode9_params(SA)
    rows, q_next, w, c = case(N, dev, SA=SA)
    assert 0 < (w != 0).sum() < N and (c[:N // 2] == 0).all() and (c[N // 2:] != 0).all()
    check(Critic(pq, N, dev, SA=SA), rows, q_next, w, c, pq, dev, "mixed N=%d (S, A)=%s" % (N, SA))
    # no row passes the mask: the only gradient is the conservative term's, the TD part of the loss is exactly 0
    got, grads = check(Critic(pq, N, dev, SA=SA), rows, q_next, np.zeros_like(w), c, pq, dev, "w = 0, N=%d (S, A)=%s" % (N, SA))
    assert np.float32(got[0]) == np.float32(COEF) * np.float32(got[1]) and any(np.abs(g).max() > 0 for g in grads.values())


@pytest.mark.parametrize("mode,tol", [("f16x2", None), ("bf16x3", None), ("bf16x2", 2e-4), ("bf16", 5e-2)])
def test_mode9_split_precision_instances(mode, tol, dev):
    """k_mlp3_bwd_ccritic<1..4> (and the forward / weight-gradient kernels of the mode) on the 257-row case."""
    split_precision_instance(mode, tol, 257, (S, A), dev)


@pytest.mark.parametrize("c", [(256, (S, A)), (65, (45, 24))], ids=lambda c: "N%d-s%da%d" % (c[0], c[1][0], c[1][1]))
@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_mode9_fp32_grade_split_modes_at_the_product_rows_and_pen(mode, c, dev):
    """The two fp32-grade split modes at the exact-fp32 tolerance on 256 rows (eight exact tiles) and at pen's widths."""
    split_precision_instance(mode, None, c[0], c[1], dev)


def split_precision_instance(mode, tol, N, SA, dev):
    pq = B2.mode9_params(SA)
    rows, q_next, w, c = case(N, dev, SA=SA)
    cr = Critic(pq, N, dev, mode=mode, SA=SA)
    got = cr.run(to_dev(rows, dev), *(torch.as_tensor(t).to(dev) for t in (q_next, w, c)), N - N // 2)
    want_loss, want_cons, want = restated(pq, rows, q_next, w, c)
    grads = cr.q.unpack(cr.q.grad)
    scale = max(float(np.abs(v).max()) for v in want.values())
    worst = max(float(np.abs(grads[k] - want[k]).max()) for k in want) / scale
    print("%s N=%d (S, A)=%s: critic_loss %.7g / %.7g, cons %.7g / %.7g, worst gradient error / largest entry %.3g" %
          (mode, N, SA, got[0], want_loss, got[1], want_cons, worst))
    if tol is None:
        close(float(got[0]), want_loss, rtol=1e-5, atol=0)
        close(float(got[1]), want_cons, rtol=1e-5, atol=0)
        for name, g64 in want.items():
            close(grads[name], g64, rtol=1e-5, atol=1e-5 * scale)
    else:
        assert abs(float(got[0]) - want_loss) <= tol * abs(want_loss) and abs(float(got[1]) - want_cons) <= tol * abs(want_cons)
        assert worst <= 10 * tol


@pytest.mark.parametrize("N", [33, 257, 256])
def test_mode9_with_zero_constants_is_mode8_bit_for_bit(N, dev):
    """mobody_igdf_critic bootstraps from its own V(s'); with not_done = 0 both calls regress onto y = r whatever q_next holds."""
    from mobody_amd import ops
    pa, pq, pv = IR.iql_params(S, A, 431, 16.0)
    rows, q_next, w, _ = case(N, dev)
    w = (w + np.float32(0.25) * (np.arange(N) % 3 == 0)).astype(np.float32)        # a few weights, zeros among them
    rows[4] = np.zeros_like(rows[4])
    b, wd = to_dev(rows, dev), torch.as_tensor(w).to(dev)
    m8 = WStep(S, A, pa, pq, pv, dev, N, GR.igdf_cfg(S, A), MODE)
    m8.t = 1
    ops.igdf_critic(*m8.head(b), m8.loss[0:1], m8.ws, grad=m8.q.grad, row_weight=wd)
    cr = Critic(pq, N, dev, gamma=GR.igdf_cfg(S, A)["gamma"])
    got = cr.run(b, torch.as_tensor(q_next).to(dev), wd, torch.zeros(N, device=dev), 1)
    assert torch.equal(cr.q.grad.view(torch.int32), m8.q.grad.view(torch.int32))
    assert got[1] == 0 and abs(float(got[0]) - float(m8.loss[0])) <= 2 * np.spacing(np.float32(got[0]))
    assert m8.q.grad.abs().max() > 0


def test_fused_form_is_the_gradient_form_plus_adam_and_moves_no_target(dev):
    fused_is_gradient_plus_adam(257, dev)


def test_fused_form_is_the_gradient_form_plus_adam_at_the_product_rows(dev):
    fused_is_gradient_plus_adam(256, dev)


def fused_is_gradient_plus_adam(N, dev):
    _, pq, _ = IR.iql_params(S, A, 431, 16.0)
    rows, q_next, w, c = case(N, dev)
    b, args = to_dev(rows, dev), [torch.as_tensor(t).to(dev) for t in (q_next, w, c)]
    two, one = Critic(pq, N, dev), Critic(pq, N, dev)
    lr = 3e-4
    for t in (1, 2):
        la = two.run(b, *args, N - N // 2)
        two.q.adam(t, lr, MODE)
        lb = one.run(b, *args, N - N // 2, m=one.q.am, v=one.q.av, t=t, lr=lr)
        torch.cuda.synchronize()
        assert np.array_equal(la.view(np.int32), lb.view(np.int32))
        for x, y in ((two.q.blob, one.q.blob), (two.q.am, one.q.am), (two.q.av, one.q.av), (two.q.blob_T, one.q.blob_T)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_refusals(dev):
    from mobody_amd import _lib, ops
    N = 33
    _, pq, _ = IR.iql_params(S, A, 431, 16.0)
    rows, q_next, w, c = case(N, dev)
    cr = Critic(pq, N, dev)
    b, (qn, wd, cd) = to_dev(rows, dev), [torch.as_tensor(t).to(dev) for t in (q_next, w, c)]
    call = lambda *a, **kw: ops.bosa_critic(cr.dims, cr.hyp, cr.q.blob, cr.q.blob_T, b, *a, cr.loss[:2], cr.ws, **kw)
    with pytest.raises(_lib.MobodyError, match="q_next is NULL"):
        call(None, wd, cd, COEF, 16, grad_q=cr.q.grad)
    with pytest.raises(_lib.MobodyError, match="row_weight / row_const is NULL"):
        call(qn, wd, None, COEF, 16, grad_q=cr.q.grad)
    with pytest.raises(_lib.MobodyError, match="cons_rows_global 0"):
        call(qn, wd, cd, COEF, 0, grad_q=cr.q.grad)
    with pytest.raises(_lib.MobodyError, match="exactly one of grad_q"):
        call(qn, wd, cd, COEF, 16)
