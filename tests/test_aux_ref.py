"""The fp64 references of tests/aux_ref.py against torch.autograd in float64 on the reference project's own formulation
(F.cross_entropy applied to Softmax outputs, the expectile loss, a three-layer ReLU MLP), so that the GPU tests are not
compared with a reference that is itself wrong.  Also the preconditions of the exact-integer sweep and its case table.
No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_ref as R

RTOL = 1e-12


def close(got, want, what, atol=0.0):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(want, np.float64), rtol=RTOL, atol=atol, err_msg=what)


@pytest.mark.parametrize("in_dim,out_dim,members,rows", [(17, 1, 1, 37), (29, 2, 1, 64), (23, 6, 2, 33), (7, 3, 7, 9)])
def test_mlp3_backward_ref_vs_autograd(in_dim, out_dim, members, rows):
    rng = np.random.default_rng(in_dim)
    torch.manual_seed(in_dim)
    x = rng.standard_normal((rows, in_dim))
    G = rng.standard_normal((members, rows, out_dim))
    Ws, h1s, h2s, want = [], [], [], []
    for m in range(members):
        net = torch.nn.Sequential(torch.nn.Linear(in_dim, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                                  torch.nn.Linear(256, out_dim)).double()                   # MLPNetwork, mobody.py:35-48
        xt = torch.from_numpy(x)
        h1 = net[1](net[0](xt)); h2 = net[3](net[2](h1)); z3 = net[4](h2)
        (z3 * torch.from_numpy(G[m])).sum().backward()                                    # dL/dz3 = G
        Ws.append([net[i].weight.detach().numpy() for i in (0, 2, 4)])
        h1s.append(h1.detach().numpy()); h2s.append(h2.detach().numpy())
        want.append({"dW1": net[0].weight.grad, "db1": net[0].bias.grad, "dW2": net[2].weight.grad, "db2": net[2].bias.grad,
                     "dW3": net[4].weight.grad, "db3": net[4].bias.grad})
    W1, W2, W3 = (np.stack([w[i] for w in Ws]) for i in range(3))
    ref = R.mlp3_backward_ref(W1, W2, W3, x, np.stack(h1s), np.stack(h2s), G)
    for m in range(members):
        for k, w in want[m].items():
            # rtol alone, except for entries that cancel: two fp64 evaluations of one contraction in different summation
            # orders (through dz2 and dz1: three nested ones) differ by up to ~K * 2^-53 of its sum |a||b|, whatever the result
            close(ref[k][m], w.numpy(), f"{k}[{m}]", atol=3 * 256 * 2.0 ** -53 * ref["abs_" + k][m].max())
            assert (ref["abs_" + k][m] >= np.abs(ref[k][m]) * (1 - 1e-12)).all()
    # the companions are the same contractions over absolute values
    a = R.mlp3_backward_ref(np.abs(W1), np.abs(W2), np.abs(W3), np.abs(x), np.abs(np.stack(h1s)), np.abs(np.stack(h2s)), np.abs(G))
    for k in ("dW3", "db3"):
        close(ref["abs_" + k], a[k], "abs_" + k)


LOGITS = {"random": lambda rng, n: 3.0 * rng.standard_normal((n, 2)),
          "saturated": lambda rng, n: np.where(rng.random((n, 1)) < 0.5, [[80.0, -80.0]], [[-80.0, 80.0]]),
          "equal": lambda rng, n: np.repeat(rng.standard_normal((n, 1)), 2, 1),
          "huge": lambda rng, n: np.full((n, 2), 1e4),
          "huge_apart": lambda rng, n: np.tile([1e4, 1e4 - 3.0], (n, 1))}


@pytest.mark.parametrize("kind", list(LOGITS))
@pytest.mark.parametrize("n", [1, 5, 257])
def test_double_softmax_ce_ref_vs_autograd(kind, n):
    rng = np.random.default_rng(n)
    z = LOGITS[kind](rng, n).astype(np.float64)
    lab = rng.integers(0, 2, n)
    zt = torch.tensor(z, requires_grad=True)
    loss = F.cross_entropy(torch.softmax(zt, dim=1), torch.from_numpy(lab))      # Classifier.forward + update_classifier :25, :169
    loss.backward()
    got_l, got_dz, rows = R.double_softmax_ce_ref(z, lab)
    close(got_l, loss.item(), "loss")
    # autograd forms p_i (g_i - sum_j g_j p_j) / n, which cancels when p_i -> 1: its own fp64 rounding is a few 2^-53 of
    # p_i |g| / n <= 1 / n absolutely, whatever the size of the result.  That floor is torch's, not the closed form's.
    close(got_dz, zt.grad.numpy(), "dL/dz", atol=2.0 ** -50 / n)
    close(rows.mean(), loss.item(), "row losses")
    l_sa, l_sas, d_sas, d_sa = R.dara_loss_grad_ref(z, z[::-1].copy(), lab)
    assert l_sas == got_l and np.array_equal(d_sas, got_dz) and d_sa.shape == (n, 2)


def test_dara_penalty_ref_vs_torch():
    rng = np.random.default_rng(0)
    z_sas = np.concatenate([f(rng, 40) for f in LOGITS.values()])
    z_sa = np.concatenate([f(rng, 40) for f in reversed(list(LOGITS.values()))])
    sas = torch.softmax(torch.softmax(torch.tensor(z_sas), 1), 1)                # Softmax head, then F.softmax: mobody.py:373-374
    sa = torch.softmax(torch.softmax(torch.tensor(z_sa), 1), 1)
    ls, la = torch.log(sas + 1e-10), torch.log(sa + 1e-10)
    want = (ls[:, 1:] - la[:, 1:] - ls[:, :1] + la[:, :1]).clamp(-10, 10)          # :375-378
    got, raw = R.dara_penalty_ref(z_sas, z_sa)
    close(got, want.numpy()[:, 0], "delta", atol=1e-15)
    assert np.abs(raw).max() <= 2.0 and np.array_equal(got, raw)                 # the clamp cannot bind


@pytest.mark.parametrize("mult", [1, 3])
def test_value_loss_ref_vs_autograd(mult):
    rng = np.random.default_rng(1)
    N = 300
    qt = 5.0 * rng.standard_normal((2, N))
    v = qt.min(0) + rng.standard_normal(N)
    v[::7] = qt.min(0)[::7]                              # the kink
    vt = torch.tensor(v, requires_grad=True)
    adv = torch.min(torch.tensor(qt[0]), torch.tensor(qt[1])) - vt                # update_v_function, mobody.py:233-237
    loss = torch.mean(torch.abs(0.7 - (adv < 0).double()) * adv ** 2) / mult      # asymmetric_l2_loss(adv, 0.7), :85-86, :241
    loss.backward()
    got_l, got_dv = R.value_loss_ref(qt, v, mult * N)
    assert R.EXPECTILE == 0.7
    # (the indicator as float64: with the reference's .float() torch would round the 0.7 itself to fp32)
    close(got_l, loss.item(), "V loss")
    close(got_dv, vt.grad.numpy(), "dL/dV")
    assert (got_dv[::7] == 0).all()


def test_par_penalty_ref_vs_torch():
    rng = np.random.default_rng(2)
    t, m, r = rng.standard_normal((50, 17)), rng.standard_normal((50, 17)), rng.standard_normal((50, 1))
    want = torch.tensor(r) - 0.1 * torch.mean((torch.tensor(t) - torch.tensor(m)) ** 2, axis=1, keepdims=True)   # mobody.py:431-434
    got, mse = R.par_penalty_ref(t, m, r, 0.1)
    close(got, want.numpy()[:, 0], "reward")


def test_wgrad_geometry_matches_the_launch_formulas():
    g = R.wgrad_geometry(65, 1)                         # rows_per_wave 17 -> 32: 32 + 32 + 1 + 0
    assert g["nsplit"] == 1 and g["rows_per_wave"] == 32 and [w[0] for w in g["waves"]] == [32, 32, 1, 0]
    g = R.wgrad_geometry(4097, 1)
    assert g["nsplit"] == 32 and g["rows_per_wave"] == 48 and sum(w[0] > 0 for w in g["waves"]) == 86
    assert R.wgrad_geometry(280, 1)["waves"][5] == (40, 5, 0)
    assert [R.wgrad_nsplit(r, 1) for r in (127, 128, 255, 256, 383, 384, 4095, 4096, 10240)] == [1, 1, 1, 2, 2, 3, 31, 32, 32]
    assert [R.wgrad_nsplit(r, 2) for r in (511, 512, 768, 4096, 10240)] == [1, 2, 3, 16, 16]
    assert [R.wgrad_nsplit(r, 7) for r in (1023, 1024, 1280, 10240, 40960)] == [3, 4, 4, 4, 8]
    for rows in (1, 33, 257, 4097, 10240):
        for members in (1, 2, 7):
            g = R.wgrad_geometry(rows, members)
            assert sum(w[0] for w in g["waves"]) == rows and g["rows_per_wave"] % 16 == 0


def test_case_table_of_the_exact_sweep():
    import test_hip_aux_grad as G
    G.check_case_table()


@pytest.mark.parametrize("kind,sa", [("mopo", (111, 8)), ("twin_q", (111, 8)), ("cls_sas", (111, 8)), ("actor", (45, 24)),
                                      ("mopo", (45, 24))])
def test_integer_generators_stay_exact_at_the_largest_case(kind, sa):
    import test_hip_aux_grad as G
    in_dim, out_dim, members = G.KINDS[kind](*sa)
    rows = max(c[2] for c in G.CASES)
    assert rows == 10240
    c = R.int_case(1000 + rows + 7 * in_dim, in_dim, out_dim, members, rows)
    ref = R.mlp3_backward_ref(c["W1"], c["W2"], c["W3"], c["x"], c["h1"], c["h2"], c["dz3"])
    worst, ok = R.int_exact_ok(ref)
    assert ok and worst < 2.0 ** 22, worst             # two bits of room below the 2^24 the bit equality needs
    assert (c["h1"] <= 0).any() and np.abs(ref["dW1"]).max() > 0 and set(np.unique(c["W2"])) == {-1.0, 0.0, 1.0}
