"""GPU checks of the IGDF baseline: the C ABI against the g26 fixtures (the real reference's update_info and train()
steps), the row-wise kernels per element against fp64 at their edges, the row-weighted critic, and the mirror class.

Tolerances.  Against the fixtures: scores atol 1e-5, kept rows exact and in order, weights rtol 1e-5, batch rows bit-equal, info loss
rtol 1e-5, encoder gradients rtol 1e-5 / atol 1e-5 x the encoder's largest entry, parameters params_close at actor_lr, IQL's phases
as tests/test_hip_iql.py.  mobody_igdf_contrast against fp64, per element (u = 2^-24): a logit is a sequential fp32 dot product of Z
terms, E_l = Z u sum |phi psi|; sigma moves by at most sigma (1 - sigma) per unit of l, and expf (two units in the last place, 4 u),
1 + e, the division, the rounded 1 / n^2 and the product with it cost at most 12 u of it, so E_G = (s (1 - s) E_l + 12 u s) / n^2; a
gradient entry sums n such terms in fp32: sum E_G |psi| + (n + 2) u sum |G psi|; the loss terms move by at most sigma per unit of l,
expf and log1pf cost 12 u, the sum of the n^2 terms (n + 40) u of their total.
"""
import json
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import igdf_ref as GR
import iql_ref as IR
from test_hip_iql import FixedRows, Net, Step, to_dev
from test_hip_train import close, params_close

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Enc(Net):
    """One encoder on the device: blob, T blob, Adam moments, and a gradient blob with a sentinel float behind it."""

    def __init__(self, pe, pre, in_dim, Z, dev, mode):
        from mobody_amd import ops, packing
        self.dims, self.prefixes = (in_dim, Z, 1), [pre]
        self.blob = packing.pack_mlp(pe, in_dim, Z, dev, prefixes=[pre])
        self.blob_T = ops.mlp_transpose(self.blob, in_dim, Z, 1, precision=mode)
        self.am, self.av = torch.zeros_like(self.blob), torch.zeros_like(self.blob)
        self.gbuf = torch.full((self.blob.numel() + 1,), NAN, device=dev)
        self.grad = self.gbuf[:-1]


class Info:
    """mobody_igdf_info + mobody_igdf_filter on one pair of encoders, gradient form (+ mobody_adam_polyak) or fused form."""

    def __init__(self, S, A, Z, pe, dev, n, mode):
        from mobody_amd import ops
        self.sa, self.ss = Enc(pe, GR.ENCS[0], S + A, Z, dev, mode), Enc(pe, GR.ENCS[1], S, Z, dev, mode)
        self.S, self.A, self.Z, self.n, self.mode, self.dev = S, A, Z, n, mode, dev
        self.dims = ops.train_dims(S, A, n, n)
        self.ws = ops.igdf_workspace(self.dims, n, Z, dev)
        self.loss = torch.full((2,), NAN, device=dev)
        self.t = 0

    def step(self, b, lr, fused=False):
        from mobody_amd import ops
        self.t += 1
        head = (self.dims, self.mode, (self.sa, self.ss), self.n, self.Z, b, self.loss[:1], self.ws)
        if fused:
            ops.igdf_info(*head, opts=((self.sa.am, self.sa.av), (self.ss.am, self.ss.av)), t=self.t, lr=lr)
        else:
            ops.igdf_info(*head, grads=(self.sa.grad, self.ss.grad))
            self.sa.adam(self.t, lr, self.mode)
            self.ss.adam(self.t, lr, self.mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.loss[1])) and bool(torch.isnan(self.sa.gbuf[-1])) and bool(torch.isnan(self.ss.gbuf[-1]))

    def filter(self, staged, k, iw, ws, dims):
        """Returns (batch, w, score, kept), every output array with a NaN (or -1) sentinel behind it, checked."""
        from mobody_amd import ops
        S, A, n, dev = self.S, self.A, self.n, self.dev
        N = k + staged[0].shape[0] - n
        bufs = [torch.full((N * w + 1,), NAN, device=dev) for w in (S, A, S, 1, 1)]
        out = [b[:-1].view(N, w) for b, w in zip(bufs, (S, A, S, 1, 1))]
        wb, sb = torch.full((N + 1,), NAN, device=dev), torch.full((n + 1,), NAN, device=dev)
        kb = torch.full((k + 1,), -1, dtype=torch.int32, device=dev)
        ops.igdf_filter(dims, self.mode, (self.sa, self.ss), n, k, self.Z, iw, staged, out, wb[:-1], ws, score_out=sb[:-1], kept_out=kb[:-1])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b[-1])) for b in bufs + [wb, sb]) and int(kb[-1]) == -1
        return out, wb[:-1], sb[:-1], kb[:-1]

    def unpack(self, part):
        out = self.sa.unpack(getattr(self.sa, part))
        out.update(self.ss.unpack(getattr(self.ss, part)))
        return out


class WStep(Step):
    """tests/test_hip_iql.py's Step with the twin-Q phase through mobody_igdf_critic and a row weight."""

    def run(self, b, w, fused=False):
        from mobody_amd import ops
        c, mode = self.cfg, self.mode
        self.t += 1
        t, h = self.t, self.head(b)
        if fused:
            ops.iql_value(*h, self.loss[3:4], self.ws, m=self.v.am, v=self.v.av, t=t, lr=c["critic_lr"], log_out=self.log)
            ops.igdf_critic(*h, self.loss[0:1], self.ws, m=self.q.am, v=self.q.av, t=t, lr=c["critic_lr"], row_weight=w)
            ops.iql_actor(*h, self.loss[1:2], self.ws, m=self.pi.am, v=self.pi.av, t=t, lr=c["actor_lr"])
        else:
            ops.iql_value(*h, self.loss[3:4], self.ws, grad=self.v.grad, log_out=self.log)
            self.v.adam(t, c["critic_lr"], mode)
            ops.igdf_critic(*h, self.loss[0:1], self.ws, grad=self.q.grad, row_weight=w)
            self.q.adam(t, c["critic_lr"], mode, target=self.qt, tau=c["tau"])
            ops.iql_actor(*h, self.loss[1:2], self.ws, grad=self.pi.grad)
            self.pi.adam(t, ops.cosine_lr(c["actor_lr"], t, c["max_step"]), mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.adv[-1])), "the sentinel behind adv was overwritten"


def fixture_setup(tag):
    g = gu.load(f"g26_igdf_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = GR.igdf_cfg(S, A, **GR.VARIANTS[tag])
    pe = GR.info_params(S, A, int(g["seed_sa"]), int(g["seed_ss"]), cfg["repr_dim"], float(g["e_scale"]))
    src, tar = GR.g26_rows(S, A)
    return g, S, A, bs, cfg, pe, [np.asarray(x[:bs]) for x in src], [np.asarray(x[:bs]) for x in tar]


# ---- 1. the C ABI against the fixtures; fused == gradient form + mobody_adam_polyak ----------------------------------------------
@pytest.mark.parametrize("tag", list(GR.VARIANTS))
def test_c_abi_vs_reference_fixture(tag, mfma, dev):
    from mobody_amd import ops
    g, S, A, bs, cfg, pe, src, tar = fixture_setup(tag)
    Z, k = cfg["repr_dim"], int(g["k"])
    N = k + bs
    ref, fus = Info(S, A, Z, pe, dev, bs, mfma), Info(S, A, Z, pe, dev, bs, mfma)
    ib = to_dev([tar[0], tar[1], np.concatenate([tar[2], src[2][:bs - 1]], 0)], dev)
    ib0 = [x.clone() for x in ib]
    misses = []
    for step in range(1, GR.INFO_STEPS + 1):
        ref.step(ib, cfg["actor_lr"])
        fus.step(ib, cfg["actor_lr"], fused=True)
        print(tag, mfma, "info", step, float(ref.loss[0]), float(g["info_loss"][step - 1]))
        close(float(ref.loss[0]), g["info_loss"][step - 1], rtol=1e-5, atol=0)
        for name in ("sa", "ss"):
            for part in ("blob", "blob_T", "am", "av"):
                assert torch.equal(getattr(getattr(ref, name), part), getattr(getattr(fus, name), part)), (step, name, part)
        assert torch.equal(ref.loss[:1], fus.loss[:1])
        if f"i{step}_g::{GR.PARAM_ORDER[0]}" not in g:
            continue
        grads = ref.unpack("grad")
        for pre in GR.ENCS:
            ks = [x for x in grads if x.startswith(pre)]
            scale = max(float(np.abs(g[f"i{step}_g::{x}"]).max()) for x in ks)
            for x in ks:
                want = g[f"i{step}_g::{x}"].astype(np.float64)
                ratio = float((np.abs(gu.sub(grads[x]).astype(np.float64) - want) / (1e-5 * scale + 1e-5 * np.abs(want))).max())
                print("   grad", x, f"worst err / (rtol 1e-5, atol 1e-5 scale) = {ratio:.3g}")
                if not ratio <= 1.0:
                    misses.append((step, x, float("%.3g" % ratio)))
        for x, v in ref.unpack("blob").items():
            params_close(gu.sub(v), g[f"i{step}_p::{x}"], cfg["actor_lr"])
    assert all(torch.equal(a, b) for a, b in zip(ib, ib0))
    # the filter and IQL's three phases
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    ref_i, fus_i = WStep(S, A, pa, pq, pv, dev, N, cfg, mfma), WStep(S, A, pa, pq, pv, dev, N, cfg, mfma)
    for st in (ref_i, fus_i):                       # one workspace for the whole step: IQL's phases use its front
        st.ws = ops.igdf_workspace(st.dims, bs, Z, dev)
    staged = to_dev([np.concatenate([x, y], 0) for x, y in zip(src, tar)], dev)
    staged0 = [x.clone() for x in staged]
    short = tag == "short"
    for step in range(1, GR.STEPS[tag] + 1):
        b, w, sc, kept = ref.filter(staged, k, cfg["importance_weight"], ref_i.ws, ref_i.dims)
        bf, wf, _, _ = fus.filter(staged, k, cfg["importance_weight"], fus_i.ws, fus_i.dims)
        kp = kept.cpu().numpy()
        print(tag, mfma, step, "score max err", float(np.abs(sc.cpu().numpy() - g[f"s{step}_score"]).max()))
        close(sc.cpu().numpy(), g[f"s{step}_score"], rtol=0, atol=1e-5)
        assert np.array_equal(kp, g[f"s{step}_kept"])
        close(w.cpu().numpy(), g[f"s{step}_w"], rtol=1e-5, atol=0)
        idx = torch.as_tensor(np.concatenate([kp, bs + np.arange(bs)]), device=dev, dtype=torch.long)
        for o, s0, s1 in zip(b, staged, staged0):
            assert torch.equal(o, s0[idx]) and torch.equal(s0, s1)            # bit-equal copies; the staged batch is unchanged
        assert np.array_equal(gu.sub(b[0].cpu().numpy()), g[f"s{step}_state"]) and np.array_equal(b[3].cpu().numpy()[:, 0], g[f"s{step}_reward"])
        assert all(torch.equal(x, y) for x, y in zip(b, bf)) and torch.equal(w, wf)
        ref_i.run(b, w)
        fus_i.run(bf, wf, fused=True)
        q_loss, pi_loss, v_loss = float(ref_i.loss[0]), float(ref_i.loss[1]), float(ref_i.loss[3])
        print("   v", v_loss, float(g["v_loss"][step - 1]), "q", q_loss, float(g["q_loss"][step - 1]), "pi", pi_loss, float(g["pi_loss"][step - 1]))
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        close(ref_i.adv[:-1].cpu().numpy(), g[f"s{step}_adv"], rtol=1e-5, atol=1e-5)
        if not short:
            for nm, net in (("v", ref_i.v), ("q", ref_i.q), ("actor", ref_i.pi)):
                ks = [x for x in g if x.startswith(f"s{step}_{nm}_g::")]
                scale = max(float(np.abs(g[x]).max()) for x in ks)
                for x, v in net.unpack(net.grad).items():
                    close(gu.sub(v), g[f"s{step}_{nm}_g::{x}"], rtol=1e-5, atol=1e-5 * scale)
            for nm, net in (("v", ref_i.v), ("q", ref_i.q), ("qt", ref_i.qt)):
                for x, v in net.unpack(net.blob).items():
                    params_close(gu.sub(v), g[f"s{step}_{nm}_p::{x}"], cfg["critic_lr"])
        for x, v in ref_i.pi.unpack(ref_i.pi.blob).items():
            params_close(gu.sub(v), g[f"s{step}_actor_p::{x}"], cfg["actor_lr"])
        for name in ("v", "q", "qt", "pi"):
            for part in ("blob", "blob_T", "am", "av"):
                assert torch.equal(getattr(getattr(ref_i, name), part), getattr(getattr(fus_i, name), part)), (step, name, part)
        assert torch.equal(ref_i.loss, fus_i.loss)
    assert not misses, f"encoder gradients outside rtol 1e-5, atol 1e-5 scale (step, tensor, err / tolerance): {misses}"


# ---- 2. mobody_igdf_contrast per element against fp64 -------------------------------------------------------------------------------
def contrast_bounds(phi, pt, ps):
    phi, pt, ps = [np.asarray(x, np.float64) for x in (phi, pt, ps)]
    n, Z = phi.shape
    loss, dphi, dpt, dps, logits = GR.contrast(phi, pt, ps)
    El = Z * U * np.concatenate([(np.abs(phi) * np.abs(pt)).sum(1, keepdims=True), np.abs(phi) @ np.abs(ps).T], 1)
    s = GR.sigmoid(logits)
    s0 = GR.sigmoid(-logits[:, 0])
    G = s / (n * n); G[:, 0] = -s0 / (n * n)
    EG = (s * (1 - s) * El + 12 * U * s) / (n * n)
    EG[:, 0] = (s0 * (1 - s0) * El[:, 0] + 12 * U * s0) / (n * n)
    tiny = 2.0 ** -120
    Ephi = EG[:, :1] * np.abs(pt) + EG[:, 1:] @ np.abs(ps) + (n + 2) * U * (np.abs(G[:, :1]) * np.abs(pt) + np.abs(G[:, 1:]) @ np.abs(ps)) + tiny
    Ept = EG[:, :1] * np.abs(phi) + 2 * U * np.abs(dpt) + tiny
    Eps = EG[:, 1:].T @ np.abs(phi) + (n + 2) * U * (np.abs(G[:, 1:]).T @ np.abs(phi)) + tiny
    y = np.zeros((n, n)); y[:, 0] = 1
    terms = GR.bce_logits(logits, y)
    sl = s.copy(); sl[:, 0] = s0
    Eloss = ((sl * El + 12 * U * terms).sum() + (n + 40) * U * terms.sum()) / (n * n) + 2 * U * loss
    return (loss, dphi, dpt, dps), (Eloss, Ephi, Ept, Eps)


@pytest.mark.parametrize("Z", [1, 16, 40, 64, 128])
@pytest.mark.parametrize("n", [2, 31, 32, 33, 130])
def test_contrast_vs_fp64(n, Z, dev):
    from mobody_amd import ops
    rng = np.random.default_rng(1000 * n + Z)
    ldz = Z + 3
    amp = np.sqrt(30.0 / Z) * 1.3                                       # logits of a few tens at the aligned pairs
    phi = rng.standard_normal((n, Z)).astype(np.float32) * np.float32(amp) * rng.choice([0.05, 0.3, 1.0], (n, 1)).astype(np.float32)
    pt = (phi * rng.choice([-1.0, 1.0, 0.1], (n, 1)) + 0.1 * rng.standard_normal((n, Z))).astype(np.float32)
    ps = (phi[rng.integers(0, n, n - 1)] * rng.choice([-1.0, 1.0, 0.0], (n - 1, 1)) + 0.2 * rng.standard_normal((n - 1, Z))).astype(np.float32)
    (loss, dphi, dpt, dps), (El, Ephi, Ept, Eps) = contrast_bounds(phi, pt, ps)
    lg = GR.contrast(phi, pt, ps)[4]
    if n >= 31:
        assert lg.max() > 30 and lg.min() < -30, (lg.min(), lg.max())    # both ends of the stable form
    pad = lambda x: torch.as_tensor(np.concatenate([x, np.full((len(x), ldz - Z), np.nan, np.float32)], 1)).to(dev).contiguous()
    runs = [ops.igdf_contrast(pad(phi), pad(pt), pad(ps), Z) for _ in range(2)]
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                        # fixed summation order: the same bits
    l, dsa, dss = [x.cpu().numpy().astype(np.float64) for x in runs[0]]
    Np3 = (Z + 15) // 16 * 16
    assert dsa.shape == (n, Np3) and dss.shape == (2 * n - 1, Np3)
    assert np.isfinite(l).all() and np.isfinite(dsa).all() and np.isfinite(dss).all()
    assert not dsa[:, Z:].any() and not dss[:, Z:].any()                # padded columns: exactly zero
    worst = max(abs(l[0] - loss) / El, (np.abs(dsa[:, :Z] - dphi) / Ephi).max(), (np.abs(dss[:n, :Z] - dpt) / Ept).max(),
                (np.abs(dss[n:, :Z] - dps) / Eps).max())
    print(f"n={n} Z={Z}: loss {l[0]:.6g} ({loss:.6g}); worst err / bound = {worst:.3g}")
    assert worst <= 1.0


# ---- 3. mobody_igdf_select ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 33, 64, 130])
def test_select_is_a_permutation_prefix(n, dev):
    from mobody_amd import ops
    rng = np.random.default_rng(n)
    cases = [rng.standard_normal(n).astype(np.float32), np.round(rng.standard_normal(n)).astype(np.float32)]      # plain; exact ties
    x = rng.standard_normal(n).astype(np.float32)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 0.0, -0.0, np.nan], np.float32)
    x[rng.permutation(n)[:min(n, len(sp))]] = sp[:min(n, len(sp))]
    cases += [x, np.full(n, np.nan, np.float32), np.zeros(n, np.float32)]
    for sc in cases:
        for k in sorted({1, max(1, n // 2), n}):
            kb = torch.full((k + 1,), -7, dtype=torch.int32, device=dev)
            wb = torch.full((k + 1,), 123.0, device=dev)
            ops.igdf_select(torch.as_tensor(sc).to(dev), k, 2.0, kept=kb[:-1], w=wb[:-1])
            torch.cuda.synchronize()
            kept, w = kb[:-1].cpu().numpy(), wb[:-1].cpu().numpy()
            assert int(kb[-1]) == -7 and float(wb[-1]) == 123.0
            assert len(set(kept.tolist())) == k and kept.min() >= 0 and kept.max() < n
            assert np.array_equal(kept, GR.select(sc, k)), (n, k, sc, kept)
            fin = np.isfinite(sc[kept])
            assert not fin[:-1][~fin[1:]].any() if k > 1 else True       # non-finite scores come first among the kept: the last to be kept
            assert fin.sum() == min(k, int(np.isfinite(sc).sum()))
            with np.errstate(over="ignore", invalid="ignore"):
                want = np.exp(2.0 * sc[kept].astype(np.float64))
            np.testing.assert_allclose(w[fin], want[fin], rtol=1e-5)


# ---- 4. the row-weighted critic -----------------------------------------------------------------------------------------------------
def test_weighted_critic_vs_fp64_and_null_weight(mfma, dev):
    from mobody_amd import ops
    S, A, N = 17, 6, 57
    cfg = GR.igdf_cfg(S, A)
    pa, pq, pv = IR.iql_params(S, A, 431, 16.0)
    rows = gu.gi.batch(501, 64, S, A)
    b = to_dev([np.asarray(x[:N]) for x in rows], dev)
    w = np.exp(np.linspace(-3.0, 3.0, N)).astype(np.float32)[np.random.default_rng(5).permutation(N)]
    wd = torch.as_tensor(w).to(dev)
    a, c, d = (WStep(S, A, pa, pq, pv, dev, N, cfg, mfma) for _ in range(3))
    for st in (a, c, d):
        st.t = 1
    ops.igdf_critic(*a.head(b), a.loss[0:1], a.ws, grad=a.q.grad, row_weight=wd)
    ops.igdf_critic(*c.head(b), c.loss[0:1], c.ws, grad=c.q.grad, row_weight=None)
    ops.iql_critic(*d.head(b), d.loss[0:1], d.ws, grad=d.q.grad)
    torch.cuda.synchronize()
    assert torch.equal(c.q.grad, d.q.grad) and torch.equal(c.loss[0:1], d.loss[0:1])          # a null weight: the same bits
    assert not torch.equal(a.q.grad, d.q.grad)
    t64 = lambda p: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()}
    q64, v64 = t64(pq), t64(pv)
    s, ac, s2, r, nd = [torch.tensor(np.asarray(x[:N], np.float64)) for x in rows]

    def mlp(p, pre, x):
        h = torch.relu(x @ p[pre + "network.0.weight"].T + p[pre + "network.0.bias"])
        h = torch.relu(h @ p[pre + "network.2.weight"].T + p[pre + "network.2.bias"])
        return h @ p[pre + "network.4.weight"].T + p[pre + "network.4.bias"]
    y = (r + nd * cfg["gamma"] * mlp(v64, "network.", s2)).detach()
    x = torch.cat([s, ac], 1)
    wt = torch.tensor(w.astype(np.float64)).reshape(-1, 1)
    loss = (wt * (mlp(q64, "network1.", x) - y) ** 2).mean() + (wt * (mlp(q64, "network2.", x) - y) ** 2).mean()
    gq = torch.autograd.grad(loss, list(q64.values()))
    close(float(a.loss[0]), float(loss.detach()), rtol=1e-5, atol=0)
    got = a.q.unpack(a.q.grad)
    scale = max(float(v.abs().max()) for v in gq)
    for (name, _), want in zip(q64.items(), gq):
        close(got[name], want.numpy(), rtol=1e-5, atol=1e-5 * scale)


# ---- 5. the mirror ------------------------------------------------------------------------------------------------------------------
def load_fixture_weights(pol, g, S, A, pe):
    t = lambda d: {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    pol.policy.load_state_dict(t(pa)); pol.q_funcs.load_state_dict(t(pq)); pol.target_q_funcs.load_state_dict(t(pq))
    pol.v_func.load_state_dict(t(pv)); pol.info.load_state_dict(t(pe))


def mirror_run(tag, dev, unweighted=False, check=True):
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.igdf import IGDF
    g, S, A, bs, cfg, pe, _, _ = fixture_setup(tag)
    pol = call_algo("IGDF", cfg, 3, dev)
    assert isinstance(pol, IGDF) and pol.total_it == 0 and pol.update_interval == 2 and pol.info_optimizer.t == 0
    load_fixture_weights(pol, g, S, A, pe)
    rows_src, rows_tar = GR.g26_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    pol.config["info_update_step"] = 1
    for step in range(1, GR.INFO_STEPS + 1):
        pol.update_info(src.rb, tar.rb, bs, None)
        if check:
            close(pol.info_loss(), g["info_loss"][step - 1], rtol=1e-5, atol=0)
            if f"i{step}_p::{GR.PARAM_ORDER[0]}" in g:
                for k, v in pol.info.state_dict().items():
                    params_close(gu.sub(v.cpu().numpy()), g[f"i{step}_p::{k}"], cfg["actor_lr"])
    assert src.calls == [bs - 1] * GR.INFO_STEPS and tar.calls == [bs] * GR.INFO_STEPS and pol.info_optimizer.t == GR.INFO_STEPS
    del src.calls[:], tar.calls[:]
    if unweighted:
        from mobody_amd import ops
        pol._critic = lambda *a, **kw: ops.igdf_critic(*a, row_weight=torch.ones_like(pol._w), **kw)
    dev_q = []
    for step in range(1, GR.STEPS[tag] + 1):
        pol.train(src.rb, tar.rb, bs, None, None)
        q_loss, pi_loss, v_loss = pol.losses()
        dev_q.append(abs(q_loss - float(g["q_loss"][step - 1])) / float(g["q_loss"][step - 1]))
        if not check:
            continue
        close(pol._score.cpu().numpy(), g[f"s{step}_score"], rtol=0, atol=1e-5)
        assert np.array_equal(pol._kept.cpu().numpy(), g[f"s{step}_kept"])
        close(pol._w.cpu().numpy(), g[f"s{step}_w"], rtol=1e-5, atol=0)
        assert np.array_equal(pol._batch[3].cpu().numpy()[:, 0], g[f"s{step}_reward"])
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        short = tag == "short"
        nets = (("actor", pol.policy),) if short else (("v", pol.v_func), ("q", pol.q_funcs), ("qt", pol.target_q_funcs), ("actor", pol.policy))
        for nm, net in nets:
            for k, v in net.state_dict().items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
    n = GR.STEPS[tag]
    if check:
        assert src.calls == list(g["calls_src"]) and tar.calls == list(g["calls_tar"])
        opts = (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer)
        assert pol.total_it == int(g["total_it"]) == n and [o.t for o in opts] == [n] * 3
    return pol, g, dev_q


@pytest.mark.parametrize("tag", list(GR.VARIANTS))
def test_mirror_vs_reference_fixture(tag, mfma, dev):
    mirror_run(tag, dev)


def test_mirror_with_unit_weights_misses_the_fixture(mfma, dev):
    """The same run with the critic's row weights forced to 1: the critic's loss leaves the fixture's tolerance."""
    _, g, dev_q = mirror_run("default", dev, unweighted=True, check=False)
    print(mfma, "unit weights: relative q_loss deviation", dev_q)
    assert dev_q[0] > 1e-5 * 10


def _make(graph, dev, seeds=(1, 2), **over):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task = 17, 6, "walker2d-medium-v2"
    torch.manual_seed(3)
    cfg = dict(GR.igdf_cfg(S, A, max_step=40, info_update_step=6, **over), rng="device", seed=7, graph=graph)
    pol = call_algo("igdf", cfg, 3, dev)
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=seeds[0]), 4000, task, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=seeds[1]), 500, task, 1)
    return pol, src, tar


def test_graph_replay_equals_eager_steps(mfma, dev, tmp_path):
    """rng='device', config['graph'] = 1: the replayed info steps and twelve replayed train() steps equal the same steps enqueued
    eagerly (the steps' own closures run outside a capture), bit for bit; the counters advance by one per replay."""
    bs, steps = 65, 12                                                     # k = 48, N = 113: odd, no multiple of 32
    g, gs, gt = _make(1, dev)
    g.update_info(gs, gt, bs, None)                  # step 1 eager, five replays
    assert g._info_graph is not None and g.info_optimizer.t == 6 and g._ictr.tolist() == [5, 6]
    g.train(gs, gt, bs, None, None)                  # step 1 allocates the minibatches: eager
    assert g._graph is None
    for k in range(steps):
        g.train(gs, gt, bs, None, None)
        assert g._ctr.tolist() == [k + 1, k + 2, k + 2, k + 2]
    assert g._graph is not None and g._batch[0].shape[0] == 113
    assert [o.t for o in (g.v_optimizer, g.q_optimizer, g.policy_optimizer)] == [steps + 1] * 3
    e, es, et = _make(0, dev)
    e.config["info_update_step"] = 1
    e.update_info(es, et, bs, None)
    e._ictr[1] = e.info_optimizer.t
    seg = e._info_segment(es, et, bs)
    for _ in range(5):
        seg()
    e.train(es, et, bs, None, None)
    assert e._graph is None
    e._ctr[1], e._ctr[2], e._ctr[3] = e.q_optimizer.t, e.policy_optimizer.t, e.v_optimizer.t
    (seg,) = e._graph_segments(es, et, bs, 1, False)
    for _ in range(steps):
        seg()
    torch.cuda.synchronize()
    ig, ie = g.info, e.info
    for a, b in ((ig.encoder_sa.blob, ie.encoder_sa.blob), (ig.encoder_ss.blob, ie.encoder_ss.blob), (ig.encoder_ss.blob_T, ie.encoder_ss.blob_T),
                 (g.info_optimizer.sa.m, e.info_optimizer.sa.m), (g.info_optimizer.ss.v, e.info_optimizer.ss.v), (g._ictr, e._ictr),
                 (g._info_loss, e._info_loss), (g.q_funcs.blob, e.q_funcs.blob), (g.target_q_funcs.blob, e.target_q_funcs.blob),
                 (g.policy.blob, e.policy.blob), (g.v_func.blob, e.v_func.blob), (g._ctr, e._ctr), (g._loss, e._loss), (g._batch[0], e._batch[0]),
                 (g._batch[3], e._batch[3]), (g._w, e._w), (g._score, e._score), (g._kept, e._kept), (g._adv, e._adv)):
        assert torch.equal(a, b)
    kept = g._kept.cpu().numpy()
    assert len(set(kept.tolist())) == 48 and np.all(np.diff(g._score.cpu().numpy()[kept]) >= 0)
    assert all(np.isfinite(x) for x in g.losses() + (g.info_loss(),))
    g.save(str(tmp_path / "m"))
    g.load(str(tmp_path / "m"))
    assert g._graph is None and g._info_graph is None and g.info_optimizer.t == 6
    g.train(gs, gt, bs, None, None)
    assert g._graph is not None


REF_FILES = ["model_actor", "model_actor_lr_scheduler", "model_actor_optimizer", "model_critic", "model_critic_optimizer", "model_value",
             "model_value_optimizer"]
EXTRA = ["model_info", "model_info_optimizer"]


def test_mirror_checkpoint_round_trip_and_keys(mfma, dev, tmp_path):
    from mobody_amd.algo.call_algo import call_algo
    g, S, A, bs, cfg, pe, _, _ = fixture_setup("short")
    assert [str(x) for x in g["ckpt_files"]] == REF_FILES
    rows_src, rows_tar = GR.g26_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)

    def make():
        p = call_algo("igdf", cfg, 3, dev)
        load_fixture_weights(p, g, S, A, pe)
        return p
    a = make()
    a.update_info(src.rb, tar.rb, bs, None)
    for _ in range(3):
        a.train(src.rb, tar.rb, bs, None, None)
    (tmp_path / "full").mkdir(); (tmp_path / "seven").mkdir()
    a.save(str(tmp_path / "full" / "model"))
    assert sorted(os.listdir(tmp_path / "full")) == sorted(REF_FILES + EXTRA)
    ld = lambda s: torch.load(str(tmp_path / "full" / ("model" + s)), map_location="cpu", weights_only=True)
    inf, io = ld("_info"), ld("_info_optimizer")
    assert list(inf) == [str(x) for x in g["info_keys"]] == list(GR.PARAM_ORDER)
    assert ["x".join(str(d) for d in v.shape) for v in inf.values()] == [str(x) for x in g["info_shapes"]]
    assert io["param_groups"][0]["params"] == list(range(12)) and sorted(io["state"]) == list(range(12))
    assert all(float(io["state"][i]["step"]) == float(GR.INFO_STEPS) for i in range(12))
    topt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(v)) for v in inf.values()], lr=cfg["actor_lr"])
    topt.load_state_dict(io)                                               # loads into torch's own optimizer over 12 parameters
    import shutil
    for f in REF_FILES:
        shutil.copy(tmp_path / "full" / f, tmp_path / "seven" / f)
    b = make()
    b.load(str(tmp_path / "full" / "model"))
    opts = lambda p: [o.t for o in (p.v_optimizer, p.q_optimizer, p.policy_optimizer, p.info_optimizer)]
    assert opts(b) == [3, 3, 3, GR.INFO_STEPS]
    b.target_q_funcs.load_state_dict(a.target_q_funcs.state_dict())           # (the files hold no target net)
    a.config["info_update_step"] = b.config["info_update_step"] = 1
    for p in (a, b):
        p.update_info(src.rb, tar.rb, bs, None)
        for _ in range(2):
            p.train(src.rb, tar.rb, bs, None, None)
    for x, y in ((a.policy.blob, b.policy.blob), (a.q_funcs.blob, b.q_funcs.blob), (a.v_func.blob, b.v_func.blob),
                 (a.info.encoder_sa.blob, b.info.encoder_sa.blob), (a.info.encoder_ss.blob, b.info.encoder_ss.blob),
                 (a.info_optimizer.ss.v, b.info_optimizer.ss.v), (a._w, b._w)):
        assert torch.equal(x, y)
    # a directory holding only the reference's seven files loads: the encoders keep what the object had
    c = make()
    before = c.info.encoder_ss.blob.clone()
    c.load(str(tmp_path / "seven" / "model"))
    assert opts(c) == [3, 3, 3, 0] and torch.equal(c.info.encoder_ss.blob, before)


class W:
    def __init__(self):
        self.rows = {}

    def add_scalar(self, k, v, global_step=None):
        self.rows[k] = (float(v), global_step)


def test_logged_scalars(dev):
    from mobody_amd.algo.call_algo import call_algo
    g, S, A, bs, cfg, pe, _, _ = fixture_setup("default")
    pol = call_algo("igdf", cfg, 3, dev)
    load_fixture_weights(pol, g, S, A, pe)
    rows_src, rows_tar = GR.g26_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    w = W()
    pol.config["info_update_step"] = 100
    pol.update_info(src.rb, tar.rb, bs, w)
    assert sorted(w.rows) == ["train/info loss"] and w.rows["train/info loss"][1] == 100 and np.isfinite(w.rows["train/info loss"][0])
    assert w.rows["train/info loss"][0] < float(g["info_loss"][0])            # a hundred steps on the same rows: the loss has fallen
    pol = call_algo("igdf", cfg, 3, dev)
    load_fixture_weights(pol, g, S, A, pe)
    pol.update_info(src.rb, tar.rb, bs, None)
    w = W()
    pol.total_it = 4999
    pol.train(src.rb, tar.rb, bs, w, None)
    assert sorted(w.rows) == ["train/adv", "train/q1", "train/value"]
    close(w.rows["train/adv"][0], g["s1_adv"].astype(np.float64).mean(), rtol=1e-5, atol=1e-5)
    assert all(v[1] == 5000 for v in w.rows.values()) and pol._graph is None


def config_tree(tmp_path):
    import yaml
    want = json.load(open(os.path.join(gu.GOLDEN, "g26_igdf_configs.json")))
    d = tmp_path / "config" / "mujoco" / "igdf"
    d.mkdir(parents=True)
    with open(d / "walker2d.yaml", "w") as f:
        yaml.safe_dump(want["mujoco/walker2d"], f)
    return str(tmp_path / "config")


def test_cli_runs_igdf_without_dynamics(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.igdf import IGDF
    built = []
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: built.append("build_dynamics"))
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path))
    out_dir = tmp_path / "out"
    pol = tm.main(["--policy", "IGDF", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                   "--synthetic", "1", "--rng", "device", "--src_rows", "3000", "--tar_rows", "600", "--max_step", "300",
                   "--save-model", "--eval_freq", "150", "--log_every", "100", "--dir", str(out_dir),
                   "--params", json.dumps(dict(batch_size=64, graph=1, info_pretrain=1, info_update_step=20))])
    assert isinstance(pol, IGDF) and pol.total_it == 300 and pol.dynamics is None and built == [] and pol.T_max == 300
    assert pol._graph is not None and pol.info_optimizer.t == 20 and pol._ictr.tolist() == [19, 20] and pol._batch[0].shape[0] == 48 + 64
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3
    for ln in lines:
        assert all(np.isfinite(float(ln.split(k)[1].split()[0])) for k in ("q_loss ", "pi_loss ", "v_loss "))
    models = out_dir / "IGDF" / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "models"
    assert sorted(os.listdir(models)) == sorted(REF_FILES + EXTRA)
    pol.load(str(models / "model"))
    assert pol.info_optimizer.t == 20 and bool(torch.isfinite(pol.info.encoder_ss.blob).all())


def test_two_rank_job_is_refused_before_any_collective(tmp_path, monkeypatch):
    """Data-parallel IGDF is not built: under the project's launcher both ranks raise in the constructor -- before the first
    collective -- and the job ends with that message instead of waiting in one."""
    from test_cli_dp import _launcher
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path))
    r = _launcher(str(tmp_path), ["--policy", "IGDF"], timeout=120)
    assert r.returncode != 0
    assert "NotImplementedError" in r.stderr and "data-parallel IGDF is not built" in r.stderr, r.stderr[-3000:]
    assert "step 6:" not in r.stdout
