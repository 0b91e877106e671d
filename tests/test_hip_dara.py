"""The DARA baseline on the GPU: the two C-ABI entry points mobody_dara_classifier / mobody_dara_relabel (BwdSeed mode 7: the
double-softmax cross-entropy seed of the two classifier heads, one fused Adam over both), the mirror class DARA and the CLI, against
the reference's g25 fixtures (tests/golden/make_golden_dara.py) and fp64 per element (tests/dara_ref.py head_bounds).

Tolerances against the fixtures: classifier losses rtol 1e-5; classifier gradients rtol 1e-5, atol 1e-5 of the head's largest
entry; post-step parameters params_close at actor_lr; penalty and relabeled rewards rtol 1e-5, atol 1e-5; the IQL phases those of
tests/test_hip_iql.py.  Every case uses N <= 258 rows.
"""
import json
import os

import numpy as np
import pytest
import torch

import actor_ref as AR
import aux_ref as R
import dara_ref as DR
import f64_bounds as FB
import golden_util as gu
import iql_ref as IR
from test_hip_iql import FixedRows, Net, Step, to_dev
from test_hip_train import close, params_close

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Head(Net):
    """One classifier head on the device: blob, T blob, Adam moments, and a gradient blob with a sentinel float behind it."""

    def __init__(self, pc, pre, in_dim, dev, mode):
        from mobody_amd import ops, packing
        self.dims, self.prefixes = (in_dim, 2, 1), [pre]
        self.blob = packing.pack_mlp(pc, in_dim, 2, dev, prefixes=[pre])
        self.blob_T = ops.mlp_transpose(self.blob, in_dim, 2, 1, precision=mode)
        self.am, self.av = torch.zeros_like(self.blob), torch.zeros_like(self.blob)
        self.gbuf = torch.full((self.blob.numel() + 1,), NAN, device=dev)
        self.grad = self.gbuf[:-1]


class Cls:
    """mobody_dara_classifier + mobody_dara_relabel on one pair of heads, gradient form (+ mobody_adam_polyak) or fused form."""

    def __init__(self, S, A, pc, dev, N, mode, ws=None, n_global=None, n_src=0):
        from mobody_amd import ops
        self.sa, self.sas = Head(pc, DR.HEADS[0], S + A, dev, mode), Head(pc, DR.HEADS[1], 2 * S + A, dev, mode)
        ng = n_global or N
        self.dims, self.mode, self.N, self.n_src = ops.train_dims(S, A, N, N, ng, ng), mode, N, n_src
        self.ws = ws if ws is not None else ops.dara_workspace(self.dims, dev)
        self.loss = torch.full((3,), NAN, device=dev)
        ns = n_src or N // 2
        self.delta = torch.full((ns + 1,), NAN, device=dev)
        self.log = torch.full((2,), NAN, device=dev)
        self.t = 0

    def step(self, b, noise, std, lr, fused=False, **kw):
        from mobody_amd import ops
        self.t += 1
        head = (self.dims, self.mode, (self.sa, self.sas), b, std, self.loss[:2], self.ws)
        nz = dict(noise_sas=noise[0], noise_sa=noise[1]) if noise is not None else {}
        if fused:
            ops.dara_classifier(*head, n_src=self.n_src, opts=((self.sa.am, self.sa.av), (self.sas.am, self.sas.av)), t=self.t, lr=lr, **nz, **kw)
        else:
            ops.dara_classifier(*head, n_src=self.n_src, grads=(self.sa.grad, self.sas.grad), **nz, **kw)
            self.sa.adam(self.t, lr, self.mode)
            self.sas.adam(self.t, lr, self.mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.loss[2])) and bool(torch.isnan(self.sa.gbuf[-1])) and bool(torch.isnan(self.sas.gbuf[-1]))

    def relabel(self, b, eta):
        from mobody_amd import ops
        ops.dara_relabel(self.dims, self.mode, (self.sa, self.sas), b, eta, self.ws, n_src=self.n_src, delta_out=self.delta[:-1], log_out=self.log[:1])
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.delta[-1])) and bool(torch.isnan(self.log[1]))

    def unpack(self, part):
        out = self.sa.unpack(getattr(self.sa, part))
        out.update(self.sas.unpack(getattr(self.sas, part)))
        return out


def fixture_setup(tag, dev):
    g = gu.load(f"g25_dara_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = DR.dara_cfg(S, A, **DR.VARIANTS[tag])
    pc = DR.classifier_params(S, A, int(g["seed_sa"]), int(g["seed_sas"]), float(g["c_scale"]))
    return g, S, A, bs, cfg, pc


def reward_with_sentinel(b, dev):
    """The batch with its reward column re-made as the first N floats of an N + 1 buffer (NaN behind it)."""
    N = b[3].shape[0]
    buf = torch.full((N + 1,), NAN, device=dev)
    buf[:N] = b[3].reshape(-1)
    return [b[0], b[1], b[2], buf[:N].view(N, 1), b[4]], buf


# ---- 1. the C ABI against the fixtures; fused == gradient form + mobody_adam_polyak ----------------------------------------------
@pytest.mark.parametrize("tag", list(DR.VARIANTS))
def test_c_abi_vs_reference_fixture(tag, mfma, dev):
    """Every step of every variant: classifier losses, gradients and post-step parameters, the penalty and the relabeled rewards,
    then IQL's three phases on the relabeled batch; the fused form against the gradient form + mobody_adam_polyak bit for bit; a
    sentinel float behind every output array."""
    from mobody_amd import ops
    g, S, A, bs, cfg, pc = fixture_setup(tag, dev)
    eta = DR.eta_of(cfg)
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    b0 = to_dev(DR.g25_batch(bs, S, A), dev)
    N = b0[0].shape[0]
    ref_i, fus_i = Step(S, A, pa, pq, pv, dev, N, cfg, mfma), Step(S, A, pa, pq, pv, dev, N, cfg, mfma)
    for st in (ref_i, fus_i):                       # one workspace for the whole step: IQL's phases use its front
        st.ws = ops.dara_workspace(st.dims, dev)
    ref, fus = Cls(S, A, pc, dev, N, mfma, ws=ref_i.ws), Cls(S, A, pc, dev, N, mfma, ws=fus_i.ws)
    short = tag == "short"
    grad_misses = []
    for step in range(1, DR.STEPS[tag] + 1):
        noise = to_dev(DR.step_noise(g, step), dev)
        ref.step(b0, noise, cfg["gaussian_noise_std"], cfg["actor_lr"])
        fus.step(b0, noise, cfg["gaussian_noise_std"], cfg["actor_lr"], fused=True)
        l_sa, l_sas = float(ref.loss[0]), float(ref.loss[1])
        print(tag, mfma, step, "loss_sa", l_sa, float(g["cls_loss_sa"][step - 1]), "loss_sas", l_sas, float(g["cls_loss_sas"][step - 1]))
        close(l_sa, g["cls_loss_sa"][step - 1], rtol=1e-5, atol=0)
        close(l_sas, g["cls_loss_sas"][step - 1], rtol=1e-5, atol=0)
        grads = ref.unpack("grad")
        for pre in DR.HEADS:
            ks = [k for k in grads if k.startswith(pre)]
            scale = max(float(np.abs(g[f"s{step}_cls_g::{k}"]).max()) for k in ks)
            for k in ks:
                want = g[f"s{step}_cls_g::{k}"].astype(np.float64)
                ratio = float((np.abs(gu.sub(grads[k]).astype(np.float64) - want) / (1e-5 * scale + 1e-5 * np.abs(want))).max())
                print("   grad", k, f"worst err / (rtol 1e-5, atol 1e-5 scale) = {ratio:.3g}")
                if not ratio <= 1.0:                  # held to the end of the test, so that every other check of every step still runs
                    grad_misses.append((step, k, float("%.3g" % ratio)))
        for k, v in ref.unpack("blob").items():
            params_close(gu.sub(v), g[f"s{step}_cls_p::{k}"], cfg["actor_lr"])
        for name in ("sa", "sas"):
            for part in ("blob", "blob_T", "am", "av"):
                assert torch.equal(getattr(getattr(ref, name), part), getattr(getattr(fus, name), part)), (step, name, part)
        assert torch.equal(ref.loss[:2], fus.loss[:2])
        # the relabel of the training batch (a fresh copy of the rows: the reference's sample() hands out clones)
        b, rbuf = reward_with_sentinel([x.clone() for x in b0], dev)
        bf, fbuf = reward_with_sentinel([x.clone() for x in b0], dev)
        ref.relabel(b, eta)
        fus.relabel(bf, eta)
        pen, rew = ref.delta[:-1].cpu().numpy(), b[3].cpu().numpy()[:, 0]
        print("   penalty max err", float(np.abs(pen - g[f"s{step}_penalty"]).max()), "reward max err", float(np.abs(rew - g[f"s{step}_reward"]).max()))
        close(pen, g[f"s{step}_penalty"], rtol=1e-5, atol=1e-5)
        close(rew, g[f"s{step}_reward"], rtol=1e-5, atol=1e-5)
        close(float(ref.log[0]), g[f"s{step}_penalty"].astype(np.float64).mean(), rtol=1e-5, atol=1e-5)
        assert bool(torch.isnan(rbuf[-1])) and bool(torch.isnan(fbuf[-1])) and torch.equal(b[3][bs:], b0[3][bs:]) and torch.equal(b[3], bf[3])
        assert torch.equal(ref.delta[:-1], fus.delta[:-1]) and torch.equal(ref.log[:1], fus.log[:1])
        # IQL's three phases on the relabeled batch, at tests/test_hip_iql.py's tolerances
        ref_i.run(b)
        fus_i.run(bf, fused=True)
        q_loss, pi_loss, v_loss = float(ref_i.loss[0]), float(ref_i.loss[1]), float(ref_i.loss[3])
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        close(ref_i.adv[:-1].cpu().numpy(), g[f"s{step}_adv"], rtol=1e-5, atol=1e-5)
        if not short:
            for nm, net in (("v", ref_i.v), ("q", ref_i.q), ("actor", ref_i.pi)):
                ks = [k for k in g if k.startswith(f"s{step}_{nm}_g::")]
                scale = max(float(np.abs(g[k]).max()) for k in ks)
                for k, v in net.unpack(net.grad).items():
                    close(gu.sub(v), g[f"s{step}_{nm}_g::{k}"], rtol=1e-5, atol=1e-5 * scale)
            for nm, net in (("v", ref_i.v), ("q", ref_i.q), ("qt", ref_i.qt)):
                for k, v in net.unpack(net.blob).items():
                    params_close(gu.sub(v), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
        for k, v in ref_i.pi.unpack(ref_i.pi.blob).items():
            params_close(gu.sub(v), g[f"s{step}_actor_p::{k}"], cfg["actor_lr"])
        for name in ("v", "q", "qt", "pi"):
            for part in ("blob", "blob_T", "am", "av"):
                assert torch.equal(getattr(getattr(ref_i, name), part), getattr(getattr(fus_i, name), part)), (step, name, part)
        assert torch.equal(ref_i.loss, fus_i.loss)
    assert not grad_misses, f"classifier gradients outside rtol 1e-5, atol 1e-5 scale (step, tensor, err / tolerance): {grad_misses}"


# ---- 2. the classifier step per element against fp64 --------------------------------------------------------------------------------
CASES = [(3, 1, 1), (11, 3, 17), (17, 6, 32), (17, 6, 33), (45, 24, 129)]       # (S, A, bs): N = 2, 34, 64, 66, 258
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_DARA_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(dict(what="worst |got - fp64| / bound per tensor, tests/test_hip_dara.py part 2",
                           cases={k: {n: float("%.3g" % r) for n, r in v.items()} for k, v in sorted(RATIOS.items())}), f, indent=1)


_REF = {}


def case_reference(case):
    """Inputs and fp64 references of a case (shared by the f32 and the f16x2 run): rows whose ReLU masks cannot flip."""
    if case in _REF:
        return _REF[case]
    S, A, bs = case
    N, seed = 2 * bs, 3100 + 7 * S + bs
    gmul = 1 + bs % 2
    rng = np.random.default_rng(seed)
    pc = DR.classifier_params(S, A, seed, seed + 1, c_scale=4.0)
    pool = max(6 * N, 96)
    s, a, s2, _, _ = gu.gi.batch(seed + 5, pool, S, A)
    e_sas = rng.standard_normal((pool, 2 * S + A)).astype(np.float32)
    e_sa = rng.standard_normal((pool, S + A)).astype(np.float32)
    std = 0.5
    x_sas, x_sa = DR.inputs32((s, a, s2), (e_sas, e_sa), std)
    ok = IR.robust(DR.as_net(pc, DR.HEADS[0]), "network.", x_sa) & IR.robust(DR.as_net(pc, DR.HEADS[1]), "network.", x_sas)
    keep = np.flatnonzero(ok)
    assert keep.size >= N, (keep.size, N)
    rows = keep[:N]
    s, a, s2, e_sas, e_sa = [np.ascontiguousarray(x[rows]) for x in (s, a, s2, e_sas, e_sa)]
    x_sas, x_sa = x_sas[rows], x_sa[rows]
    Ng = gmul * N
    refs = {"sa": DR.head_reference(pc, DR.HEADS[0], x_sa, bs, Ng), "sas": DR.head_reference(pc, DR.HEADS[1], x_sas, bs, Ng)}
    _REF.clear()
    _REF[case] = out = dict(pc=pc, rows=(s, a, s2), noise=(e_sas, e_sa), std=std, x=dict(sa=x_sa, sas=x_sas), Ng=Ng, refs=refs)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"S{c[0]}A{c[1]}bs{c[2]}")
def test_classifier_step_vs_fp64_bounds(case, mfma, dev):
    """mobody_dara_classifier (gradient form) with explicit noise: both losses and all twelve gradient tensors within their
    per-element bounds of the fp64 reference.  The label boundary falls inside a 32-row tile at bs 17 and bs 33, the last tile is
    ragged at N = 2, 34, 66, 258, N_global is N or 2 N.  In f32 mode the existing composition (dara_inputs -> mlp3_forward(save) ->
    dara_loss_grad -> mlp3_backward) is held against the same step at the fixture tolerances."""
    from mobody_amd import ops
    S, A, bs = case
    c = case_reference(case)
    N, Ng = 2 * bs, c["Ng"]
    b = to_dev(c["rows"] + (np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)), dev)
    noise = to_dev(c["noise"], dev)
    k = Cls(S, A, c["pc"], dev, N, mfma, n_global=Ng)
    k.step(b, noise, c["std"], 3e-4)
    grads = k.unpack("grad")
    name = f"S{S}A{A}bs{bs}-{mfma}"
    RATIOS[name] = {}
    for nm, pre, li in (("sa", DR.HEADS[0], 0), ("sas", DR.HEADS[1], 1)):
        ref = c["refs"][nm]
        bd = DR.head_bounds(ref, c["x"][nm], N, Ng, mfma == "f16x2")
        got = {kk[len(pre):]: v for kk, v in grads.items() if kk.startswith(pre)}
        got = {"network." + kk: v for kk, v in got.items()}
        got["loss"], want, bound = float(k.loss[li]), dict(ref["grads"], loss=ref["loss"]), dict(bd["grads"], loss=bd["loss"])
        for kk in want:
            RATIOS[name][nm + ":" + kk] = AR.ratios(got[kk], want[kk], bound[kk])
        print(name, nm, {kk: f"{RATIOS[name][nm + ':' + kk]:.3g}" for kk in want})
        for kk in want:
            FB.check(got[kk], want[kk], bound[kk], f"{name} {nm} {kk}")
    if mfma != "f32":
        return
    # the composition that exists today (exact-fp32 forwards, separate loss launch, generic backward) on heads that have not
    # stepped; its mean is over the N local rows, so with N_global = 2 N its loss and gradients are halved (exactly)
    k0 = Cls(S, A, c["pc"], dev, N, mfma, n_global=Ng)
    share = N / Ng
    x_sas, x_sa = ops.dara_inputs(b[0], b[1], b[2], c["std"], noise[0], noise[1])
    (z_sas, xs, h1s, h2s) = ops.mlp3_forward(k0.sas.blob, 2 * S + A, 2, 1, x_sas, save=True)
    (z_sa, xa, h1a, h2a) = ops.mlp3_forward(k0.sa.blob, S + A, 2, 1, x_sa, save=True)
    dz_sas, dz_sa, loss = ops.dara_loss_grad(z_sas[0], z_sa[0], bs)
    close(k.loss[:2], loss * share, rtol=1e-5, atol=0)
    for head, new_head, dz, x, h1, h2 in ((k0.sas, k.sas, dz_sas, xs, h1s, h2s), (k0.sa, k.sa, dz_sa, xa, h1a, h2a)):
        gold = torch.zeros_like(head.blob)
        ops.mlp3_backward(head.blob_T, head.dims[0], 2, 1, dz, x, h1, h2, gold)
        old, new = head.unpack(gold * share), new_head.unpack(new_head.grad)
        scale = max(float(np.abs(v).max()) for v in old.values())
        for kk in old:
            close(new[kk], old[kk], rtol=1e-5, atol=1e-5 * scale)


# ---- 3. the relabel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"S{c[0]}A{c[1]}bs{c[2]}")
def test_relabel_vs_fp64(case, mfma, dev):
    """mobody_dara_relabel against aux_ref.dara_penalty_ref of the fp64 logits: the penalty within the row-wise bound of
    tests/test_hip_aux_rowwise.py (90 u for exact logits) plus the forward error of the four logits through the log-ratios (each
    log q moves by at most 1/2 per unit of z0 - z1, as the row loss of head_bounds); rows >= n_src keep their bits, delta_out and
    log_out agree, eta = 0 leaves the rewards' bits alone."""
    S, A, bs = case
    c = case_reference(case)
    N = 2 * bs
    U = 2.0 ** -24
    rng = np.random.default_rng(bs)
    r0 = rng.standard_normal((N, 1)).astype(np.float32)
    r0[0, 0] = -0.0
    k = Cls(S, A, c["pc"], dev, N, mfma)
    x_sas, x_sa = DR.inputs32(c["rows"], None, 0.0)
    E = 0.0
    z = {}
    for nm, pre, x in (("sa", DR.HEADS[0], x_sa[:bs]), ("sas", DR.HEADS[1], x_sas[:bs])):
        pn = DR.as_net(c["pc"], pre)
        la = FB.net_weights(pn, "network.")
        z[nm], Ez = FB.e2e_bound(x.astype(np.float64), la, FB.C_E2E, mfma == "f16x2", np.maximum(la[0][1], 0).max())
        E = E + (Ez[:, 0] + Ez[:, 1])                                        # two logs per head, 1/2 each
    want, raw = R.dara_penalty_ref(z["sas"], z["sa"])
    assert np.array_equal(want, raw) and np.abs(raw).max() <= 2.0
    for eta in (0.0, 0.1, -2.5):
        ef = float(np.float32(eta))
        b, rbuf = reward_with_sentinel(to_dev(c["rows"] + (r0, np.ones((N, 1), np.float32)), dev), dev)
        k.delta.fill_(NAN); k.log.fill_(NAN)
        k.relabel(b, ef)
        got_d, got_r = k.delta[:-1].cpu().numpy(), b[3].cpu().numpy()[:, 0]
        FB.check(got_d, want, 90 * U + E, f"{case} {mfma} delta")
        new = r0[:bs, 0].astype(np.float64) + ef * want
        FB.check(got_r[:bs], new, abs(ef) * (90 * U + E) + U * np.abs(ef * want) + U * np.abs(new), f"{case} {mfma} reward eta={eta}")
        assert np.array_equal(got_r[bs:].view(np.uint32), r0[bs:, 0].view(np.uint32)) and bool(torch.isnan(rbuf[-1]))
        d64 = got_d.astype(np.float64)
        FB.check(float(k.log[0]), d64.mean(), (bs + 3) * U * np.abs(d64).mean() + 2 * U * abs(d64.mean()), f"{case} {mfma} log_out")
        if eta == 0.0:
            assert np.array_equal(got_r.view(np.uint32), r0[:, 0].view(np.uint32))
        else:
            assert np.array_equal(got_r[:bs], (r0[:bs, 0] + np.float32(ef) * got_d).astype(np.float32))


# ---- 4. the mirror ---------------------------------------------------------------------------------------------------------------
def load_fixture_weights(pol, g, S, A):
    t = lambda d: {k: torch.from_numpy(np.asarray(v)) for k, v in d.items()}
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    pc = DR.classifier_params(S, A, int(g["seed_sa"]), int(g["seed_sas"]), float(g["c_scale"]))
    pol.policy.load_state_dict(t(pa)); pol.q_funcs.load_state_dict(t(pq)); pol.target_q_funcs.load_state_dict(t(pq))
    pol.v_func.load_state_dict(t(pv)); pol.classifier.load_state_dict(t(pc))


def mirror_run(tag, dev, eta0=False, check=True):
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.dara import DARA
    g, S, A, bs, cfg, pc = fixture_setup(tag, dev)
    pol = call_algo("DARA", cfg, 3, dev)
    assert isinstance(pol, DARA) and pol.total_it == 0 and pol.eta == float(g["eta"])
    if eta0:
        pol.eta = 0.0
    load_fixture_weights(pol, g, S, A)
    rows_src, rows_tar = DR.g25_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    steps = {"n": 0}
    pol.classifier_noise_fn = lambda n: DR.step_noise(g, steps["n"])
    dev_q, dev_r = [], []
    for step in range(1, DR.STEPS[tag] + 1):
        steps["n"] = step
        pol.train(src.rb, tar.rb, bs, None, None)
        q_loss, pi_loss, v_loss = pol.losses()
        l_sa, l_sas = pol.classifier_losses()
        rew = pol._batch[3].cpu().numpy()[:, 0]
        dev_q.append(abs(q_loss - float(g["q_loss"][step - 1])) / float(g["q_loss"][step - 1]))
        dev_r.append(float(np.abs(rew - g[f"s{step}_reward"]).max()))
        if not check:
            continue
        close(l_sa, g["cls_loss_sa"][step - 1], rtol=1e-5, atol=0)
        close(l_sas, g["cls_loss_sas"][step - 1], rtol=1e-5, atol=0)
        close(rew, g[f"s{step}_reward"], rtol=1e-5, atol=1e-5)
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        for k, v in pol.classifier.state_dict().items():
            params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_cls_p::{k}"], cfg["actor_lr"])
        short = tag == "short"
        nets = (("actor", pol.policy),) if short else (("v", pol.v_func), ("q", pol.q_funcs), ("qt", pol.target_q_funcs), ("actor", pol.policy))
        for nm, net in nets:
            for k, v in net.state_dict().items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
    n = DR.STEPS[tag]
    if check:
        assert src.calls == list(g["calls_src"]) and tar.calls == list(g["calls_tar"])
        opts = (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer, pol.classifier_optimizer)
        assert pol.total_it == int(g["total_it"]) == n and [o.t for o in opts] == [n] * 4
    return pol, g, dev_q, dev_r


@pytest.mark.parametrize("tag", list(DR.VARIANTS))
def test_mirror_train_vs_reference_fixture(tag, mfma, dev):
    pol, g, _, _ = mirror_run(tag, dev)
    # the penalty of the last step, through the public relabel path with delta_out
    pol._relabel([x.clone() for x in pol._batch], pol._batch[0].shape[0], log=True)
    torch.cuda.synchronize()
    # (the batch's rewards were relabeled in place by train(); the penalty itself does not read them)
    close(pol._delta.cpu().numpy(), g[f"s{DR.STEPS[tag]}_penalty"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag", ["default", "eta2"])
def test_mirror_with_eta_zero_misses_the_fixture(tag, mfma, dev):
    """The same run with eta forced to 0: the rewards and the critic's loss leave the fixture's tolerances."""
    _, g, dev_q, dev_r = mirror_run(tag, dev, eta0=True, check=False)
    print(tag, mfma, "eta = 0: relative q_loss deviation", dev_q, "max reward deviation", dev_r)
    assert dev_r[0] > 1e-3 and dev_q[0] > 1e-5 * 10


# ---- 5. graph replay ---------------------------------------------------------------------------------------------------------------
def _make(graph, dev, seeds=(1, 2), **over):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task = 17, 6, "walker2d-medium-v2"
    torch.manual_seed(3)
    cfg = dict(DR.dara_cfg(S, A, max_step=40, **over), rng="device", seed=7, graph=graph)
    pol = call_algo("dara", cfg, 3, dev)
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=seeds[0]), 4000, task, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=seeds[1]), 500, task, 1)
    return pol, src, tar


def test_graph_replay_equals_eager_steps(mfma, dev, tmp_path):
    """rng='device', config['graph'] = 1: twelve replayed steps equal the same twelve steps enqueued eagerly (the step's own
    closure run outside a capture: the same device counters, the same launches), bit for bit; the call word and the classifier's
    device step count advance by one per replay."""
    bs, steps = 64, 12
    g, gs, gt = _make(1, dev)
    g.train(gs, gt, bs, None, None)                  # step 1 allocates the minibatches: eager
    assert g._graph is None
    for k in range(steps):
        g.train(gs, gt, bs, None, None)
        assert g._ctr.tolist() == [k + 1, k + 2, k + 2, k + 2, k + 2]
    assert g._graph is not None
    assert [o.t for o in (g.v_optimizer, g.q_optimizer, g.policy_optimizer, g.classifier_optimizer)] == [steps + 1] * 4
    e, es, et = _make(0, dev)
    e.train(es, et, bs, None, None)
    assert e._graph is None
    e._ctr[1], e._ctr[2], e._ctr[3], e._ctr[4] = e.q_optimizer.t, e.policy_optimizer.t, e.v_optimizer.t, e.classifier_optimizer.t
    (seg,) = e._graph_segments(es, et, bs, 1, False)
    for _ in range(steps):
        seg()
    torch.cuda.synchronize()
    cg, ce = g.classifier, e.classifier
    for a, b in ((g.q_funcs.blob, e.q_funcs.blob), (g.target_q_funcs.blob, e.target_q_funcs.blob), (g.policy.blob, e.policy.blob),
                 (g.v_func.blob, e.v_func.blob), (cg.sa_classifier.blob, ce.sa_classifier.blob), (cg.sas_classifier.blob, ce.sas_classifier.blob),
                 (cg.sas_classifier.blob_T, ce.sas_classifier.blob_T), (cg.opt_sa.m, ce.opt_sa.m), (cg.opt_sas.v, ce.opt_sas.v),
                 (g._ctr, e._ctr), (g._loss, e._loss), (g._cls_loss, e._cls_loss), (g._batch[0], e._batch[0]), (g._batch[3], e._batch[3]),
                 (g._cbatch[0], e._cbatch[0]), (g._adv, e._adv)):
        assert torch.equal(a, b)
    assert not torch.equal(g._batch[0], g._cbatch[0])                       # the classifier's batch is a draw of its own
    assert all(np.isfinite(x) for x in g.losses() + g.classifier_losses())
    g.save(str(tmp_path / "m"))
    g.load(str(tmp_path / "m"))
    assert g._graph is None
    g.train(gs, gt, bs, None, None)
    assert g._graph is not None and g.classifier_optimizer.t == steps + 2 and int(g._ctr[4]) == steps + 2


# ---- 6. checkpoints ----------------------------------------------------------------------------------------------------------------
REF_FILES = ["model_actor", "model_actor_optimizer", "model_classifier", "model_classifier_optimizer", "model_critic", "model_critic_optimizer"]
EXTRA = ["model_actor_lr_scheduler", "model_value", "model_value_optimizer"]


def test_mirror_checkpoint_round_trip_and_keys(mfma, dev, tmp_path):
    from mobody_amd.algo.call_algo import call_algo
    g, S, A, bs, cfg, pc = fixture_setup("short", dev)
    assert [str(x) for x in g["ckpt_files"]] == REF_FILES
    rows_src, rows_tar = DR.g25_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)

    def make():
        p = call_algo("dara", cfg, 3, dev)
        load_fixture_weights(p, g, S, A)
        n = {"k": 0}

        def fn(rows):
            n["k"] += 1
            return DR.step_noise(g, (n["k"] - 1) % 6 + 1)
        p.classifier_noise_fn = fn
        return p, n
    (a, na) = make()
    for _ in range(3):
        a.train(src.rb, tar.rb, bs, None, None)
    (tmp_path / "full").mkdir(); (tmp_path / "six").mkdir()
    a.save(str(tmp_path / "full" / "model"))
    assert sorted(os.listdir(tmp_path / "full")) == sorted(REF_FILES + EXTRA)
    ld = lambda s: torch.load(str(tmp_path / "full" / ("model" + s)), map_location="cpu", weights_only=True)
    cl, co = ld("_classifier"), ld("_classifier_optimizer")
    assert list(cl) == [str(x) for x in g["ckpt_classifier_keys"]]
    assert ["x".join(str(d) for d in v.shape) for v in cl.values()] == [str(x) for x in g["ckpt_classifier_shapes"]]
    assert co["param_groups"][0]["params"] == [int(x) for x in g["ckpt_cls_opt_params"]] == list(range(12))
    assert sorted(co["state"]) == [int(x) for x in g["ckpt_cls_opt_state_keys"]]
    assert sorted(co["param_groups"][0]) == [str(x) for x in g["ckpt_cls_opt_group_keys"]]
    assert sorted(co["state"][0]) == [str(x) for x in g["ckpt_cls_opt_entry_keys"]]
    assert ["x".join(str(d) for d in co["state"][i]["exp_avg"].shape) for i in range(12)] == [str(x) for x in g["ckpt_cls_opt_shapes"]]
    assert all(float(co["state"][i]["step"]) == 3.0 for i in range(12))
    # the file loads into torch's own optimizer over 12 parameters (what the reference's load_state_dict call does)
    ps = [torch.nn.Parameter(torch.zeros_like(v)) for v in cl.values()]
    topt = torch.optim.Adam(ps, lr=cfg["actor_lr"])
    topt.load_state_dict(co)
    import shutil
    for f in REF_FILES:
        shutil.copy(tmp_path / "full" / f, tmp_path / "six" / f)
    b, nb = make()
    b.load(str(tmp_path / "full" / "model"))
    nb["k"] = na["k"]
    opts = lambda p: [o.t for o in (p.v_optimizer, p.q_optimizer, p.policy_optimizer, p.classifier_optimizer)]
    assert opts(b) == [3, 3, 3, 3] and b.policy_optimizer.lr == cfg["actor_lr"]
    b.target_q_funcs.load_state_dict(a.target_q_funcs.state_dict())           # (the reference's files hold no target net)
    for _ in range(2):
        a.train(src.rb, tar.rb, bs, None, None)
        b.train(src.rb, tar.rb, bs, None, None)
    cg, cb = a.classifier, b.classifier
    for x, y in ((a.policy.blob, b.policy.blob), (a.q_funcs.blob, b.q_funcs.blob), (a.v_func.blob, b.v_func.blob),
                 (cg.sa_classifier.blob, cb.sa_classifier.blob), (cg.sas_classifier.blob, cb.sas_classifier.blob), (cg.opt_sas.v, cb.opt_sas.v)):
        assert torch.equal(x, y)
    # a directory holding only the reference's six files loads: V and the schedule keep what the object had
    c, _ = make()
    c.load(str(tmp_path / "six" / "model"))
    assert opts(c) == [0, 3, 3, 3] and torch.equal(c.classifier.sas_classifier.blob, ld_blob(tmp_path, c, dev))


def ld_blob(tmp_path, pol, dev):
    """The sas head of the saved classifier file, packed as the object packs it."""
    from mobody_amd import packing
    sd = torch.load(str(tmp_path / "six" / "model_classifier"), map_location="cpu", weights_only=True)
    return packing.pack_mlp({k: v for k, v in sd.items() if k.startswith("sas_classifier.")}, 2 * pol.S + pol.A, 2, dev, prefixes=["sas_classifier."])


# ---- 7. logged scalars -------------------------------------------------------------------------------------------------------------
def test_logged_scalars(dev):
    from mobody_amd.algo.call_algo import call_algo
    g, S, A, bs, cfg, pc = fixture_setup("default", dev)
    pol = call_algo("dara", cfg, 3, dev)
    load_fixture_weights(pol, g, S, A)
    pol.classifier_noise_fn = lambda n: DR.step_noise(g, 1)
    rows_src, rows_tar = DR.g25_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)

    class W:
        def __init__(self):
            self.rows = {}

        def add_scalar(self, k, v, global_step=None):
            self.rows[k] = (float(v), global_step)
    w = W()
    pol.total_it = 4999
    pol.train(src.rb, tar.rb, bs, w, None)
    assert sorted(w.rows) == ["train/adv", "train/q1", "train/reward penalty", "train/sa classifier loss", "train/sas classifier loss", "train/value"]
    close(w.rows["train/sas classifier loss"][0], g["cls_loss_sas"][0], rtol=1e-5, atol=0)
    close(w.rows["train/sa classifier loss"][0], g["cls_loss_sa"][0], rtol=1e-5, atol=0)
    close(w.rows["train/reward penalty"][0], g["s1_penalty"].astype(np.float64).mean(), rtol=1e-5, atol=1e-5)
    close(w.rows["train/adv"][0], g["s1_adv"].astype(np.float64).mean(), rtol=1e-5, atol=1e-5)
    assert all(v[1] == 5000 for v in w.rows.values()) and pol._graph is None


# ---- 8., 9. the CLI, the launcher ----------------------------------------------------------------------------------------------------
def config_tree(tmp_path):
    import yaml
    want = json.load(open(os.path.join(gu.GOLDEN, "g25_dara_configs.json")))
    d = tmp_path / "config" / "mujoco" / "dara"
    d.mkdir(parents=True)
    with open(d / "walker2d.yaml", "w") as f:
        yaml.safe_dump(want["mujoco/walker2d"], f)
    return str(tmp_path / "config")


def test_cli_runs_dara_without_dynamics(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.dara import DARA
    built = []
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: built.append("build_dynamics"))
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path))
    out_dir = tmp_path / "out"
    pol = tm.main(["--policy", "DARA", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                   "--synthetic", "1", "--rng", "device", "--src_rows", "3000", "--tar_rows", "600", "--max_step", "300",
                   "--save-model", "--eval_freq", "150", "--log_every", "100", "--dir", str(out_dir),
                   "--params", json.dumps(dict(batch_size=64, graph=1))])
    assert isinstance(pol, DARA) and pol.total_it == 300 and pol.dynamics is None and built == [] and pol.T_max == 300 and pol.eta == 0.1
    assert pol._graph is not None and pol.classifier_optimizer.t == 300 and int(pol._ctr[4]) == 300
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3
    for ln in lines:
        assert all(np.isfinite(float(ln.split(k)[1].split()[0])) for k in ("q_loss ", "pi_loss ", "v_loss "))
    models = out_dir / "DARA" / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "models"
    assert sorted(os.listdir(models)) == sorted(REF_FILES + EXTRA)
    pol.load(str(models / "model"))
    assert pol.classifier_optimizer.t == 300 and bool(torch.isfinite(pol.classifier.sas_classifier.blob).all())


def test_two_rank_job_is_refused_before_any_collective(tmp_path, monkeypatch):
    """Data-parallel DARA is not built: under the project's launcher both ranks raise in the constructor -- before the first
    collective -- and the job ends with that message instead of waiting in one."""
    from test_cli_dp import _launcher
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path))
    r = _launcher(str(tmp_path), ["--policy", "DARA"], timeout=120)
    assert r.returncode != 0
    assert "NotImplementedError" in r.stderr and "data-parallel DARA is not built" in r.stderr, r.stderr[-3000:]
    assert "step 6:" not in r.stdout
