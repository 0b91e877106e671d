"""The TD3_BC baseline on the GPU: the two C-ABI entry points mobody_td3bc_actor_forward / _backward (BwdSeed mode 4, the frozen
twin-Q seed with the gradient through the BC weight), the mirror class TD3BC and the CLI, against the reference's g23 fixtures
(tests/golden/make_golden_td3bc.py), MOBODY's own actor entry points where the two coincide, and fp64 per element.

Tolerances: those tests/test_hip_train.py applies to G7 (written at each assert); the per-element part takes the bound of
tests/td3bc_ref.py td3bc_bounds.  Every case uses N <= 257 rows.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import actor_ref as AR
import f64_bounds as FB
import golden_util as gu
import td3bc_ref as TR
from test_hip_train import close, params_close

pytestmark = pytest.mark.gpu

NON_DARA = ["default", "adv", "adv_bc05"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def td3_cfg(S, A, **over):
    """(the reference's config, the same step in the terms ops.hyper reads)"""
    from mobody_amd.algo.offline_offline.td3_bc import step_config
    cfg = gu.policy_cfg(S, A, **over)
    return cfg, step_config(cfg)


class Step:
    """mobody_critic(policy_forward = 1) -> Adam + Polyak -> the two TD3_BC actor calls -> Adam on one Engine's blobs, in the
    gradient form (fused=False) or the fused form."""

    def __init__(self, S, A, pa, pq, dev, N, step_cfg, n_global=None):
        from mobody_amd import ops
        from mobody_amd.engine import Engine
        self.e = Engine(S, A, pa, pq, dev)
        self.cfg, self.S, self.A = step_cfg, S, A
        ng = n_global or N
        self.dims, self.hyp = ops.train_dims(S, A, N, N, ng, ng), ops.hyper(step_cfg)
        self.ws = ops.train_workspace(self.dims, dev)

    def run(self, b, fused=False, apply=True):
        from mobody_amd import ops
        e, cfg, S, A = self.e, self.cfg, self.S, self.A
        prec = self.hyp.precision
        if fused:
            e.t += 1
            ops.critic_update(self.dims, self.hyp, e.actor, e.q, e.q_T, e.qt, b, e.mq, e.vq, e.t, cfg["critic_lr"], e.loss[0:1],
                              self.ws, policy_forward=True, actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T)
            ops.td3bc_actor_forward(self.dims, self.hyp, e.actor, e.q, b[0], b[1], e.stats, self.ws, policy_ready=True,
                                    actor_blob_T=e.actor_T, q_blob_T=e.q_T)
            ops.td3bc_actor_update(self.dims, self.hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], e.stats, e.ma, e.va, e.t,
                                   cfg["actor_lr"], e.loss[1:3], self.ws)
        else:
            ops.critic_step(self.dims, self.hyp, e.actor, e.q, e.q_T, e.qt, b, e.gq, e.loss[0:1], self.ws, policy_forward=True,
                            actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T)
            if apply:
                e.t += 1
                ops.adam_polyak(S + A, 1, 2, e.q, e.q_T, e.gq, e.mq, e.vq, e.qt, e.t, cfg["critic_lr"], cfg["tau"],
                                target_T=e.qt_T, precision=prec)
            ops.td3bc_actor_forward(self.dims, self.hyp, e.actor, e.q, b[0], b[1], e.stats, self.ws, policy_ready=True,
                                    actor_blob_T=e.actor_T, q_blob_T=e.q_T)
            ops.td3bc_actor_backward(self.dims, self.hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], e.stats, e.ga,
                                     e.loss[1:3], self.ws)
            if apply:
                ops.adam_polyak(S, A, 1, e.actor, e.actor_T, e.ga, e.ma, e.va, None, e.t, cfg["actor_lr"], precision=prec)
        torch.cuda.synchronize()


def to_dev(batch, dev):
    return [torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous() for x in batch]


# ---- 1. the C ABI against the fixtures; fused == gradient form + mobody_adam_polyak ------------------------------------------
@pytest.mark.parametrize("tag", NON_DARA)
def test_c_abi_vs_reference_fixture(tag, mfma, dev):
    g = gu.load(f"g23_td3bc_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg, scfg = td3_cfg(S, A, **TR.VARIANTS[tag])
    pa, pq, _ = gu.policy_params(int(g["seed"]), S, A)
    b = to_dev(TR.g23_batch(cfg, bs, S, A), dev)
    N = b[0].shape[0]
    assert N == {"adv_bc05": 48}.get(tag, 64)
    ref, fus = Step(S, A, pa, pq, dev, N, scfg), Step(S, A, pa, pq, dev, N, scfg)
    for step in (1, 2):
        ref.run(b)
        fus.run(b, fused=True)
        e = ref.e
        q_loss, pi_loss = float(e.loss[0]), float(e.loss[1])
        print(tag, mfma, step, "q_loss", q_loss, float(g["q_loss"][step - 1]), "pi_loss", pi_loss, float(g["pi_loss"][step - 1]))
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        for nm, blob in (("q", e.gq), ("actor", e.ga)):
            ks = [k for k in g if k.startswith(f"s{step}_{nm}_g::")]
            scale = max(float(np.abs(g[k]).max()) for k in ks)
            for k, v in e.unpack(blob, nm).items():
                close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_g::{k}"], rtol=1e-5, atol=1e-5 * scale)
        for nm, blob in (("q", e.q), ("actor", e.actor), ("qt", e.qt)):
            for k, v in e.unpack(blob, "actor" if nm == "actor" else "q").items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
        for name in ("q", "q_T", "qt", "mq", "vq", "actor", "actor_T", "ma", "va", "loss", "stats"):
            assert torch.equal(getattr(ref.e, name), getattr(fus.e, name)), (step, name)
        assert float(e.stats[1]) == 0.0


# ---- 2. q_weighted = 0: the bits of mobody_actor_forward / _backward at q_weighted = 0, scale_q = 1, Nt = N -------------------
@pytest.mark.parametrize("S,A,N", [(17, 6, 65), (11, 3, 33), (45, 24, 31)])
def test_unweighted_form_coincides_with_mobody_actor_calls(S, A, N, mfma, dev):
    from mobody_amd import ops
    cfg, scfg = td3_cfg(S, A, advantage=0, bc_coef=0.7, max_action=0.4)
    assert scfg["q_weighted"] == 0 and scfg["scale_Q"] == 1
    pa, pq, _ = gu.policy_params(91, S, A)
    b = to_dev(gu.gi.batch(92, N, S, A), dev)
    outs = []
    for which in ("td3bc", "mobody"):
        st = Step(S, A, pa, pq, dev, N, scfg, n_global=2 * N)
        e = st.e
        ops.critic_step(st.dims, st.hyp, e.actor, e.q, e.q_T, e.qt, b, e.gq, e.loss[0:1], st.ws, policy_forward=True,
                        actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T)
        e.ga.fill_(float("nan")); e.loss.fill_(float("nan")); e.stats.fill_(float("nan"))
        fwd, bwd = (ops.td3bc_actor_forward, ops.td3bc_actor_backward) if which == "td3bc" else (ops.actor_forward, ops.actor_backward)
        fwd(st.dims, st.hyp, e.actor, e.q, b[0], b[1], e.stats, st.ws, policy_ready=True, actor_blob_T=e.actor_T, q_blob_T=e.q_T)
        bwd(st.dims, st.hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], e.stats, e.ga, e.loss[1:3], st.ws)
        torch.cuda.synchronize()
        outs.append((e.ga.clone(), e.loss[1:3].clone(), e.stats[0:1].clone()))
    for x, y, what in zip(outs[0], outs[1], ("gradient blob", "losses", "stats[0]")):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), what


# ---- 3. per element against fp64, weighted form --------------------------------------------------------------------------------
SA = [(11, 3), (17, 6), (45, 24), (111, 8)]
NS = [1, 31, 32, 33, 65, 257]
KINDS = ("plain", "clamp", "bc0", "ties")
CLAMP_ADV = (("ln100+1e-3", AR.LN100 + 1e-3), ("ln100-1e-3", AR.LN100 - 1e-3), ("ln100+1", AR.LN100 + 1.0), ("ln100-1", AR.LN100 - 1.0),
             ("+90", 90.0), ("-90", -90.0))
# (kind, (S, A), N, N_global / N, max_action, clamp target or None): every kind at every (S, A) and N; the clamp kind once per target
FP64_CASES = [(kind, sa, N, 1 + (i + j + k) % 2, (0.4, 1.0)[(i + j) % 2], tgt) for i, kind in enumerate(KINDS) for j, sa in enumerate(SA)
              for k, N in enumerate(NS) for tgt in (CLAMP_ADV if kind == "clamp" else (None,))]
RATIOS = {}


def fp64_id(c):
    return f"{c[0]}-S{c[1][0]}A{c[1][1]}-N{c[2]}-g{c[3]}-ma{c[4]}" + (f"-q/m={c[5][0]}" if c[5] else "")


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_TD3BC_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "worst |got - fp64| / bound per tensor, tests/test_hip_td3bc.py part 3", "cases": RATIOS}, f,
                      indent=1, sort_keys=True)


def fp64_case(kind, SA_, N, gmul, ma, seed):
    """Nets as gu.policy_params (ties: network2 = network1, every row ties), N robust rows out of a pool (FB.robust_rows) and
    the fp64 forwards."""
    S, A = SA_
    pa, pq, _ = gu.policy_params(seed, S, A)
    pq = {k: v.copy() for k, v in pq.items()}
    h = dict(max_action=ma, weight=2.5, bc_coef=0.0 if kind == "bc0" else 1.0, q_weighted=1)
    pool = max(4 * N, 64)
    s, a, _, _, _ = gu.gi.batch(seed + 5, pool, S, A)
    a = (a * np.float32(ma)).astype(np.float32)
    keep = np.flatnonzero(FB.robust_rows(pa, pq, s, a, max_action=ma))
    assert keep.size >= N, (keep.size, N)
    if kind == "ties":                              # network2 = network1: every row ties, in the kernels too (the same arithmetic
        for k in list(pq):                          # twice); the rows were screened with network1's masks in the untied critic
            if k.startswith("network2."):
                pq[k] = pq["network1." + k[len("network2."):]].copy()
    s, a = s[keep[:N]].copy(), a[keep[:N]].copy()
    fw = AR.forward_ref(pa, pq, s, a, 0, ma)
    Ng = gmul * N
    minq = np.minimum(fw["qp"][0], fw["qp"][1])
    return dict(pa=pa, pq=pq, s=s, act=a, h=h, N=N, Ng=Ng, fw=fw, minq=minq, gmul=gmul, kind=kind)


def run_td3bc_actor(c, mode, dev, stats_in=None, stats_mul=1.0):
    """pack -> NaN sentinels behind the gradient blob, the losses and the stats -> td3bc_actor_forward -> the stats handed on
    (scaled by N_global / N, or crafted) -> td3bc_actor_backward.  Returns (stats the forward wrote, gradients, loss_out[0:2], the
    fp32 twin Q at (s, pi(s)))."""
    from mobody_amd import _lib, ops, packing
    S, A, N = c["s"].shape[1], c["act"].shape[1], c["N"]
    cfg = dict(gamma=0.99, tau=0.005, mfma=mode, scale_Q=1, **{k: c["h"][k] for k in ("max_action", "weight", "bc_coef", "q_weighted")})
    actor = packing.pack_mlp([{k[len("network."):]: v for k, v in c["pa"].items()}], S, A, dev)
    q = packing.pack_mlp(c["pq"], S + A, 1, dev, prefixes=["network1.", "network2."])
    actor_T = ops.mlp_transpose(actor, S, A, 1, precision=mode)
    q_T = ops.mlp_transpose(q, S + A, 1, 2, precision=mode)
    dims, hyp = ops.train_dims(S, A, N, N, c["Ng"], c["Ng"]), ops.hyper(cfg)
    ws = ops.train_workspace(dims, dev)
    s, a = torch.from_numpy(c["s"]).to(dev).contiguous(), torch.from_numpy(c["act"]).to(dev).contiguous()
    L = _lib.mlp_layout(S, A, 1)
    n = L.total_floats
    buf = torch.full((n + 8,), float("nan"), device=dev)        # gradient blob | sentinel | losses | sentinel | stats | sentinel
    grad, loss, stats = buf[:n], buf[n + 1:n + 3], buf[n + 4:n + 6]
    ops.td3bc_actor_forward(dims, hyp, actor, q, s, a, stats, ws, actor_blob_T=actor_T, q_blob_T=q_T)
    torch.cuda.synchronize()
    wrote = stats.cpu().numpy().copy()
    # the fp32 twin Q at (s, pi(s)) as the forward kernels form it in this mode (only read to tell which side of the clamp a row took)
    pi32 = ops.mlp3_forward(actor, S, A, 1, s, out_mode=1, max_action=c["h"]["max_action"], blob_T=actor_T, precision=mode)[0]
    q32 = ops.mlp3_forward(q, S + A, 1, 2, s, pi32.contiguous(), blob_T=q_T, precision=mode).view(2, N).cpu().numpy()
    if stats_in is not None:
        stats.copy_(torch.tensor(stats_in, dtype=torch.float32, device=dev))
    else:
        stats.mul_(stats_mul)
    ops.td3bc_actor_backward(dims, hyp, actor, actor_T, q, q_T, s, a, stats, grad, loss, ws)
    torch.cuda.synchronize()
    for k in (n, n + 3, n + 6, n + 7):
        assert bool(torch.isnan(buf[k])), f"sentinel {k - n} behind the outputs was overwritten"
    assert bool(torch.isfinite(buf[:n]).all()) and bool(torch.isfinite(loss).all()), "NaN / unwritten entries in the outputs"
    g = {"network." + k: v.cpu().numpy() for k, v in packing.unpack_mlp(grad.clone(), S, A, 1)[0].items()}
    return wrote, g, loss.cpu().numpy().copy(), q32


def place_on_clamp(c, t, r0):
    """Row r0 of the case at q/m = t, signed.  The Q output biases of both members move together (the members' difference and
    every ReLU mask stay: the rows remain robust) until q[r0] has the sign of t and at least the batch's median magnitude; then
    the statistic handed to the backward is the fp32 value nearest m N_global with m = q[r0] / t.  Returns (case, stats_in)."""
    want = np.sign(t) * max(abs(c["minq"][r0]), float(np.median(np.abs(c["minq"]))), 0.25)
    pq = {k: v.copy() for k, v in c["pq"].items()}
    shift = np.float32(want - c["minq"][r0])
    for pre in ("network1.", "network2."):
        pq[pre + "network.4.bias"] = pq[pre + "network.4.bias"] + shift
    fw = AR.forward_ref(c["pa"], pq, c["s"], c["act"], 0, c["h"]["max_action"])
    minq = np.minimum(fw["qp"][0], fw["qp"][1])
    m = minq[r0] / t
    assert m > 0
    return dict(c, pq=pq, fw=fw, minq=minq), np.array([np.float32(m * c["Ng"]), 0.0], np.float64)


@functools.lru_cache(maxsize=4)
def fp64_reference(case):
    """The case, the statistic handed to the backward (None: the forward's own, times N_global / N), the fp64 closed forms and
    gradients, and for a clamp case the target row.  Cached: the f32 and the f16x2 run share it."""
    kind, sa, N, gmul, ma, tgt = case
    idx = FP64_CASES.index(case)
    c = fp64_case(kind, sa, N, gmul, ma, 900 + 17 * idx)
    h, Ng = c["h"], c["Ng"]
    if tgt is None:
        stats = np.array([gmul * np.abs(c["minq"]).sum(), 0.0])
        cf = TR.closed_forms(c["fw"]["pi"], c["fw"]["qp"], c["fw"]["dqda"], c["act"], h, N, Ng, stats=stats)
        grads, tape = AR.actor_grads_ref(c["pa"], c["s"], c["fw"], cf["dz3"])
        return c, None, cf, grads, tape, None
    r0 = idx % N                                    # the target row rotates with the case
    cc, stats_in = place_on_clamp(c, tgt[1], r0)
    cf = TR.closed_forms(cc["fw"]["pi"], cc["fw"]["qp"], cc["fw"]["dqda"], cc["act"], h, N, Ng, stats=stats_in)
    grads, tape = AR.actor_grads_ref(cc["pa"], cc["s"], cc["fw"], cf["dz3"])
    return cc, stats_in, cf, grads, tape, r0


@pytest.mark.parametrize("case", FP64_CASES, ids=fp64_id)
def test_weighted_form_vs_fp64_bounds(case, mfma, dev):
    """Clamp cases: ONE row is placed at the case's signed target q/m (place_on_clamp); the others fall where the batch puts them.
    A row within its a-priori error of the clamp may take either side of the select, and its bound then includes the whole
    gradient-through-weight term (td3bc_bounds `near`); that band is wide where mean|q| is small (the +-90 targets), so the
    rows whose side the forward kernels' own fp32 Q settles are taken out of it (td3bc_ref.clamp_side_resolved).  What stays in:
    a row whose fp32 e is within 64 ulp of 100, or on the other side than the fp64 e -- the ln 100 +- 1e-3 rows, if any."""
    kind, sa, N, gmul, ma, tgt = case
    assert AR.bwd_dx_nt(*sa) == {(11, 3): 1, (17, 6): 2, (45, 24): 0, (111, 8): 0}[sa]
    c, stats_in, cf, grads, tape, r0 = fp64_reference(case)
    fw, h, Ng = c["fw"], c["h"], c["Ng"]
    if kind == "ties":
        assert (fw["qp"][0] == fw["qp"][1]).all()
    if tgt is not None:
        t, above = tgt[1], int((cf["e"] > 100).sum())
        assert abs(cf["adv"][r0] - t) <= 1e-6 * abs(t)                   # the SIGNED target is reached
        assert (cf["e"][r0] > 100) == (t > AR.LN100) and above >= int(t > AR.LN100)
        if t == -90.0:
            assert cf["e"][r0] < 1e-38                                   # below fp32's normal range: expf flushes or underflows
    wrote, g, loss, q32 = run_td3bc_actor(c, mfma, dev, stats_in=stats_in, stats_mul=float(gmul))
    handed = np.float32(stats_in[0]) if stats_in is not None else np.float32(wrote[0]) * np.float32(gmul)
    resolved = TR.clamp_side_resolved(cf, q32, handed, Ng)
    bd = TR.td3bc_bounds(c["pa"], c["pq"], c["s"], c["act"], h, N, Ng, fw, cf, tape, mfma == "f16x2", stats_exact=stats_in is not None,
                         resolved=resolved)
    if tgt is not None:
        print(fp64_id(case), mfma, f"row {r0}: q/m = {cf['adv'][r0]:.9g} (target {t:.9g}), rows with e > 100: {above} of {N}, rows within "
              f"their a-priori error of the clamp: {int(bd['near_apriori'].sum())}, of them not settled by the fp32 Q: {int(bd['near'].sum())}")
        if abs(t - AR.LN100) >= 1.0:
            assert not bd["near"][r0]                                    # a row a whole unit (or 85) from the clamp is never in doubt
    got = dict(g, stats=wrote, L_pi=loss[0], L_BC=loss[1])
    ref = dict(grads, stats=cf["stats"], L_pi=cf["L_pi"], L_BC=cf["L_BC"])
    bound = dict(bd["grads"], stats=bd["stats"], L_pi=bd["L_pi"], L_BC=bd["L_BC"])
    name = f"{fp64_id(case)}-{mfma}"
    RATIOS[name] = {k: AR.ratios(got[k], ref[k], bound[k]) for k in ref}
    print(name, {k: f"{v:.3g}" for k, v in RATIOS[name].items()})
    for k in ref:
        FB.check(got[k], ref[k], bound[k], f"{name} {k}")


@pytest.mark.parametrize("lowest", [AR.LN100 + 1e-3, 90.0])
def test_rows_above_the_clamp_are_exact(lowest, mfma, dev):
    """Every row above the clamp, the lowest at q/m = ln 100 + 1e-3 or at 90 (e = inf on every row): the weight is exactly 100 and
    the gradient-through-weight term exactly 0, so the weighted update at bc_coef = 1 must give the BITS of the unweighted one at
    bc_coef = 100.  N_global * A = 256: 2 bc_coef / (N_global A) and its product with 100 are exact, so the two BC terms are
    the same fp32 products; the policy term does not depend on q_weighted.  No NaN anywhere (an e = inf multiplied into the
    seed instead of selected away would put one into every gradient)."""
    S, A, N = 111, 8, 32
    pa, pq, _ = gu.policy_params(77, S, A)
    pq = {k: v.copy() for k, v in pq.items()}
    s, a, _, _, _ = gu.gi.batch(78, N, S, A)
    fw = AR.forward_ref(pa, pq, s, a, 0, 1.0)
    shift = np.float32(1.0 - np.minimum(fw["qp"][0], fw["qp"][1]).min())
    for pre in ("network1.", "network2."):
        pq[pre + "network.4.bias"] = pq[pre + "network.4.bias"] + shift         # min q = 1: every q positive
    fw = AR.forward_ref(pa, pq, s, a, 0, 1.0)
    minq = np.minimum(fw["qp"][0], fw["qp"][1])
    assert abs(minq.min() - 1.0) < 1e-4 and minq.max() < 50
    stats_in = np.array([N * minq.min() / lowest, 0.0])
    base = dict(pa=pa, pq=pq, s=s, act=a, N=N, Ng=N)
    hw = dict(max_action=1.0, weight=2.5, bc_coef=1.0, q_weighted=1)
    hu = dict(max_action=1.0, weight=2.5, bc_coef=100.0, q_weighted=0)
    _, gw, lw, _ = run_td3bc_actor(dict(base, h=hw), mfma, dev, stats_in=stats_in)
    _, gu_, lu, _ = run_td3bc_actor(dict(base, h=hu), mfma, dev, stats_in=stats_in)
    for k in gw:
        assert np.array_equal(gw[k], gu_[k]), k
    np.testing.assert_allclose(lw[1], 100.0 * lu[1], rtol=1e-6)
    np.testing.assert_allclose(lw[0], lu[0], rtol=1e-6)
    cf = TR.closed_forms(fw["pi"], fw["qp"], fw["dqda"], a, hw, N, N, stats=stats_in)
    assert (cf["bcw"] == 100.0).all() and (cf["gw"] == 0).all()
    np.testing.assert_allclose(lw[1], cf["L_BC"], rtol=1e-5)


# ---- 4. a second backward on the same forward ------------------------------------------------------------------------------------
def test_second_backward_gives_the_same_bits(mfma, dev):
    from mobody_amd import ops
    S, A, N = 17, 6, 65
    cfg, scfg = td3_cfg(S, A, advantage=1)
    pa, pq, _ = gu.policy_params(93, S, A)
    b = to_dev(gu.gi.batch(94, N, S, A), dev)
    st = Step(S, A, pa, pq, dev, N, scfg)
    st.run(b, apply=False)
    first = (st.e.ga.clone(), st.e.loss.clone())
    st.e.ga.fill_(float("nan"))
    ops.td3bc_actor_backward(st.dims, st.hyp, st.e.actor, st.e.actor_T, st.e.q, st.e.q_T, b[0], b[1], st.e.stats, st.e.ga,
                             st.e.loss[1:3], st.ws)
    torch.cuda.synchronize()
    assert torch.equal(first[0], st.e.ga) and torch.equal(first[1], st.e.loss)


# ---- 5. two half batches with summed stats ---------------------------------------------------------------------------------------
def test_shards_sum_to_the_whole_batch(mfma, dev):
    from mobody_amd import ops
    S, A, N = 17, 6, 130
    cfg, scfg = td3_cfg(S, A, advantage=1)
    pa, pq, _ = gu.policy_params(95, S, A)
    batch = gu.gi.batch(96, N, S, A)
    full = Step(S, A, pa, pq, dev, N, scfg)
    full.run(to_dev(batch, dev), apply=False)
    parts, stats = [], torch.zeros(2, device=dev)
    for sel in (np.arange(0, N // 2), np.arange(N // 2, N)):
        st = Step(S, A, pa, pq, dev, N // 2, scfg, n_global=N)
        b = to_dev([x[sel] for x in batch], dev)
        e = st.e
        ops.critic_step(st.dims, st.hyp, e.actor, e.q, e.q_T, e.qt, b, e.gq, e.loss[0:1], st.ws, policy_forward=True,
                        actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T)
        ops.td3bc_actor_forward(st.dims, st.hyp, e.actor, e.q, b[0], b[1], e.stats, st.ws, policy_ready=True,
                                actor_blob_T=e.actor_T, q_blob_T=e.q_T)
        stats += e.stats
        parts.append((st, b))
    ga = torch.zeros_like(full.e.ga)
    for st, b in parts:
        e = st.e
        ops.td3bc_actor_backward(st.dims, st.hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], stats, e.ga, e.loss[1:3], st.ws)
        ga += e.ga
    torch.cuda.synchronize()
    close(stats[0], full.e.stats[0], rtol=1e-6, atol=0)
    close(ga, full.e.ga, rtol=1e-5, atol=1e-5 * float(full.e.ga.abs().max()))
    close(sum(float(p[0].e.loss[1]) for p in parts), float(full.e.loss[1]), rtol=1e-5, atol=1e-7)


# ---- 6. the mirror ---------------------------------------------------------------------------------------------------------------
class FixedRows:
    """ReplayBuffer mirror whose index draw is the identity (the fixture run used preset rows); counts the draws."""

    def __init__(self, rows, S, A, dev):
        from mobody_amd.algo import utils
        self.rb = utils.ReplayBuffer(S, A, dev, max_size=len(rows[0]))
        self.rb.convert_D4RL(dict(observations=rows[0], actions=rows[1], next_observations=rows[2],
                                  rewards=rows[3][:, 0], terminals=1.0 - rows[4][:, 0]))
        self.calls = calls = []
        self.rb.draw_indices = lambda n: (calls.append(n), torch.arange(n, dtype=torch.int32, device=dev))[1]


def load_fixture_weights(pol, g, S, A):
    pa, pq, _ = gu.policy_params(int(g["seed"]), S, A)
    pol.policy.load_state_dict({k: torch.from_numpy(v) for k, v in pa.items()})
    pol.q_funcs.load_state_dict({k: torch.from_numpy(v) for k, v in pq.items()})
    pol.target_q_funcs.load_state_dict({k: torch.from_numpy(v) for k, v in pq.items()})


@pytest.mark.parametrize("tag", list(TR.VARIANTS))
def test_mirror_train_vs_reference_fixture(tag, mfma, dev):
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.td3_bc import TD3BC
    g = gu.load(f"g23_td3bc_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = gu.policy_cfg(S, A, **TR.VARIANTS[tag])
    pol = call_algo("TD3_BC", cfg, 3, dev)
    assert isinstance(pol, TD3BC) and pol.total_it == 0
    load_fixture_weights(pol, g, S, A)
    rows_src, rows_tar = TR.g23_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    td = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if tag == "dara":
        pol.classifier.load_state_dict({k: torch.from_numpy(v) for k, v in TR.classifier_params().items()})
    for step in (1, 2):
        if tag == "dara":
            # the mirror keeps the classifier rows in draw order (its loss is a mean over rows): the recorded noise of permuted
            # row i belongs to row perm[i]
            perm = g[f"s{step}_perm"]
            nz = []
            for k in ("noise_sas", "noise_sa"):
                u = np.empty_like(g[f"s{step}_{k}"]); u[perm] = g[f"s{step}_{k}"]; nz.append(td(u))
            pol.classifier_noise_fn = lambda n, nz=nz: tuple(nz)
        pol.train(src.rb, tar.rb, bs, None, None)
        q_loss, pi_loss, _ = pol.losses()
        print(tag, mfma, step, "q_loss", q_loss, float(g["q_loss"][step - 1]), "pi_loss", pi_loss, float(g["pi_loss"][step - 1]))
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        if tag == "dara":
            close(pol._batch[3], g[f"s{step}_reward"], rtol=1e-4, atol=2e-6)
            for k, v in pol.classifier.state_dict().items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_cls_p::{k}"], cfg["actor_lr"], max_frac=0.5)
        for nm, net in (("q", pol.q_funcs), ("actor", pol.policy), ("qt", pol.target_q_funcs)):
            for k, v in net.state_dict().items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
    assert src.calls == list(g["calls_src"]) and tar.calls == list(g["calls_tar"])
    assert pol.total_it == int(g["total_it"]) == 2 and pol.q_optimizer.t == 2 and pol.policy_optimizer.t == 2
    assert pol.fake_replay_buffer.size == 0 and pol.dynamics is None


def test_mirror_gradient_form_equals_fused_form(mfma, dev):
    """config['fused_update'] = 0 (dp.dp_update's engine interface on one rank) gives the fused step's bits."""
    from mobody_amd.algo.call_algo import call_algo
    g = gu.load("g23_td3bc_adv")
    S, A, bs = 17, 6, 32
    rows_src, rows_tar = TR.g23_rows(S, A)
    blobs = []
    for fused in (1, 0):
        pol = call_algo("td3_bc", gu.policy_cfg(S, A, advantage=1, fused_update=fused), 3, dev)
        load_fixture_weights(pol, g, S, A)
        src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
        for _ in range(2):
            pol.train(src.rb, tar.rb, bs, None, None)
        torch.cuda.synchronize()
        blobs.append([x.clone() for x in (pol.q_funcs.blob, pol.target_q_funcs.blob, pol.policy.blob, pol.policy_optimizer.m, pol._loss[:3])])
    for x, y in zip(*blobs):
        assert torch.equal(x, y)


def test_mirror_checkpoint_round_trip_and_keys(mfma, dev, tmp_path):
    from mobody_amd.algo.call_algo import call_algo
    g = gu.load("g23_td3bc_adv")
    S, A, bs = 17, 6, 32
    cfg = gu.policy_cfg(S, A, advantage=1)
    rows_src, rows_tar = TR.g23_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    pol = call_algo("td3_bc", cfg, 3, dev)
    load_fixture_weights(pol, g, S, A)
    for _ in range(2):
        pol.train(src.rb, tar.rb, bs, None, None)
    pol.save(str(tmp_path / "model"))
    assert sorted(os.listdir(tmp_path)) == ["model_actor", "model_actor_optimizer", "model_critic", "model_critic_optimizer"]
    ld = lambda s: torch.load(str(tmp_path / ("model" + s)), map_location="cpu", weights_only=True)
    assert sorted(ld("_actor")) == sorted(f"network.network.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias"))
    assert sorted(ld("_critic")) == sorted(f"network{j}.network.{i}.{w}" for j in (1, 2) for i in (0, 2, 4) for w in ("weight", "bias"))
    assert sorted(ld("_critic_optimizer")) == ["param_groups", "state"] and len(ld("_critic_optimizer")["state"]) == 12
    assert len(ld("_actor_optimizer")["state"]) == 6 and float(ld("_actor_optimizer")["state"][0]["step"]) == 2.0
    fresh = call_algo("td3_bc", cfg, 3, dev)
    fresh.load(str(tmp_path / "model"))
    # the target net is not in the reference's four files: the next step is compared on what they hold
    fresh.target_q_funcs.blob.copy_(pol.target_q_funcs.blob)
    fresh.target_q_funcs.blob_T.copy_(pol.target_q_funcs.blob_T)
    fresh.total_it = pol.total_it
    for p in (pol, fresh):
        p.train(src.rb, tar.rb, bs, None, None)
    torch.cuda.synchronize()
    for a, b in ((pol.q_funcs.blob, fresh.q_funcs.blob), (pol.policy.blob, fresh.policy.blob), (pol.q_optimizer.m, fresh.q_optimizer.m),
                 (pol.policy_optimizer.v, fresh.policy_optimizer.v), (pol._loss[:3], fresh._loss[:3])):
        assert torch.equal(a, b)
    act = pol.select_action(np.zeros(S, np.float32))
    assert isinstance(act, np.ndarray) and act.shape == (A,) and np.abs(act).max() <= 1.0
    before = pol.target_q_funcs.blob.clone()
    pol.update_target()
    want = pol.tau * pol.q_funcs.blob + (1.0 - pol.tau) * before
    assert torch.equal(pol.target_q_funcs.blob, want)


@pytest.mark.parametrize("fused_gather", [1, 0])
def test_graph_replay_equals_eager_steps(fused_gather, mfma, dev, tmp_path):
    """rng='device', config['graph'] = 1: twenty replayed steps equal the same twenty steps enqueued eagerly (the step's own closure
    run outside a capture: the same device counters, the same launches), bit for bit; a load() drops the graph and the next step
    captures it again."""
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task, bs = 17, 6, "walker2d-medium-v2", 64

    def make(graph):
        torch.manual_seed(3)
        cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, advantage=1, fused_gather=fused_gather, trg_ratio=0.5)
        pol = call_algo("td3_bc", cfg, 3, dev)
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, task, 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, task, 1)
        return pol, src, tar

    g, gs, gt = make(1)
    g.train(gs, gt, bs, None, None)                  # step 1 allocates the minibatch: eager
    assert g._graph is None
    for _ in range(20):
        g.train(gs, gt, bs, None, None)
    assert g._graph is not None and g.q_optimizer.t == 21 and g._ctr.tolist()[:3] == [20, 21, 21]
    assert g._gather_in_forward([gs._fields(), gt._fields()]) == bool(fused_gather)
    e, es, et = make(0)
    e.train(es, et, bs, None, None)
    assert e._graph is None
    e._ctr[1], e._ctr[2] = e.q_optimizer.t, e.policy_optimizer.t
    (seg,) = e._graph_segments(es, et, bs, 1, False)
    for _ in range(20):
        seg()
    torch.cuda.synchronize()
    for a, b in ((g.q_funcs.blob, e.q_funcs.blob), (g.target_q_funcs.blob, e.target_q_funcs.blob), (g.policy.blob, e.policy.blob),
                 (g.q_funcs.blob_T, e.q_funcs.blob_T), (g.policy_optimizer.m, e.policy_optimizer.m), (g._ctr, e._ctr),
                 (g._loss[:3], e._loss[:3]), (g._batch[0], e._batch[0])):
        assert torch.equal(a, b)
    assert all(np.isfinite(x) for x in g.losses())
    g.save(str(tmp_path / "m"))
    g.load(str(tmp_path / "m"))
    assert g._graph is None
    g.train(gs, gt, bs, None, None)
    assert g._graph is not None and g.q_optimizer.t == 22


def test_graph_replay_tracks_the_eager_train_path(mfma, dev):
    """The captured step against TD3BC.train() on the EAGER path, twenty steps, the same rows: the buffers carry the seeds of the
    captured step's index streams (seed + 101 / + 102) and the eager object's draw counts are set back after step 1, so that its
    k-th later draw is the replay's call id k.  Not bit for bit: the eager path forms Adam's bias corrections on the host (libm
    pow), the captured one on the device, one ulp of the step size apart (tests/test_hip_mirror.py allows rtol 1e-6 after three
    steps for the same reason).  Held to the per-step allowance of tests/test_hip_train.py (99.5 % of the entries within 1e-5
    relative + 1e-6, every entry within 0.1 lr per step -- entries whose gradient sits at the rounding floor move by O(lr) under
    Adam) accumulated over the twenty steps for the maximum; the figures are printed."""
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task, bs, steps = 17, 6, "walker2d-medium-v2", 64, 20

    def make(graph):
        torch.manual_seed(3)
        cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, advantage=1, trg_ratio=0.5)
        pol = call_algo("td3_bc", cfg, 3, dev)
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=7 + 101), 4000, task, 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=7 + 102), 500, task, 1)
        return pol, src, tar

    g, gs, gt = make(1)
    e, es, et = make(0)
    for p, a, b in ((g, gs, gt), (e, es, et)):
        p.train(a, b, bs, None, None)                # step 1: eager in both, call id 1 of the buffers' own streams
    assert torch.equal(g.policy.blob, e.policy.blob) and torch.equal(g._batch[0], e._batch[0])
    es._draws = et._draws = 0                        # the captured step counts its call ids from 1 again
    for _ in range(steps):
        g.train(gs, gt, bs, None, None)
        e.train(es, et, bs, None, None)
    torch.cuda.synchronize()
    assert g._graph is not None and e._graph is None and g.q_optimizer.t == e.q_optimizer.t == steps + 1
    assert torch.equal(g._batch[0], e._batch[0]) and torch.equal(g._batch[3], e._batch[3])       # the same rows to the end
    lr = e.config["critic_lr"]
    for name, a, b in (("critic", g.q_funcs.blob, e.q_funcs.blob), ("target", g.target_q_funcs.blob, e.target_q_funcs.blob),
                       ("actor", g.policy.blob, e.policy.blob)):
        d = (a.double() - b.double()).abs()
        tight = float((d <= 1e-6 + 1e-5 * b.double().abs()).double().mean())
        print(f"{mfma} {name}: max |replay - eager| = {float(d.max()):.3e} ({float(d.max()) / lr:.3g} lr), within 1e-5: {tight:.5f}")
        assert tight >= 0.995 and float(d.max()) <= steps * 0.1 * lr
    close(g._loss[:3], e._loss[:3], rtol=1e-4, atol=1e-6)


def test_writer_scalars_and_dara_run_eagerly(dev):
    """train/q1 on the reference's cadence (every 5000th step, eagerly); 'dara' never replays."""
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task, bs = 17, 6, "walker2d-medium-v2", 32

    class W:
        def __init__(self):
            self.rows = []

        def add_scalar(self, tag, v, global_step=None, *a):
            self.rows.append((tag, int(global_step), float(v)))

    for pen in ("none", "dara"):
        pol = call_algo("td3_bc", gu.policy_cfg(S, A, rng="device", seed=5, graph=1, penalty_type=pen), 3, dev)
        src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=2000, rng="device", seed=1), 2000, task, 0)
        tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, task, 1)
        w = W()
        r0 = src.reward.clone()
        pol.train(src, tar, bs, w, None)
        pol.train(src, tar, bs, w, None)
        assert (pol._graph is not None) == (pen == "none") and w.rows == []
        pol.total_it = 4999
        pol.train(src, tar, bs, w, None)
        assert pol._graph is None and pol.total_it == 5000
        tags = [t for t, s, _ in w.rows if s == 5000]
        assert "train/q1" in tags and all(np.isfinite(v) for _, _, v in w.rows)
        if pen == "dara":
            assert {"train/sas classifier loss", "train/sa classifier loss", "train/reward penalty"} <= set(tags)
            assert pol.classifier.opt_sa.t == 3
        assert torch.equal(src.reward, r0)            # the penalty goes to the step's rows, never into the buffer


# ---- 7. the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_runs_td3bc_without_dynamics(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.dynamics import mobody_dynamics, mobody_module
    from mobody_amd.algo.offline_offline.td3_bc import TD3BC
    built = []
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: built.append("build_dynamics"))
    for mod, name in ((mobody_dynamics, "MOBODYEnsembleDynamics"), (mobody_module, "MOBODYModule")):
        orig = getattr(mod, name).__init__
        monkeypatch.setattr(getattr(mod, name), "__init__", lambda self, *a, _o=orig, _n=name, **k: (built.append(_n), _o(self, *a, **k))[1])
    pol = tm.main(["--policy", "TD3_BC", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                   "--synthetic", "1", "--rng", "device", "--src_rows", "3000", "--tar_rows", "600", "--max_step", "12",
                   "--save-model", "--eval_freq", "6", "--log_every", "4", "--advantage", "1", "--dir", str(tmp_path),
                   "--params", json.dumps(dict(batch_size=64, graph=1))])
    assert isinstance(pol, TD3BC) and pol.total_it == 12 and pol.dynamics is None and built == []
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3
    for ln in lines:
        assert all(np.isfinite(float(ln.split(k)[1].split()[0])) for k in ("q_loss ", "pi_loss ", "bc_loss "))
    models = tmp_path / "TD3_BC" / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "models"
    assert sorted(os.listdir(models)) == ["model_actor", "model_actor_optimizer", "model_critic", "model_critic_optimizer"]
    pol.load(str(models / "model"))
    assert pol.q_optimizer.t == 12
    csv = (models.parent / "tb" / "scalars.csv").read_text()
    assert "model error" not in csv


def test_two_rank_job_is_refused_before_any_collective(tmp_path):
    """Data-parallel TD3_BC is not built: under the project's launcher both ranks raise in the constructor -- before the first
    collective -- and the job ends with that message instead of waiting in one."""
    from test_cli_dp import _launcher
    r = _launcher(str(tmp_path), ["--policy", "TD3_BC"], timeout=120)
    assert r.returncode != 0
    assert "NotImplementedError" in r.stderr and "data-parallel TD3_BC is not built" in r.stderr, r.stderr[-3000:]
    assert "step 6:" not in r.stdout and not os.path.exists(os.path.join(str(tmp_path), "logs", "TD3_BC"))


# ---- 8. refusals: MOBODY_E_ARG, the field named, nothing launched ------------------------------------------------------------------
def test_refusals_launch_nothing(dev):
    from mobody_amd import _lib, ops
    S, A, N = 17, 6, 40
    cfg, scfg = td3_cfg(S, A, advantage=1)
    pa, pq, _ = gu.policy_params(97, S, A)
    st = Step(S, A, pa, pq, dev, N, scfg)
    b = to_dev(gu.gi.batch(98, N, S, A), dev)
    e = st.e
    bad = [(ops.train_dims(S, A, N, N - 8, N, N - 8), st.hyp, None, "d.Nt"), (ops.train_dims(S, A, N, N, 2 * N, N), st.hyp, None, "d.Nt_global"),
           (st.dims, st.hyp, torch.zeros(N, device=dev), "v_true"),
           (st.dims, ops.hyper(dict(scfg, scale_Q=0)), None, "h.scale_q"),
           (ops.train_dims(S, 25, N, N, N, N), st.hyp, None, "d.A 25 > 24")]       # (the seed spreads A <= 24 columns over eight lanes)
    for dims, hyp, v_true, word in bad:
        for entry in ("mobody_td3bc_actor_forward", "mobody_td3bc_actor_backward"):
            e.stats.fill_(float("nan")); e.ga.fill_(float("nan")); e.loss.fill_(float("nan"))
            blk = ops._actor_block(dims, hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], e.stats, st.ws)
            blk.v_true, blk.grad_actor, blk.loss_out = _lib.ptr(v_true), _lib.ptr(e.ga), _lib.ptr(e.loss[1:3])
            rc = getattr(_lib.load(), entry)(C.byref(blk), _lib.cur_stream())
            msg = _lib.load().mobody_last_error().decode()
            torch.cuda.synchronize()
            assert rc == -1 and msg.startswith(entry + ":") and word in msg, (rc, msg)
            assert bool(torch.isnan(e.stats).all()) and bool(torch.isnan(e.ga).all()) and bool(torch.isnan(e.loss).all())
