"""The IQL baseline on the GPU: the three C-ABI entry points mobody_iql_value / _critic / _actor (BwdSeed modes 5 and 6: the
expectile seed of the V net and the advantage-weighted regression seed of the policy net, the cosine learning rate of the fused
policy step), the mirror class IQL and the CLI, against the reference's g24 fixtures (tests/golden/make_golden_iql.py), fp64 per
element and exact integer probes.

Tolerances: those tests/test_hip_td3bc.py applies to G23 (written at each assert); the per-element part takes the bounds of
tests/iql_ref.py value_bounds / policy_bounds.  Every case uses N <= 257 rows.
"""
import json
import os

import numpy as np
import pytest
import torch

import actor_ref as AR
import f64_bounds as FB
import golden_util as gu
import iql_ref as IR
from test_hip_train import close, params_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Net:
    """One packed net on the device with its T blob, Adam moments and gradient blob."""

    def __init__(self, p, in_dim, out_dim, members, dev, mode):
        from mobody_amd import ops, packing
        prefixes = ["network1.", "network2."] if members == 2 else ["network."]
        self.dims = (in_dim, out_dim, members)
        self.blob = packing.pack_mlp(p, in_dim, out_dim, dev, prefixes=prefixes)
        self.blob_T = ops.mlp_transpose(self.blob, in_dim, out_dim, members, precision=mode)
        self.am, self.av, self.grad = torch.zeros_like(self.blob), torch.zeros_like(self.blob), torch.zeros_like(self.blob)
        self.prefixes = prefixes

    def copy(self):
        c = object.__new__(Net)
        c.__dict__ = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.__dict__.items()}
        return c

    def unpack(self, blob):
        from mobody_amd import packing
        out = {}
        for pre, m in zip(self.prefixes, packing.unpack_mlp(blob.clone(), *self.dims)):
            out.update({pre + k: v.cpu().numpy() for k, v in m.items()})
        return out

    def adam(self, t, lr, mode, target=None, tau=-1.0):
        from mobody_amd import ops
        i, o, m = self.dims
        ops.adam_polyak(i, o, m, self.blob, self.blob_T, self.grad, self.am, self.av, None if target is None else target.blob, t, lr, tau,
                        target_T=None if target is None else target.blob_T, precision=mode)


def hyper_of(cfg, mode):
    from mobody_amd import ops
    return ops.hyper(dict(gamma=cfg["gamma"], tau=cfg["tau"], max_action=cfg["max_action"], weight=0.0, bc_coef=0.0, q_weighted=0,
                          scale_Q=0, mfma=mode))


class Step:
    """mobody_iql_value -> _critic -> _actor on one set of blobs, in the gradient form (+ mobody_adam_polyak) or the fused form."""

    def __init__(self, S, A, pa, pq, pv, dev, N, cfg, mode, n_global=None):
        from mobody_amd import ops
        self.S, self.A, self.cfg, self.mode = S, A, cfg, mode
        self.v, self.q, self.pi = Net(pv, S, 1, 1, dev, mode), Net(pq, S + A, 1, 2, dev, mode), Net(pa, S, 2 * A, 1, dev, mode)
        self.qt = self.q.copy()
        ng = n_global or N
        self.dims, self.hyp = ops.train_dims(S, A, N, N, ng, ng), hyper_of(cfg, mode)
        self.ws = ops.iql_workspace(self.dims, dev)
        self.adv = torch.full((N + 1,), float("nan"), device=dev)
        self.loss = torch.zeros(4, device=dev)
        self.log = torch.zeros(2, device=dev)
        self.t = 0

    def head(self, b):
        c = self.cfg
        return (self.dims, self.hyp, c["lam"], c["temp"], c["max_step"], (self.v, self.q, self.qt, self.pi), b, self.adv[:-1])

    def run(self, b, fused=False):
        from mobody_amd import ops
        c, mode = self.cfg, self.mode
        self.t += 1
        t, h = self.t, self.head(b)
        if fused:
            ops.iql_value(*h, self.loss[3:4], self.ws, m=self.v.am, v=self.v.av, t=t, lr=c["critic_lr"], log_out=self.log)
            ops.iql_critic(*h, self.loss[0:1], self.ws, m=self.q.am, v=self.q.av, t=t, lr=c["critic_lr"])
            ops.iql_actor(*h, self.loss[1:2], self.ws, m=self.pi.am, v=self.pi.av, t=t, lr=c["actor_lr"])
        else:
            ops.iql_value(*h, self.loss[3:4], self.ws, grad=self.v.grad, log_out=self.log)
            self.v.adam(t, c["critic_lr"], mode)
            ops.iql_critic(*h, self.loss[0:1], self.ws, grad=self.q.grad)
            self.q.adam(t, c["critic_lr"], mode, target=self.qt, tau=c["tau"])
            ops.iql_actor(*h, self.loss[1:2], self.ws, grad=self.pi.grad)
            self.pi.adam(t, ops.cosine_lr(c["actor_lr"], t, c["max_step"]), mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.adv[-1])), "the sentinel behind adv was overwritten"


def to_dev(batch, dev):
    return [torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous() for x in batch]


def logstd_rows(d, A):
    """The logstd half of an unpacked policy blob: rows A .. 2A of the output layer's weight and bias."""
    return np.concatenate([d["network.network.4.weight"][A:].reshape(-1), d["network.network.4.bias"][A:].reshape(-1)])


# ---- 1. the C ABI against the fixtures; fused == gradient form + mobody_adam_polyak; the logstd half keeps its bits ------------
@pytest.mark.parametrize("tag", list(IR.VARIANTS))
def test_c_abi_vs_reference_fixture(tag, mfma, dev):
    g = gu.load(f"g24_iql_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = IR.iql_cfg(S, A, **IR.VARIANTS[tag])
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    b = to_dev(IR.g24_batch(bs, S, A), dev)
    N = b[0].shape[0]
    assert N == 64
    ref, fus = Step(S, A, pa, pq, pv, dev, N, cfg, mfma), Step(S, A, pa, pq, pv, dev, N, cfg, mfma)
    short = tag == "short"
    ls0 = logstd_rows(ref.pi.unpack(ref.pi.blob), A)
    for step in range(1, IR.STEPS[tag] + 1):
        ref.run(b)
        fus.run(b, fused=True)
        q_loss, pi_loss, v_loss = float(ref.loss[0]), float(ref.loss[1]), float(ref.loss[3])
        print(tag, mfma, step, "v_loss", v_loss, float(g["v_loss"][step - 1]), "q_loss", q_loss, float(g["q_loss"][step - 1]), "pi_loss",
              pi_loss, float(g["pi_loss"][step - 1]))
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        adv = ref.adv[:-1].cpu().numpy()
        close(adv, g[f"s{step}_adv"], rtol=1e-5, atol=1e-5)
        close(float(ref.log[0]), g[f"s{step}_adv"].astype(np.float64).mean(), rtol=1e-5, atol=1e-5)      # train/adv (N_global = N)
        if not short:
            for nm, net in (("v", ref.v), ("q", ref.q), ("actor", ref.pi)):
                ks = [k for k in g if k.startswith(f"s{step}_{nm}_g::")]
                scale = max(float(np.abs(g[k]).max()) for k in ks)
                for k, v in net.unpack(net.grad).items():
                    close(gu.sub(v), g[f"s{step}_{nm}_g::{k}"], rtol=1e-5, atol=1e-5 * scale)
            for nm, net in (("v", ref.v), ("q", ref.q), ("qt", ref.qt)):
                for k, v in net.unpack(net.blob).items():
                    params_close(gu.sub(v), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
        for k, v in ref.pi.unpack(ref.pi.blob).items():                      # `short`: the six policy states of the schedule
            params_close(gu.sub(v), g[f"s{step}_actor_p::{k}"], cfg["actor_lr"])
        for name in ("v", "q", "qt", "pi"):
            for part in ("blob", "blob_T", "am", "av"):
                assert torch.equal(getattr(getattr(ref, name), part), getattr(getattr(fus, name), part)), (step, name, part)
        assert torch.equal(ref.loss, fus.loss) and torch.equal(ref.adv[:-1], fus.adv[:-1]) and torch.equal(ref.log, fus.log)
        # the logstd half: exactly zero gradient, zero moments, the initial bits
        assert not logstd_rows(ref.pi.unpack(ref.pi.grad), A).any()
        for net in (ref.pi, fus.pi):
            assert not logstd_rows(net.unpack(net.am), A).any() and not logstd_rows(net.unpack(net.av), A).any()
            assert np.array_equal(logstd_rows(net.unpack(net.blob), A), ls0)
    if short:                                                               # the schedule moved the policy: the constant rate would not do
        assert ref.t == 6


# ---- 2. exact probes: integer nets, power-of-two scalars, bit for bit against the fp64 closed forms ---------------------------
@pytest.mark.parametrize("S,A,N,gmul", [(11, 4, 33, 1), (17, 8, 65, 2), (45, 32, 31, 1), (17, 2, 257, 2)])
def test_exact_probe_equals_closed_forms_bit_for_bit(S, A, N, gmul, mfma, dev):
    """mu = 0 (th = 0, 1 - th^2 = 1), integer actions, temp * adv in {-128, 0, 128} so that w is 0, 1 or 100 exactly (expf
    underflows to 0 / overflows to inf), lam = 3/4, N_global a power of two, A a power of two: every term of every gradient is
    an integer multiple of one power of two, and every sum is exact in any order."""
    from mobody_amd import ops
    seed = 7 * S + A + N
    rng = np.random.default_rng(seed)
    Ng = gmul * AR.pow2ceil(N)
    s = rng.integers(-3, 4, (N, S)).astype(np.float32)
    act = rng.integers(-2, 3, (N, A)).astype(np.float32)
    cfg = IR.iql_cfg(S, A, lam=0.75, temp=128.0, max_step=8)
    hyp, dims = hyper_of(cfg, mfma), ops.train_dims(S, A, N, N, Ng, Ng)
    ws = ops.iql_workspace(dims, dev)
    b = to_dev((s, act, s, np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32)), dev)
    # ---- policy: adv handed in ----
    pa = AR.int_nets(S, 2 * A, seed)[0]
    adv = np.resize(np.array([0.0, 1.0, -1.0], np.float32), N)
    rng.shuffle(adv[1:])
    fw = IR.net_forward(pa, "network.", s)
    assert not fw["z3"].any()
    cf = IR.awr_seed(fw["z3"], act, adv, 128.0, Ng)
    with np.errstate(under="ignore", over="ignore"):
        w32 = np.minimum(np.exp(np.float32(128.0) * adv, dtype=np.float32), np.float32(100.0))
    assert set(np.unique(w32)) <= {0.0, 1.0, 100.0} and 1.0 in w32 and (N < 3 or {0.0, 100.0} <= set(np.unique(w32)))
    cf["w"] = w32.astype(np.float64)                                         # e^-128 is 0 in fp32 (2.6e-56 in fp64): the kernel's exact value
    cf["dz3"][:, :A] = 2.0 * cf["w"][:, None] * cf["df"] / (Ng * A)
    cf["L_pi"] = float((cf["w"][:, None] * cf["df"] ** 2).sum() / (Ng * A))
    grads, tape = IR.grads_ref(pa, s, fw, cf["dz3"])
    quantum = 2.0 / (Ng * A)
    ax = {0: np.abs(s.astype(np.float64)), 2: np.maximum(fw["z1"], 0), 4: np.maximum(fw["z2"], 0)}
    for i in (0, 2, 4):
        adz = np.abs(tape[f"network.network.{i}"][0]["dz"])
        assert AR.dyadic_ok(grads[f"network.network.{i}.weight"], adz.T @ ax[i], quantum) and AR.dyadic_ok(grads[f"network.network.{i}.bias"], adz.sum(0), quantum)
    assert AR.f16_bits_ok(dict(fw=fw), dict(tape=tape))
    pi = Net(pa, S, 2 * A, 1, dev, mfma)
    n = pi.blob.numel()
    buf = torch.full((n + 4,), float("nan"), device=dev)
    advd = torch.full((N + 1,), float("nan"), device=dev)
    advd[:N] = torch.from_numpy(adv).to(dev)
    ops.iql_actor(dims, hyp, 0.75, 128.0, 8, (pi, pi, pi, pi), b, advd[:N], buf[n + 1:n + 2], ws, grad=buf[:n])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n])) and bool(torch.isnan(buf[n + 2])) and bool(torch.isnan(advd[N]))
    got = pi.unpack(buf[:n])
    for k, ref in grads.items():
        assert np.array_equal(got[k].astype(np.float64), ref), (mfma, "policy", k, float(np.abs(got[k] - ref).max()))
    assert float(buf[n + 1]) == cf["L_pi"]
    # ---- V: V(s) = 0 by construction, adv = min target-Q(s, a), integers ----
    pv = AR.int_nets(S, 1, seed + 1)[0]
    pq = AR.int_nets(S, A, seed + 2)[1]
    fv = IR.net_forward(pv, "network.", s)
    x = np.concatenate([s, act], 1)
    qt = np.stack([IR.net_forward(pq, pre, x)["z3"][:, 0] for pre in ("network1.", "network2.")])
    assert not fv["z3"].any() and np.array_equal(qt, np.rint(qt))
    cv = IR.expectile_seed(qt, fv["z3"][:, 0], 0.75, Ng)
    assert (cv["adv"] < 0).any() and (cv["adv"] >= 0).any()
    gv, tv = IR.grads_ref(pv, s, fv, cv["dz3"][:, None])
    qv = 0.5 / Ng
    ax = {0: np.abs(s.astype(np.float64)), 2: np.maximum(fv["z1"], 0), 4: np.maximum(fv["z2"], 0)}
    for i in (0, 2, 4):
        adz = np.abs(tv[f"network.network.{i}"][0]["dz"])
        assert AR.dyadic_ok(gv[f"network.network.{i}.weight"], adz.T @ ax[i], qv) and AR.dyadic_ok(gv[f"network.network.{i}.bias"], adz.sum(0), qv)
    assert AR.f16_bits_ok(dict(fw=fv), dict(tape=tv))
    vn, qn = Net(pv, S, 1, 1, dev, mfma), Net(pq, S + A, 1, 2, dev, mfma)
    n = vn.blob.numel()
    buf = torch.full((n + 7,), float("nan"), device=dev)
    advd.fill_(float("nan"))
    ops.iql_value(dims, hyp, 0.75, 128.0, 8, (vn, qn, qn, pi), b, advd[:N], buf[n + 1:n + 2], ws, grad=buf[:n], log_out=buf[n + 3:n + 5])
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(buf[k])) for k in (n, n + 2, n + 5, n + 6)) and bool(torch.isnan(advd[N]))
    got = vn.unpack(buf[:n])
    for k, ref in gv.items():
        assert np.array_equal(got[k].astype(np.float64), ref), (mfma, "value", k, float(np.abs(got[k] - ref).max()))
    assert np.array_equal(advd[:N].cpu().numpy().astype(np.float64), cv["adv"])
    assert float(buf[n + 1]) == cv["L_V"] and float(buf[n + 3]) == cv["adv_mean"] and float(buf[n + 4]) == 0.0


# ---- 3. per element against fp64 -------------------------------------------------------------------------------------------------
SA = [(11, 3), (17, 6), (45, 24), (111, 8)]
NS = [1, 31, 32, 33, 65, 257]
TEMP = 3.0
CLAMP_X = (("ln100+1e-3", IR.LN100 + 1e-3), ("ln100-1e-3", IR.LN100 - 1e-3), ("ln100+1", IR.LN100 + 1.0), ("ln100-1", IR.LN100 - 1.0),
           ("+90", 90.0), ("-90", -90.0))
PI_KINDS = ("plain", "all_neg", "all_pos", "clamp", "tile_scale")
# (kind, (S, A), N, N_global / N, clamp target or None): every kind at every (S, A) and N; the clamp kind once per target
PI_CASES = [(kind, sa, N, 1 + (i + j + k) % 2, tgt) for i, kind in enumerate(PI_KINDS) for j, sa in enumerate(SA) for k, N in enumerate(NS)
            for tgt in (CLAMP_X if kind == "clamp" else (None,))]
V_KINDS = ("plain", "all_neg", "all_pos")
V_CASES = [(kind, sa, N, 1 + (i + j + k) % 2, (0.5, 0.7, 0.9)[(i + j + k) % 3]) for i, kind in enumerate(V_KINDS) for j, sa in enumerate(SA)
           for k, N in enumerate(NS)]
RATIOS = {}


def pi_id(c):
    return f"pi-{c[0]}-S{c[1][0]}A{c[1][1]}-N{c[2]}-g{c[3]}" + (f"-x={c[4][0]}" if c[4] else "")


def v_id(c):
    return f"v-{c[0]}-S{c[1][0]}A{c[1][1]}-N{c[2]}-g{c[3]}-lam{c[4]}"


@pytest.fixture(scope="module", autouse=True)
def bounds_file():
    yield
    path = os.environ.get("MOBODY_IQL_BOUNDS_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            # one line per case and mode: the ratios in the order of `tensors` (the policy's seven, then V's ten)
            keys = {ph: sorted(next(v for k, v in RATIOS.items() if k.startswith(ph))) for ph in ("pi-", "v-") if any(k.startswith(ph) for k in RATIOS)}
            f.write('{"what": "worst |got - fp64| / bound per tensor, tests/test_hip_iql.py part 3",\n "tensors": %s,\n "cases": {\n' % json.dumps(keys))
            f.write(",\n".join('  %s: %s' % (json.dumps(n), json.dumps([float("%.3g" % r[k]) for k in keys[n[:n.index("-") + 1]]]))
                               for n, r in sorted(RATIOS.items())))
            f.write("\n }}\n")


_PI_REF = {}


def pi_reference(case):
    """Inputs, fp64 closed forms and gradients of a policy case (shared by the f32 and the f16x2 run)."""
    if case in _PI_REF:
        return _PI_REF[case]
    kind, (S, A), N, gmul, tgt = case
    idx = PI_CASES.index(case)
    seed = 1300 + 17 * idx
    rng = np.random.default_rng(seed)
    pa = IR.iql_params(S, A, seed)[0]
    pool = max(4 * N, 64)
    s, act, _, _, _ = gu.gi.batch(seed + 5, pool, S, A)
    keep = np.flatnonzero(IR.robust(pa, "network.", s))
    assert keep.size >= N, (keep.size, N)
    s, act = s[keep[:N]].copy(), act[keep[:N]].copy()
    adv = rng.standard_normal(N).astype(np.float32)
    if kind == "all_neg":
        adv = -np.abs(adv) - np.float32(0.1)
    elif kind == "all_pos":
        adv = np.abs(adv) + np.float32(0.1)
    elif kind == "tile_scale":
        adv = (adv * np.where((np.arange(N) // 32) % 2 == 0, 2.0 ** 12, 2.0 ** -12)).astype(np.float32)
    r0 = None
    if tgt is not None:
        r0 = idx % N                                 # the target row rotates with the case
        adv[r0] = np.float32(tgt[1] / TEMP)
    Ng = gmul * N
    fw = IR.net_forward(pa, "network.", s)
    cf = IR.awr_seed(fw["z3"], act, adv, TEMP, Ng)
    grads, tape = IR.grads_ref(pa, s, fw, cf["dz3"])
    _PI_REF.clear()
    _PI_REF[case] = out = dict(pa=pa, s=s, act=act, adv=adv, Ng=Ng, fw=fw, cf=cf, grads=grads, tape=tape, r0=r0)
    return out


@pytest.mark.parametrize("case", PI_CASES, ids=pi_id)
def test_policy_phase_vs_fp64_bounds(case, mfma, dev):
    """mobody_iql_actor (gradient form) with the advantages handed in.  Clamp cases put ONE rotating row at the signed target
    temp * adv; the inputs leave no row within its a-priori error of the clamp (asserted: count 0), and the fp32 restatement of
    e takes the fp64 side on every row."""
    from mobody_amd import ops
    kind, (S, A), N, gmul, tgt = case
    c = pi_reference(case)
    cf, Ng = c["cf"], c["Ng"]
    assert int(IR.clamp_unresolved(cf, TEMP).sum()) == 0
    with np.errstate(over="ignore", under="ignore"):
        e32 = np.exp(np.float32(TEMP) * c["adv"], dtype=np.float32)
    assert np.array_equal(e32 > 100, cf["e"] > 100)
    if kind == "all_neg":
        assert (c["adv"] < 0).all()
    if kind == "all_pos":
        assert (c["adv"] > 0).all()
    if tgt is not None:
        t = tgt[1]
        assert abs(cf["x"][c["r0"]] - t) <= 1e-6 * abs(t) and (cf["e"][c["r0"]] > 100) == (t > IR.LN100)
    cfg = IR.iql_cfg(S, A, temp=TEMP)
    hyp, dims = hyper_of(cfg, mfma), ops.train_dims(S, A, N, N, Ng, Ng)
    ws = ops.iql_workspace(dims, dev)
    pi = Net(c["pa"], S, 2 * A, 1, dev, mfma)
    n = pi.blob.numel()
    buf = torch.full((n + 3,), float("nan"), device=dev)
    s, act = torch.from_numpy(c["s"]).to(dev).contiguous(), torch.from_numpy(c["act"]).to(dev).contiguous()
    advd = torch.from_numpy(c["adv"]).to(dev).contiguous()
    ops.iql_actor(dims, hyp, 0.7, TEMP, 8, (pi, pi, pi, pi), (s, act, s, advd, advd), advd, buf[n + 1:n + 2], ws, grad=buf[:n])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[n])) and bool(torch.isnan(buf[n + 2])) and bool(torch.isfinite(buf[:n]).all())
    g = pi.unpack(buf[:n])
    assert not logstd_rows(g, A).any()                                       # exactly zero, not merely small
    bd = IR.policy_bounds(c["pa"], c["s"], c["act"], c["adv"], TEMP, N, Ng, c["fw"], cf, c["tape"], mfma == "f16x2")
    got, ref, bound = dict(g, L_pi=float(buf[n + 1])), dict(c["grads"], L_pi=cf["L_pi"]), dict(bd["grads"], L_pi=bd["L_pi"])
    name = f"{pi_id(case)}-{mfma}"
    RATIOS[name] = {k: AR.ratios(got[k], ref[k], bound[k]) for k in ref}
    print(name, {k: f"{v:.3g}" for k, v in RATIOS[name].items()})
    for k in ref:
        FB.check(got[k], ref[k], bound[k], f"{name} {k}")


_V_REF = {}


def v_reference(case):
    if case in _V_REF:
        return _V_REF[case]
    kind, (S, A), N, gmul, lam = case
    lam = float(np.float32(lam))                     # lam as the kernel holds it
    idx = V_CASES.index(case)
    seed = 2100 + 17 * idx
    _, pq, pv = IR.iql_params(S, A, seed, q_scale=4.0)
    pool = max(6 * N, 96)
    s, act, _, _, _ = gu.gi.batch(seed + 5, pool, S, A)
    x = np.concatenate([s, act], 1)
    ok = IR.robust(pv, "network.", s) & IR.robust(pq, "network1.", x) & IR.robust(pq, "network2.", x)

    def forms(rows, pv):
        fv = IR.net_forward(pv, "network.", s[rows])
        qt = np.stack([IR.net_forward(pq, pre, x[rows])["z3"][:, 0] for pre in ("network1.", "network2.")])
        return fv, qt, IR.expectile_seed(qt, fv["z3"][:, 0], lam, gmul * N)
    allr = np.arange(pool)
    fv, qt, cf = forms(allr, pv)
    # V's output bias centres the advantages on their median (plain: both signs occur) or moves every one of them to one side
    pv = {k: v.copy() for k, v in pv.items()}
    shift = np.float32(np.abs(cf["adv"]).max() + 1.0)
    pv["network.network.4.bias"] = pv["network.network.4.bias"] + (np.float32(np.median(cf["adv"])) if kind == "plain" else
                                                                     shift if kind == "all_neg" else -shift)
    fv, qt, cf = forms(allr, pv)
    # rows whose advantage keeps its sign under the forward error of both nets (the weight |lam - 1[adv < 0]| is then exact)
    gr, tp = IR.grads_ref(pv, s, fv, cf["dz3"][:, None])
    Eadv = IR.value_bounds(pv, pq, s, act, lam, pool, gmul * N, fv, cf, tp, True)["adv"]
    keep = np.flatnonzero(ok & (np.abs(cf["adv"]) > 2 * Eadv))
    assert keep.size >= N, (keep.size, N)
    rows = keep[:N]
    fv, qt, cf = forms(rows, pv)
    grads, tape = IR.grads_ref(pv, s[rows], fv, cf["dz3"][:, None])
    _V_REF.clear()
    _V_REF[case] = out = dict(pv=pv, pq=pq, s=s[rows].copy(), act=act[rows].copy(), Ng=gmul * N, fv=fv, cf=cf, grads=grads, tape=tape)
    return out


@pytest.mark.parametrize("case", V_CASES, ids=v_id)
def test_value_phase_vs_fp64_bounds(case, mfma, dev):
    """mobody_iql_value (gradient form): adv, L_V, the two logged means and V's gradients.  lam rotates over 0.5, 0.7, 0.9."""
    from mobody_amd import ops
    kind, (S, A), N, gmul, lam = case
    c = v_reference(case)
    lam = float(np.float32(lam))
    cf, Ng = c["cf"], c["Ng"]
    if kind == "all_neg":
        assert (cf["adv"] < 0).all()
    if kind == "all_pos":
        assert (cf["adv"] > 0).all()
    if kind == "plain" and N >= 31:
        assert (cf["adv"] < 0).any() and (cf["adv"] > 0).any()
    cfg = IR.iql_cfg(S, A, lam=lam)
    hyp, dims = hyper_of(cfg, mfma), ops.train_dims(S, A, N, N, Ng, Ng)
    ws = ops.iql_workspace(dims, dev)
    vn, qn = Net(c["pv"], S, 1, 1, dev, mfma), Net(c["pq"], S + A, 1, 2, dev, mfma)
    n = vn.blob.numel()
    buf = torch.full((n + 6,), float("nan"), device=dev)
    advd = torch.full((N + 1,), float("nan"), device=dev)
    s, act = torch.from_numpy(c["s"]).to(dev).contiguous(), torch.from_numpy(c["act"]).to(dev).contiguous()
    ops.iql_value(dims, hyp, lam, 3.0, 8, (vn, qn, qn, vn), (s, act, s, advd, advd), advd[:N], buf[n + 1:n + 2], ws,
                  grad=buf[:n], log_out=buf[n + 3:n + 5])
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(buf[k])) for k in (n, n + 2, n + 5)) and bool(torch.isnan(advd[N])) and bool(torch.isfinite(buf[:n]).all())
    g = vn.unpack(buf[:n])
    bd = IR.value_bounds(c["pv"], c["pq"], c["s"], c["act"], lam, N, Ng, c["fv"], cf, c["tape"], mfma == "f16x2")
    got = dict(g, adv=advd[:N].cpu().numpy(), L_V=float(buf[n + 1]), adv_mean=float(buf[n + 3]), v_mean=float(buf[n + 4]))
    ref = dict(c["grads"], adv=cf["adv"], L_V=cf["L_V"], adv_mean=cf["adv_mean"], v_mean=cf["v_mean"])
    bound = dict(bd["grads"], adv=bd["adv"], L_V=bd["L_V"], adv_mean=bd["adv_mean"], v_mean=bd["v_mean"])
    name = f"{v_id(case)}-{mfma}"
    RATIOS[name] = {k: AR.ratios(got[k], ref[k], bound[k]) for k in ref}
    print(name, {k: f"{v:.3g}" for k, v in RATIOS[name].items()})
    for k in ref:
        FB.check(got[k], ref[k], bound[k], f"{name} {k}")


# ---- 4. the mirror ---------------------------------------------------------------------------------------------------------------
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
    pa, pq, pv = IR.iql_params(S, A, int(g["seed"]), float(g["q_scale"]))
    t = lambda p: {k: torch.from_numpy(v) for k, v in p.items()}
    pol.policy.load_state_dict(t(pa)); pol.q_funcs.load_state_dict(t(pq)); pol.target_q_funcs.load_state_dict(t(pq))
    pol.v_func.load_state_dict(t(pv))
    return pa


@pytest.mark.parametrize("tag", list(IR.VARIANTS))
def test_mirror_train_vs_reference_fixture(tag, mfma, dev):
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.offline_offline.iql import IQL
    g = gu.load(f"g24_iql_{tag}")
    S, A, bs = int(g["S"]), int(g["A"]), int(g["bs"])
    cfg = IR.iql_cfg(S, A, **IR.VARIANTS[tag])
    pol = call_algo("IQL", cfg, 3, dev)
    assert isinstance(pol, IQL) and pol.total_it == 0 and pol.policy_lr_schedule.last_epoch == 0
    pa = load_fixture_weights(pol, g, S, A)
    rows_src, rows_tar = IR.g24_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    short = tag == "short"
    for step in range(1, IR.STEPS[tag] + 1):
        close(pol.policy_lr_schedule.get_last_lr()[0], g["lr"][step - 1], rtol=2e-7, atol=0)      # the rate of the coming step
        pol.train(src.rb, tar.rb, bs, None, None)
        q_loss, pi_loss, v_loss = pol.losses()
        close(v_loss, g["v_loss"][step - 1], rtol=1e-5, atol=0)
        close(q_loss, g["q_loss"][step - 1], rtol=1e-5, atol=0)
        close(pi_loss, g["pi_loss"][step - 1], rtol=5e-5, atol=2e-5)
        nets = (("actor", pol.policy),) if short else (("v", pol.v_func), ("q", pol.q_funcs), ("qt", pol.target_q_funcs), ("actor", pol.policy))
        for nm, net in nets:
            for k, v in net.state_dict().items():
                params_close(gu.sub(v.cpu().numpy()), g[f"s{step}_{nm}_p::{k}"], cfg["critic_lr"])
    n = IR.STEPS[tag]
    assert src.calls == list(g["calls_src"]) and tar.calls == list(g["calls_tar"])
    assert pol.total_it == int(g["total_it"]) == n and [o.t for o in (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer)] == [n] * 3
    assert pol.policy_lr_schedule.last_epoch == int(g["last_epoch"]) and pol.fake_replay_buffer.size == 0 and pol.dynamics is None
    sd = pol.policy.state_dict()                                             # the logstd half: the initial bits
    for k in ("network.network.4.weight", "network.network.4.bias"):
        assert np.array_equal(sd[k].cpu().numpy()[A:], pa[k][A:])
    a = pol.select_action(rows_src[0][0])
    mu = pol.policy.mu_logstd(torch.from_numpy(rows_src[0][:1]).to(dev))[0, :A]
    assert a.shape == (A,) and np.allclose(a, (torch.tanh(mu) * cfg["max_action"]).cpu().numpy(), atol=1e-6)
    assert pol.select_action(rows_src[0][0], test=False).shape == (A,)


def test_mirror_gradient_form_equals_fused_form(mfma, dev):
    """config['fused_update'] = 0 (gradient blobs + mobody_adam_polyak at the scheduled rate) gives the fused step's bits."""
    from mobody_amd.algo.call_algo import call_algo
    g = gu.load("g24_iql_short")
    S, A, bs = 17, 6, 32
    rows_src, rows_tar = IR.g24_rows(S, A)
    blobs = []
    for fused in (1, 0):
        pol = call_algo("iql", dict(IR.iql_cfg(S, A, max_step=8), fused_update=fused), 3, dev)
        load_fixture_weights(pol, g, S, A)
        src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
        for _ in range(3):
            pol.train(src.rb, tar.rb, bs, None, None)
        torch.cuda.synchronize()
        blobs.append([x.clone() for x in (pol.q_funcs.blob, pol.target_q_funcs.blob, pol.v_func.blob, pol.policy.blob, pol.policy_optimizer.m,
                                          pol.policy_optimizer.v, pol._loss)])
    for x, y in zip(*blobs):
        assert torch.equal(x, y)


FILES = ["model_actor", "model_actor_lr_scheduler", "model_actor_optimizer", "model_critic", "model_critic_optimizer", "model_value",
         "model_value_optimizer"]


def test_mirror_checkpoint_round_trip_and_keys(mfma, dev, tmp_path):
    from mobody_amd.algo.call_algo import call_algo
    g = gu.load("g24_iql_short")
    S, A, bs = 17, 6, 32
    cfg = IR.iql_cfg(S, A, max_step=8)
    rows_src, rows_tar = IR.g24_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)
    a = call_algo("iql", cfg, 3, dev)
    load_fixture_weights(a, g, S, A)
    for _ in range(3):
        a.train(src.rb, tar.rb, bs, None, None)
    a.save(str(tmp_path / "model"))
    assert sorted(os.listdir(tmp_path)) == FILES
    ld = lambda s: torch.load(str(tmp_path / ("model" + s)), map_location="cpu", weights_only=True)
    assert sorted(ld("_actor")) == sorted(f"network.network.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias"))
    assert ld("_actor")["network.network.4.weight"].shape == (2 * A, 256) and ld("_value")["network.network.4.weight"].shape == (1, 256)
    sched = ld("_actor_lr_scheduler")
    assert (sched["T_max"], sched["last_epoch"], sched["base_lrs"], sched["eta_min"]) == (8, 3, [cfg["actor_lr"]], 0)
    opt = ld("_actor_optimizer")
    assert opt["param_groups"][0]["initial_lr"] == cfg["actor_lr"] and abs(opt["param_groups"][0]["lr"] - IR.cosine_lr(3e-4, 4, 8)) < 1e-10
    # the files load into torch's own optimizer / scheduler (what the reference's load_state_dict calls do)
    ps = [torch.nn.Parameter(torch.zeros_like(v)) for v in ld("_actor").values()]
    topt = torch.optim.Adam(ps, lr=cfg["actor_lr"])
    tsch = torch.optim.lr_scheduler.CosineAnnealingLR(topt, 8)
    topt.load_state_dict(opt); tsch.load_state_dict(sched)
    assert tsch.last_epoch == 3 and abs(topt.param_groups[0]["lr"] - IR.cosine_lr(3e-4, 4, 8)) < 1e-10
    b = call_algo("iql", cfg, 3, dev)
    b.load(str(tmp_path / "model"))
    assert [o.t for o in (b.v_optimizer, b.q_optimizer, b.policy_optimizer)] == [3, 3, 3] and b.policy_optimizer.lr == cfg["actor_lr"]
    b.target_q_funcs.load_state_dict(a.target_q_funcs.state_dict())           # (the reference's files hold no target net)
    for p, q in ((a, b),):
        for _ in range(2):
            p.train(src.rb, tar.rb, bs, None, None)
            q.train(src.rb, tar.rb, bs, None, None)
    for x, y in ((a.policy.blob, b.policy.blob), (a.q_funcs.blob, b.q_funcs.blob), (a.v_func.blob, b.v_func.blob), (a.policy_optimizer.v, b.policy_optimizer.v)):
        assert torch.equal(x, y)


def test_update_target_and_logged_scalars(dev):
    from mobody_amd import ops
    from mobody_amd.algo.call_algo import call_algo
    g = gu.load("g24_iql_default")
    S, A, bs = 17, 6, 32
    pol = call_algo("iql", IR.iql_cfg(S, A), 3, dev)
    load_fixture_weights(pol, g, S, A)
    rows_src, rows_tar = IR.g24_rows(S, A)
    src, tar = FixedRows(rows_src, S, A, dev), FixedRows(rows_tar, S, A, dev)

    class W:
        def __init__(self):
            self.rows = {}

        def add_scalar(self, k, v, global_step=None):
            self.rows[k] = float(v)
    w = W()
    pol.total_it = 4999
    pol.train(src.rb, tar.rb, bs, w, None)
    adv = g["s1_adv"].astype(np.float64)
    assert sorted(w.rows) == ["train/adv", "train/q1", "train/value"]
    close(w.rows["train/adv"], adv.mean(), rtol=1e-5, atol=1e-5)
    assert np.isfinite(w.rows["train/value"]) and np.isfinite(w.rows["train/q1"])
    t0 = pol.target_q_funcs.blob.clone()
    pol.update_target()
    assert torch.equal(pol.target_q_funcs.blob, pol.tau * pol.q_funcs.blob + (1.0 - pol.tau) * t0)


# ---- 5. graph replay ---------------------------------------------------------------------------------------------------------------
def _make(graph, dev, seeds=(1, 2)):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    S, A, task = 17, 6, "walker2d-medium-v2"
    torch.manual_seed(3)
    cfg = dict(IR.iql_cfg(S, A, max_step=40), rng="device", seed=7, graph=graph)
    pol = call_algo("iql", cfg, 3, dev)
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=seeds[0]), 4000, task, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=seeds[1]), 500, task, 1)
    return pol, src, tar


def test_graph_replay_equals_eager_steps(mfma, dev, tmp_path):
    """rng='device', config['graph'] = 1, T_max = 40 (the rate moves visibly): twenty replayed steps equal the same twenty steps
    enqueued eagerly (the step's own closure run outside a capture: the same device counters, the same launches), bit for bit; a
    load() drops the graph and the next step captures it again."""
    bs = 64
    g, gs, gt = _make(1, dev)
    g.train(gs, gt, bs, None, None)                  # step 1 allocates the minibatch: eager
    assert g._graph is None
    for _ in range(20):
        g.train(gs, gt, bs, None, None)
    assert g._graph is not None and g._ctr.tolist() == [20, 21, 21, 21]
    assert [o.t for o in (g.v_optimizer, g.q_optimizer, g.policy_optimizer)] == [21, 21, 21] and g.policy_lr_schedule.last_epoch == 21
    e, es, et = _make(0, dev)
    e.train(es, et, bs, None, None)
    assert e._graph is None
    e._ctr[1], e._ctr[2], e._ctr[3] = e.q_optimizer.t, e.policy_optimizer.t, e.v_optimizer.t
    (seg,) = e._graph_segments(es, et, bs, 1, False)
    for _ in range(20):
        seg()
    torch.cuda.synchronize()
    for a, b in ((g.q_funcs.blob, e.q_funcs.blob), (g.target_q_funcs.blob, e.target_q_funcs.blob), (g.policy.blob, e.policy.blob),
                 (g.v_func.blob, e.v_func.blob), (g.policy.blob_T, e.policy.blob_T), (g.policy_optimizer.m, e.policy_optimizer.m),
                 (g._ctr, e._ctr), (g._loss, e._loss), (g._batch[0], e._batch[0]), (g._adv, e._adv)):
        assert torch.equal(a, b)
    assert all(np.isfinite(x) for x in g.losses())
    g.save(str(tmp_path / "m"))
    g.load(str(tmp_path / "m"))
    assert g._graph is None
    g.train(gs, gt, bs, None, None)
    assert g._graph is not None and g.policy_optimizer.t == 22


def test_graph_replay_tracks_the_eager_train_path(mfma, dev):
    """The captured step against IQL.train() on the EAGER path, twenty steps, the same rows (buffers seeded as the captured step's
    index streams, the eager object's draw counts set back after step 1).  Not bit for bit: the eager path forms Adam's bias
    corrections and the cosine rate on the host (libm pow / cos), the captured one on the device.  Held to the per-step allowance of
    tests/test_hip_train.py (99.5 % of the entries within 1e-5 relative + 1e-6, every entry within 0.1 lr per step); printed."""
    bs, steps = 64, 20
    g, gs, gt = _make(1, dev, seeds=(7 + 101, 7 + 102))
    e, es, et = _make(0, dev, seeds=(7 + 101, 7 + 102))
    for p, a, b in ((g, gs, gt), (e, es, et)):
        p.train(a, b, bs, None, None)
    assert torch.equal(g.policy.blob, e.policy.blob) and torch.equal(g._batch[0], e._batch[0])
    es._draws = et._draws = 0
    for _ in range(steps):
        g.train(gs, gt, bs, None, None)
        e.train(es, et, bs, None, None)
    torch.cuda.synchronize()
    assert g._graph is not None and e._graph is None and g.policy_optimizer.t == e.policy_optimizer.t == steps + 1
    assert torch.equal(g._batch[0], e._batch[0]) and torch.equal(g._batch[3], e._batch[3])
    lr = e.config["critic_lr"]
    for name, a, b in (("critic", g.q_funcs.blob, e.q_funcs.blob), ("target", g.target_q_funcs.blob, e.target_q_funcs.blob),
                       ("value", g.v_func.blob, e.v_func.blob), ("policy", g.policy.blob, e.policy.blob)):
        d = (a.double() - b.double()).abs()
        tight = float((d <= 1e-6 + 1e-5 * b.double().abs()).double().mean())
        print(f"{mfma} {name}: max |replay - eager| = {float(d.max()):.3e} ({float(d.max()) / lr:.3g} lr), within 1e-5: {tight:.5f}")
        assert tight >= 0.995 and float(d.max()) <= steps * 0.1 * lr
    close(g._loss, e._loss, rtol=1e-4, atol=1e-6)


# ---- 6. the CLI, the launcher ------------------------------------------------------------------------------------------------------
def test_cli_runs_iql_without_dynamics(tmp_path, capsys, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.iql import IQL
    built = []
    monkeypatch.setattr(tm, "build_dynamics", lambda *a, **k: built.append("build_dynamics"))
    pol = tm.main(["--policy", "IQL", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1",
                   "--synthetic", "1", "--rng", "device", "--src_rows", "3000", "--tar_rows", "600", "--max_step", "12",
                   "--save-model", "--eval_freq", "6", "--log_every", "4", "--dir", str(tmp_path),
                   "--params", json.dumps(dict(batch_size=64, graph=1))])
    assert isinstance(pol, IQL) and pol.total_it == 12 and pol.dynamics is None and built == [] and pol.T_max == 12
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3
    for ln in lines:
        assert all(np.isfinite(float(ln.split(k)[1].split()[0])) for k in ("q_loss ", "pi_loss ", "v_loss "))
    models = tmp_path / "IQL" / "walker2d-friction-srcdatatype-medium-tardatatype-medium-2.0" / "r1" / "models"
    assert sorted(os.listdir(models)) == FILES
    pol.load(str(models / "model"))
    assert pol.policy_optimizer.t == 12 and bool(torch.isfinite(pol.policy.blob).all())


def test_two_rank_job_is_refused_before_any_collective(tmp_path):
    """Data-parallel IQL is not built: under the project's launcher both ranks raise in the constructor -- before the first
    collective -- and the job ends with that message instead of waiting in one."""
    from test_cli_dp import _launcher
    r = _launcher(str(tmp_path), ["--policy", "IQL"], timeout=120)
    assert r.returncode != 0
    assert "NotImplementedError" in r.stderr and "data-parallel IQL is not built" in r.stderr, r.stderr[-3000:]
    assert "step 6:" not in r.stdout
