#!/usr/bin/env python
"""DARA step benchmark (one GPU): ms per `DARA.train()` step at walker2d shapes (S = 17, A = 6) under graph replay, next to --
alternating in the same process --

  iql        the bare IQL step (`IQL.train()`, graph replay): what DARA's step adds to is dara - iql
  composed   the same DARA step with the classifier update and the relabel put together from what existed before the
             mobody_dara_classifier / mobody_dara_relabel entry points: MOBODY.update_classifier (k_dara_inputs, two unpaired
             exact-fp32 forwards, k_dara_loss + k_dara_loss_final, per head mobody_mlp3_backward and a separate Adam launch) and
             MOBODY._dara_delta (k_dara_inputs, two forwards, k_dara_penalty).  Host-side call and step counters: it cannot be
             captured, so this leg runs eagerly (its IQL phases too); `dara_eager` is the new step run the same way
  torch      a PyTorch-eager restatement of the DARA step on the same GPU (tensors + autograd + torch.optim.Adam)

and the classifier update + relabel alone on a fixed batch: `cls_fused_replay` (gather + mobody_dara_classifier + mobody_dara_relabel
as one captured graph, device counters), `cls_fused_eager`, `cls_composed_eager`.

for bs in {256, 4096} x mfma in {f16x2, f32}.  Each leg is timed `--repeats` times (`--steps` steps between two device
synchronisations, after `--warmup` steps of that leg), the legs alternating; medians and the min / max spread are reported.  Results:
one JSON document (`--out`, default profiles/dara_step.json) with the build's source fingerprint.

  python tools/bench_dara.py [--bs 256 4096] [--mfma f16x2 f32] [--steps 200] [--warmup 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_iql import CFG as IQL_CFG, S, A, TASK, timed  # noqa: E402

CFG = dict(IQL_CFG, gaussian_noise_std=1.0, eta=0.1, dara_eta=0)
LAUNCHES = dict(
    classifier_fused="8: k_dara_inputs, one paired forward, per head the backward with seed mode 7, the weight-gradient launch and "
                     "the reduce + Adam launch (2 x 3)",
    relabel_fused="2: one paired forward reading state | action | next_state in place, k_dara_penalty",
    classifier_composed="13: k_dara_inputs, 2 forwards, k_dara_loss, k_dara_loss_final, per head backward + weight gradients + "
                        "reduce (3) and k_adam (1)",
    relabel_composed="4: k_dara_inputs, 2 forwards, k_dara_penalty",
    dara_step="the classifier-batch gather + 8 + the training-batch gather + 2 + IQL's 12",
)


def composed_class():
    from mobody_amd.algo.offline_offline.dara import DARA
    from mobody_amd.algo.offline_offline.mobody import MOBODY, _Classifier

    class ComposedDARA(DARA):
        """DARA.train with the classifier update and the relabel from the entry points that existed before (exact-fp32 heads)."""

        def __init__(self, config, device):
            DARA.__init__(self, config, device)
            self.old = _Classifier(self.S, self.A, self.device, config["gaussian_noise_std"], config["actor_lr"])
            self.classifier_keep, self.classifier = self.classifier, self.old      # MOBODY's methods read self.classifier

        def _classifier_step(self, cb, N, dev=False, noise=None):
            assert not dev
            MOBODY.update_classifier(self, None, None, N // 2, rows=(cb[0], cb[1], cb[2]), noise=noise)

        def _relabel(self, b, N, log=False):
            n = N // 2
            r = b[3][:n]
            MOBODY._dara_delta(self, b[0][:n], b[1][:n], b[2][:n], r, self.eta)
    return ComposedDARA


def torch_step(dev, bs, src, tar, lr=3e-4, gamma=0.99, tau=0.005, lam=0.7, temp=3.0, T_max=500000, std=1.0, eta=0.1):
    """One DARA step (classifier update on a batch of its own, relabel, IQL's three phases) in eager PyTorch on the device."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device=dev); g.manual_seed(0)

    def mlp_params(i, o):
        ps = []
        for a, b in ((i, 256), (256, 256), (256, o)):
            bound = a ** -0.5
            ps += [torch.empty(b, a, device=dev).uniform_(-bound, bound, generator=g).requires_grad_(True),
                   torch.empty(b, device=dev).uniform_(-bound, bound, generator=g).requires_grad_(True)]
        return ps

    def mlp(p, x):
        return F.linear(torch.relu(F.linear(torch.relu(F.linear(x, p[0], p[1])), p[2], p[3])), p[4], p[5])

    pol, vf, q1, q2 = mlp_params(S, 2 * A), mlp_params(S, 1), mlp_params(S + A, 1), mlp_params(S + A, 1)
    c_sa, c_sas = mlp_params(S + A, 2), mlp_params(2 * S + A, 2)
    t1, t2 = [x.detach().clone() for x in q1], [x.detach().clone() for x in q2]
    opt_q, opt_v, opt_p = torch.optim.Adam(q1 + q2, lr=lr), torch.optim.Adam(vf, lr=lr), torch.optim.Adam(pol, lr=lr)
    opt_c = torch.optim.Adam(c_sa + c_sas, lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt_p, T_max)
    fields = [(rb.state, rb.action, rb.next_state, rb.reward, rb.not_done) for rb in (src, tar)]
    sizes = [int(src.size), int(tar.size)]
    label = torch.cat([torch.zeros(bs), torch.ones(bs)]).long().to(dev)

    def draw():
        idx = [torch.randint(0, n, (bs,), device=dev, generator=g) for n in sizes]
        return tuple(torch.cat([f[k][i] for f, i in zip(fields, idx)], 0) for k in range(5))

    def heads(s, a, s2, noise):
        sas, sa = torch.cat([s, a, s2], 1), torch.cat([s, a], 1)
        if noise:
            sas = sas + std * torch.randn(sas.shape, device=dev, generator=g)
            sa = sa + std * torch.randn(sa.shape, device=dev, generator=g)
        return torch.softmax(mlp(c_sas, sas), 1), torch.softmax(mlp(c_sa, sa), 1)

    def step():
        s, a, s2, _, _ = draw()
        p_sas, p_sa = heads(s, a, s2, True)
        c_loss = F.cross_entropy(p_sas, label) + F.cross_entropy(p_sa, label)
        opt_c.zero_grad(); c_loss.backward(); opt_c.step()
        s, a, s2, r, nd = draw()
        with torch.no_grad():
            p_sas, p_sa = heads(s[:bs], a[:bs], s2[:bs], False)
            ls, la = torch.log(torch.softmax(p_sas, 1) + 1e-10), torch.log(torch.softmax(p_sa, 1) + 1e-10)
            pen = (ls[:, 1:] - la[:, 1:] - ls[:, :1] + la[:, :1]).clamp(-10, 10)
            r = torch.cat([r[:bs] + eta * pen, r[bs:]], 0)
        x = torch.cat([s, a], 1)
        with torch.no_grad():
            q_t = torch.min(mlp(t1, x), mlp(t2, x))
        adv = q_t - mlp(vf, s)
        v_loss = torch.mean(torch.abs(lam - (adv < 0).float()) * adv ** 2)
        opt_v.zero_grad(); v_loss.backward(); opt_v.step()
        with torch.no_grad():
            y = r + nd * gamma * mlp(vf, s2)
        q_loss = F.mse_loss(mlp(q1, x), y) + F.mse_loss(mlp(q2, x), y)
        opt_q.zero_grad(); q_loss.backward(); opt_q.step()
        with torch.no_grad():
            for t, p in zip(t1 + t2, q1 + q2):
                t.copy_(tau * p + (1.0 - tau) * t)
        w = torch.exp(temp * adv.detach()).clamp(max=100.0)
        pi_loss = torch.mean(w * (torch.tanh(mlp(pol, s)[:, :A]) - a) ** 2)
        opt_p.zero_grad(); pi_loss.backward(); opt_p.step(); sched.step()
    return step


def make_legs(dev, bs, mfma, buffers):
    import numpy as np
    import torch
    from mobody_amd import ops
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    cfg = dict(CFG, rng="device", seed=0, batch_size=bs, mfma=mfma)
    torch.manual_seed(0); np.random.seed(0)
    dara = call_algo("dara", dict(cfg, graph=1), 3, dev)
    iql = call_algo("iql", dict({k: v for k, v in cfg.items() if k not in ("gaussian_noise_std", "eta", "dara_eta")}, graph=1), 3, dev)
    dara_e = call_algo("dara", dict(cfg, graph=0), 3, dev)
    comp = composed_class()(dict(cfg, graph=0), dev)
    tr = lambda p: (lambda: p.train(src, tar, bs, None, None))
    legs = {"dara": tr(dara), "iql": tr(iql), "dara_eager": tr(dara_e), "composed": tr(comp), "torch": torch_step(dev, bs, src, tar)}
    # the classifier update + relabel alone, on the rows the first steps left in the objects' batches
    for fn in (legs["dara_eager"], legs["composed"]):
        fn()
    N = 2 * bs
    cls_f = call_algo("dara", dict(cfg, graph=0), 3, dev)
    cls_f.train(src, tar, bs, None, None)
    c = cls_f._ctr

    def fused_eager():
        cls_f._classifier_step(cls_f._cbatch, N)
        cls_f._relabel(cls_f._batch, N)

    def fused_dev():
        ops.gather_batch_rng(buffers=[rb._fields() for rb in (src, tar)], counts=[bs, bs], call_offsets=[1, 1], counter=c[0:1],
                             sizes=[rb.ptr_size[1:2] for rb in (src, tar)], S=S, A=A, seeds=[cls_f._seed_for(104), cls_f._seed_for(105)],
                             out=cls_f._cbatch, bump=(c[4:5],))
        cls_f._classifier_step(cls_f._cbatch, N, dev=True)
        cls_f._relabel(cls_f._batch, N)
    c[4] = cls_f.classifier_optimizer.t
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused_dev()

    def composed_eager():
        comp._classifier_step(comp._cbatch, N)
        comp._relabel(comp._batch, N)
    legs.update(cls_fused_replay=graph.replay, cls_fused_eager=fused_eager, cls_composed_eager=composed_eager)
    return legs, dara, iql, (dara_e, comp, cls_f, graph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src_rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dara_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_dara.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.src_rows, rng="device", seed=100), args.src_rows, TASK, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=5000, rng="device", seed=200), 5000, TASK, 1000)
    runs = []
    for bs in args.bs:
        for mfma in args.mfma:
            legs, dara, iql, keep = make_legs(dev, bs, mfma, (src, tar))
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            assert dara._graph is not None and iql._graph is not None and keep[0]._graph is None and keep[1]._graph is None
            ms = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, fn in legs.items():                # alternating: every repeat times each leg once
                    ms[k].append(timed(fn, args.steps))
            assert all(x == x for x in dara.losses() + dara.classifier_losses()), "non-finite losses"
            rec = dict(bs=bs, N=2 * bs, mfma=mfma)
            for k, v in ms.items():
                rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
            med = lambda k: rec[k]["median_ms"]
            rec["classifier_fused_in_step_ms"] = med("dara") - med("iql")                 # what the replayed step pays for DARA's additions
            rec["classifier_composed_in_step_ms"] = med("composed") - (med("dara_eager") - med("cls_fused_eager"))
            rec["composed_today_ms"] = med("iql") + med("cls_composed_eager")             # the replayed IQL step + the eager old pieces
            rec["cls_fused_over_composed"] = med("cls_fused_replay") / med("cls_composed_eager")
            rec["cls_fused_eager_over_composed"] = med("cls_fused_eager") / med("cls_composed_eager")
            rec["dara_over_composed_today"] = med("dara") / rec["composed_today_ms"]
            rec["fused_faster_than_composed"] = bool(med("cls_fused_replay") < med("cls_composed_eager")
                                                     and med("cls_fused_eager") < med("cls_composed_eager"))
            runs.append(rec)
            print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"})
                              for k, v in rec.items()}), flush=True)
            del legs, dara, iql, keep
    doc = dict(what="ms per step, walker2d shapes S=17 A=6: DARA.train (graph replay) | bare IQL.train (graph replay) | DARA eager | the "
                    "same step with the classifier update + relabel composed from the earlier entry points (eager: not capturable) | "
                    "PyTorch-eager DARA restatement | the classifier update + relabel alone (fused replay / fused eager / composed "
                    "eager); medians over alternating repeats",
               launches=LAUNCHES, src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), steps=args.steps,
               warmup=args.warmup, repeats=args.repeats, src_rows=args.src_rows, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        runs_ = doc.pop("runs")                               # one line per run
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(r) for r in runs_) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
