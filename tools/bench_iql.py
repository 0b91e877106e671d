#!/usr/bin/env python
"""IQL step benchmark (one GPU): ms per `IQL.train()` step at walker2d shapes (S = 17, A = 6), next to -- alternating in the same
process --

  composed  the same step composed from the entry points that existed before the IQL ones: mlp3_forward + value_loss_grad (its
            expectile is the literal 0.7, the benchmark's lam) + mlp3_backward + adam_polyak for V; mlp3_forward + mobody_critic
            with q_next for Q; mlp3_forward + the advantage-weighted seed in torch element-wise ops (no entry point forms it) +
            mlp3_backward + adam_polyak for the policy.  The generic entries are exact fp32 whatever `mfma` says, so only the
            critic of this leg follows the mode; under replay its policy runs at the constant rate (its Adam launch takes a host rate)
  torch     a PyTorch-eager restatement of the IQL step on the same GPU (tensors + autograd + torch.optim.Adam +
            CosineAnnealingLR, index draws by torch.randint on the device); eager legs only

for bs in {128 (the reference's default), 4096} x mfma in {f16x2, f32} x {graph replay, eager}.  Each leg is timed `--repeats` times
(`--steps` steps between two device synchronisations, after `--warmup` steps of that leg), the legs alternating; medians and the
min / max spread of each are reported.  Results: one JSON document (`--out`, default profiles/iql_step.json) with the build's source
fingerprint; keys already in that file that this tool does not write are kept.

  python tools/bench_iql.py [--bs 128 4096] [--mfma f16x2 f32] [--steps 300] [--warmup 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S, A, TASK = 17, 6, "walker2d-medium-v2"
CFG = dict(gamma=0.99, tau=0.005, update_interval=2, state_dim=S, action_dim=A, hidden_sizes=256, max_action=1.0, critic_lr=3e-4,
           actor_lr=3e-4, lam=0.7, temp=3.0, max_step=500000)


def composed_class():
    import torch
    from mobody_amd import ops
    from mobody_amd.algo.offline_offline.iql import IQL
    from mobody_amd.algo.offline_offline.mobody import _Adam, _PackedNet

    class ComposedIQL(IQL):
        """IQL.train with `_update` put together from the entry points that existed before mobody_iql_*."""

        def __init__(self, config, device):
            IQL.__init__(self, config, device)
            S_, A_ = self.S, self.A
            self.v_func = _PackedNet(S_, 1, 1, ("network.",), self.device)                 # the generic entries: exact fp32
            self.v_optimizer = _Adam(self.v_func, config["critic_lr"])
            self.policy.precision = 0
            ops.mlp_transpose(self.policy.blob, S_, 2 * A_, 1, out=self.policy.blob_T, precision=0)
            self._pws = self._vws = None

        def _update(self, b, N, Nt, dev=False, log=False):
            S_, A_, c = self.S, self.A, self._ctr
            dims, hyp = self._dims(N, N, N, N)
            ov, oq, op = self.v_optimizer, self.q_optimizer, self.policy_optimizer
            if not dev:
                oq.t += 1                                   # (_Adam.step counts V's and the policy's steps itself)
            qt = ops.mlp3_forward(self.target_q_funcs.blob, S_ + A_, 1, 2, b[0], b[1])
            v, x, h1, h2 = ops.mlp3_forward(self.v_func.blob, S_, 1, 1, b[0], save=True)
            dz3, loss = ops.value_loss_grad(qt.view(2, N), v.view(N), N)
            adv = torch.minimum(qt.view(2, N)[0], qt.view(2, N)[1]) - v.view(N)
            self._vws = ops.mlp3_backward(self.v_func.blob_T, S_, 1, 1, dz3, x, h1, h2, ov.grad, self._vws)
            if dev:
                ov.step_dev(c[3:4])
            else:
                ov.step()
            q_next = ops.mlp3_forward(self.v_func.blob, S_, 1, 1, b[2]).view(N)
            ops.critic_update(dims, hyp, self.policy.blob, self.q_funcs.blob, self.q_funcs.blob_T, self.target_q_funcs.blob, b, oq.m, oq.v,
                              oq.t, oq.lr, self._loss[0:1], self._ws, q_next=q_next, t_dev=c[1:2] if dev else None,
                              qtarg_blob_T=self.target_q_funcs.blob_T, bump=c[0:1] if dev else None)
            z, x, h1, h2 = ops.mlp3_forward(self.policy.blob, S_, 2 * A_, 1, b[0], save=True)
            th = torch.tanh(z.view(N, 2 * A_)[:, :A_])
            w = torch.exp(self.temp * adv).clamp(max=100.0)[:, None]
            dz = torch.zeros(N, 16, device=self.device)
            dz[:, :A_] = 2.0 * w * (th - b[1]) * (1.0 - th * th) / (N * A_)
            self._pws = ops.mlp3_backward(self.policy.blob_T, S_, 2 * A_, 1, dz, x, h1, h2, op.grad, self._pws)
            if dev:
                op.step_dev(c[2:3])
            else:
                lr0 = op.lr
                op.lr = self.policy_lr_schedule.lr_of_step(op.t + 1)
                op.step()
                op.lr = lr0
    return ComposedIQL


def make_legs(dev, bs, mfma, graph, buffers):
    import numpy as np
    import torch
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    cfg = dict(CFG, rng="device", seed=0, batch_size=bs, graph=graph, mfma=mfma)
    torch.manual_seed(0); np.random.seed(0)
    iql = call_algo("iql", dict(cfg), 3, dev)
    comp = composed_class()(dict(cfg), dev)
    legs = {"iql": lambda: iql.train(src, tar, bs, None, None), "composed": lambda: comp.train(src, tar, bs, None, None)}
    if not graph:
        legs["torch"] = torch_step(dev, bs, src, tar)
    return legs, iql, comp


def torch_step(dev, bs, src, tar, lr=3e-4, gamma=0.99, tau=0.005, lam=0.7, temp=3.0, T_max=500000):
    """One IQL step (src(bs) | tar(bs); V, Q + Polyak, policy under the cosine schedule) in eager PyTorch on the device."""
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
    t1, t2 = [x.detach().clone() for x in q1], [x.detach().clone() for x in q2]
    opt_q, opt_v, opt_p = torch.optim.Adam(q1 + q2, lr=lr), torch.optim.Adam(vf, lr=lr), torch.optim.Adam(pol, lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt_p, T_max)
    fields = [(rb.state, rb.action, rb.next_state, rb.reward, rb.not_done) for rb in (src, tar)]
    sizes = [int(src.size), int(tar.size)]

    def step():
        idx = [torch.randint(0, n, (bs,), device=dev, generator=g) for n in sizes]
        s, a, s2, r, nd = (torch.cat([f[k][i] for f, i in zip(fields, idx)], 0) for k in range(5))
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


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 4096])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--graph", type=int, nargs="+", default=[1, 0])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src_rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iql_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_iql.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.src_rows, rng="device", seed=100), args.src_rows, TASK, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=5000, rng="device", seed=200), 5000, TASK, 1000)
    runs = []
    for bs in args.bs:
        for mfma in args.mfma:
            for graph in args.graph:
                legs, iql, comp = make_legs(dev, bs, mfma, graph, (src, tar))
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                assert (iql._graph is not None) == bool(graph) and (comp._graph is not None) == bool(graph)
                ms = {k: [] for k in legs}
                for _ in range(args.repeats):
                    for k, fn in legs.items():            # alternating: every repeat times each leg once
                        ms[k].append(timed(fn, args.steps))
                assert all(x == x for x in iql.losses()), "non-finite losses"
                rec = dict(bs=bs, N=2 * bs, mfma=mfma, graph=graph)
                for k, v in ms.items():
                    rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
                rec["iql_minus_composed_ms"] = rec["iql"]["median_ms"] - rec["composed"]["median_ms"]
                rec["no_slower_than_composed"] = rec["iql_minus_composed_ms"] <= rec["composed"]["spread_ms"]
                runs.append(rec)
                print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"})
                                  for k, v in rec.items()}), flush=True)
    doc = dict(what="ms per train() step, walker2d shapes S=17 A=6: IQL (mobody_iql_value / _critic / _actor) | the same step composed "
                    "from the earlier entry points | PyTorch-eager IQL restatement; medians over alternating repeats",
               launches=dict(iql_step="12 (4 per phase: forward, backward with the seed, weight gradients, reduce + Adam) + the gather",
                             iql_dependent_chain="8 (V's four, then Q's four; the policy's four hang off V's backward)",
                             composed_step="19 library launches + the torch element-wise launches of the policy seed and adv"),
               src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, src_rows=args.src_rows, runs=runs)
    if os.path.exists(args.out):
        try:
            old = json.load(open(args.out))
            doc.update({k: v for k, v in old.items() if k not in doc})      # records this tool does not write are kept
        except (OSError, ValueError):
            pass
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        runs_ = doc.pop("runs")                               # one line per run
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(r) for r in runs_) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
