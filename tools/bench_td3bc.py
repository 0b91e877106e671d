#!/usr/bin/env python
"""TD3_BC step benchmark (one GPU): ms per `TD3BC.train()` step at walker2d shapes (S = 17, A = 6), next to -- alternating in the
same process --

  mobody   the MOBODY step at the same N with q_weighted=0, fake_batch_scale=0, penalty_type='none': what the TD3_BC step launches
           plus N twin-Q forward rows (Q(s_t, a_t)); at trg_ratio 1 a batch size of 4096 gives N = 8192 for both
  torch    a PyTorch-eager restatement of the TD3_BC step on the same GPU (nn-free: tensors + autograd + torch.optim.Adam, index
           draws by torch.randint on the device), the way tools/bench_pretrain.py --mopo has one

for bs in {4096, 256} x mfma in {f16x2, f32} x {graph replay, eager}.  Each leg is timed `--repeats` times (`--steps` steps between two
device synchronisations, after `--warmup` steps of that leg), the legs alternating; medians and the min / max spread of each are
reported.  Results: one JSON document (`--out`, default profiles/td3bc_step.json) with the build's source fingerprint; keys
already in that file that this tool does not write (the bench.py records against the parent commit) are kept.

  python tools/bench_td3bc.py [--bs 4096 256] [--mfma f16x2 f32] [--steps 300] [--warmup 50] [--repeats 5] [--advantage 1]
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


def make_legs(dev, bs, mfma, graph, advantage, buffers):
    import numpy as np
    import torch
    from mobody_amd import engine
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    common = dict(rng="device", seed=0, batch_size=bs, graph=graph, mfma=mfma, penalty_type="none", src_rollout_length=0,
                  trg_rollout_length=0, use_src_sa_to_get_target_next_state=0)
    torch.manual_seed(0); np.random.seed(0)
    td3 = call_algo("td3_bc", engine.default_config(S, A, advantage=advantage, **common), 3, dev)
    mob = call_algo("mobody", engine.default_config(S, A, q_weighted=0, fake_batch_scale=0, **common), 3, dev)
    legs = {"td3bc": lambda: td3.train(src, tar, bs, None, None), "mobody": lambda: mob.train(src, tar, bs, None, None)}
    if not graph:                                     # the restatement has no replay form: timed beside the eager legs only
        legs["torch"] = torch_step(dev, bs, advantage, src, tar)
    return legs, td3, mob


def torch_step(dev, bs, advantage, src, tar, lr=3e-4, gamma=0.99, tau=0.005, weight=2.5, bc_coef=1.0, max_action=1.0):
    """One TD3_BC step (src(bs) | tar(bs), critic + Adam + Polyak, actor + Adam) in eager PyTorch on the device."""
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

    actor, q1, q2 = mlp_params(S, A), mlp_params(S + A, 1), mlp_params(S + A, 1)
    t1, t2 = [x.detach().clone() for x in q1], [x.detach().clone() for x in q2]
    opt_q, opt_a = torch.optim.Adam(q1 + q2, lr=lr), torch.optim.Adam(actor, lr=lr)
    fields = [(rb.state, rb.action, rb.next_state, rb.reward, rb.not_done) for rb in (src, tar)]
    sizes = [int(src.size), int(tar.size)]

    def step():
        idx = [torch.randint(0, n, (bs,), device=dev, generator=g) for n in sizes]
        s, a, s2, r, nd = (torch.cat([f[k][i] for f, i in zip(fields, idx)], 0) for k in range(5))
        with torch.no_grad():
            x2 = torch.cat([s2, max_action * torch.tanh(mlp(actor, s2))], 1)
            y = r + nd * gamma * torch.min(mlp(t1, x2), mlp(t2, x2))
        x = torch.cat([s, a], 1)
        q_loss = F.mse_loss(mlp(q1, x), y) + F.mse_loss(mlp(q2, x), y)
        opt_q.zero_grad(); q_loss.backward(); opt_q.step()
        with torch.no_grad():
            for t, p in zip(t1 + t2, q1 + q2):
                t.copy_(tau * p + (1.0 - tau) * t)
        for p in q1 + q2:
            p.requires_grad_(False)
        pi = max_action * torch.tanh(mlp(actor, s))
        xp = torch.cat([s, pi], 1)
        qv = torch.min(mlp(q1, xp), mlp(q2, xp))
        m = qv.abs().mean().detach()
        sq = (pi - a) ** 2
        bc = (torch.exp(qv / m).clamp(max=100.0) * sq if advantage == 1 else sq).mean()
        loss = weight / m * (-qv).mean() + bc_coef * bc
        opt_a.zero_grad(); loss.backward(); opt_a.step()
        for p in q1 + q2:
            p.requires_grad_(True)
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
    ap.add_argument("--bs", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--graph", type=int, nargs="+", default=[1, 0])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--advantage", type=int, default=1)
    ap.add_argument("--src_rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td3bc_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_td3bc.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
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
                legs, td3, mob = make_legs(dev, bs, mfma, graph, args.advantage, (src, tar))
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                assert (td3._graph is not None) == bool(graph) and (mob._graph is not None) == bool(graph)
                ms = {k: [] for k in legs}
                for _ in range(args.repeats):
                    for k, fn in legs.items():            # alternating: every repeat times each leg once
                        ms[k].append(timed(fn, args.steps))
                assert all(x == x for x in td3.losses() + mob.losses()), "non-finite losses"
                rec = dict(bs=bs, N=2 * bs, mfma=mfma, graph=graph)
                for k, v in ms.items():
                    rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
                rec["td3bc_minus_mobody_ms"] = rec["td3bc"]["median_ms"] - rec["mobody"]["median_ms"]
                rec["within_mobody_spread"] = rec["td3bc_minus_mobody_ms"] <= rec["mobody"]["spread_ms"]
                runs.append(rec)
                print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"})
                                  for k, v in rec.items()}), flush=True)
    doc = dict(what="ms per train() step, walker2d shapes S=17 A=6: TD3BC (advantage=%d) | MOBODY(q_weighted=0, fake_batch_scale=0, "
                    "penalty_type='none') at the same N | PyTorch-eager TD3_BC restatement; medians over alternating repeats" % args.advantage,
               src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, advantage=args.advantage, src_rows=args.src_rows, runs=runs)
    if os.path.exists(args.out):
        try:
            old = json.load(open(args.out))
            doc.update({k: v for k, v in old.items() if k not in doc})      # records this tool does not write are kept
        except (OSError, ValueError):
            pass
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
