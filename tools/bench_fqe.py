#!/usr/bin/env python
"""Fitted Q evaluation benchmark (one GPU): ms per FQE step at walker2d shapes (S = 17, A = 6), a Gaussian policy (head 1),
per batch size and MFMA mode.  Legs, alternating in the same process:

  replayed    FQE.fit's step replayed as one HIP graph (rng='device')
  eager       the same launches issued by the host: gather, mobody_fqe_target, mobody_critic in its q_next form (fused Adam + Polyak)
  torch       an eager PyTorch restatement on the same GPU: randint + index_select, the policy and target forwards under no_grad, the
              twin-Q loss under autograd, torch.optim.Adam, a Polyak update with torch._foreach ops (always fp32)

and, once per mode at the first batch size, a whole evaluation: reset(), fit(--fit_steps), value(256 start rows), wall time with one
device synchronisation at the end.  The tool runs the shapes in the order given -- smallest first --, sizes every workspace of a shape
before it times anything, never retries a step and sets no pass threshold.

  timeout -k 10 300 python tools/bench_fqe.py --bs 256 4096 --modes f16x2 f32

Each leg is timed `--repeats` times (one fit(`--steps`) between two device synchronisations, after `--warmup` steps), the legs alternating;
medians and the min / max spread are reported.  Results: profiles/fqe_step.json (`--out`) with the build's source fingerprint."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_iql import S, A, TASK  # noqa: E402

HEAD, GAMMA, TAU, LR = 1, 0.99, 0.005, 3e-4
LAUNCHES = dict(step="gather 1 + mobody_fqe_target 4 (policy forward, k_fqe_action, target twin-Q forward, k_fqe_qnext; 3 for head 0) + "
                     "mobody_critic with q_next and m, v (forward, backward, weight gradients with the fused Adam + Polyak launch)",
                value="policy forward, k_fqe_action (head 1), twin-Q forward, k_fqe_value_rows, k_fqe_value")


def timed(fn, steps):
    """ms per step of fn(steps) between two device synchronisations (fit's one host read of the health words comes once per call)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def torch_step(dev, bs, tar):
    """Eager PyTorch FQE step on rows of the same buffer."""
    import torch
    g = torch.Generator(device=dev); g.manual_seed(0)
    mlp = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                                           torch.nn.Linear(256, o)).to(dev)
    pi, q, qt = mlp(S, 2 * A), [mlp(S + A, 1), mlp(S + A, 1)], [mlp(S + A, 1), mlp(S + A, 1)]
    for a_, b_ in zip(q, qt):
        b_.load_state_dict(a_.state_dict())
    params = [p for n in q for p in n.parameters()]
    tparams = [p for n in qt for p in n.parameters()]
    opt = torch.optim.Adam(params, lr=LR)
    store, n = tar.store, tar.size
    mse = torch.nn.functional.mse_loss

    def run():
        idx = torch.randint(0, n, (bs,), device=dev, generator=g)
        row = store.index_select(0, idx)
        s, a, s2, r, nd = row[:, :S], row[:, S:S + A], row[:, S + A:2 * S + A], row[:, 2 * S + A:2 * S + A + 1], row[:, 2 * S + A + 1:2 * S + A + 2]
        with torch.no_grad():
            x2 = torch.cat([s2, torch.tanh(pi(s2)[:, :A])], 1)
            y = r + nd * GAMMA * 0.5 * (qt[0](x2) + qt[1](x2))
        x = torch.cat([s, a], 1)
        loss = mse(q[0](x), y) + mse(q[1](x), y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        with torch.no_grad():
            torch._foreach_mul_(tparams, 1.0 - TAU)
            torch._foreach_add_(tparams, params, alpha=TAU)
    return lambda steps: [run() for _ in range(steps)]


def make_fqe(dev, mode, bs, rng):
    import torch
    from mobody_amd import ops
    from mobody_amd.algo.offline_offline.iql import _GaussianPolicy
    from mobody_amd.fqe import FQE
    torch.manual_seed(0)
    policy = _GaussianPolicy(S, A, 1.0, dev, ops.prec_id(mode))
    return FQE(policy, HEAD, S, A, 1.0, GAMMA, dev, mode, lr=LR, tau=TAU, batch_size=bs, seed=0, rng=rng)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--modes", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit_steps", type=int, default=10000)
    ap.add_argument("--tar_rows", type=int, default=100000)
    ap.add_argument("--isa_diff", default=None, help="text recorded in the document: the line of tools/isa_diff.py against the parent build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fqe_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_fqe.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.tar_rows, rng="device", seed=200), args.tar_rows, TASK, 1000)
    start = tar.state[:256].contiguous()
    runs, evals = [], []
    for mode in args.modes:
        for k, bs in enumerate(sorted(args.bs)):
            rep, eag = make_fqe(dev, mode, bs, "device"), make_fqe(dev, mode, bs, "eager")
            legs = dict(replayed=lambda n, f=rep: f.fit(tar, n), eager=lambda n, f=eag: f.fit(tar, n), torch=torch_step(dev, bs, tar))
            for fn in legs.values():                              # sizes every workspace; the replayed leg captures on its second step
                fn(2)
            torch.cuda.synchronize()
            for fn in legs.values():
                fn(args.warmup)
            ms = {name: [] for name in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():                     # alternating: every repeat times each leg once
                    ms[name].append(timed(fn, args.steps))
            rec = dict(mode=mode, bs=bs, captures=rep.captures, replays=rep.replays, eager_replays=eag.replays)
            for name, v in ms.items():
                rec[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
            med = lambda name: rec[name]["median_ms"]
            rec["replayed_over_eager"], rec["replayed_over_torch"] = med("replayed") / med("eager"), med("replayed") / med("torch")
            rec["replay_gain_beyond_spread"] = med("eager") - med("replayed") > rec["eager"]["spread_ms"]
            runs.append(rec)
            print(json.dumps({a: (b if not isinstance(b, dict) else {c: round(d, 4) for c, d in b.items() if c != "runs_ms"}) for a, b in rec.items()}),
                  flush=True)
            if k == 0:                                            # a whole evaluation, the CLI's sequence
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rep.prepare(warm_start=False)
                ok = rep.fit(tar, args.fit_steps)                 # (ends with the one host read of the health words)
                v = rep.value(start)
                dt = time.perf_counter() - t0
                evals.append(dict(mode=mode, bs=bs, fit_steps=args.fit_steps, start_rows=256, seconds=dt, healthy=bool(ok), value=v["value"],
                                  head_gap=v["head_gap"]))
                print(json.dumps(evals[-1]), flush=True)
            del rep, eag, legs
    doc = dict(what="ms per FQE step, walker2d shapes S=17 A=6, Gaussian policy (head 1): replayed as one HIP graph | the same launches eager | "
                    "an eager PyTorch restatement (fp32); medians over alternating repeats; and one whole evaluation reset + fit + value per mode",
               launches=LAUNCHES, src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, tar_rows=args.tar_rows, isa_diff=args.isa_diff, evaluations=evals)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(r) for r in runs) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
