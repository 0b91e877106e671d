#!/usr/bin/env python
"""BOSA stage-2 benchmark (one GPU): ms per call at walker2d shapes (S = 17, A = 6), the reference's widths (VAEs 750 wide,
E = 5), config['critic_actor'] set; the mixed batch [tar | src] has 2 bs rows.  Legs, alternating in the same process:

  stage2_critic     `BOSA.critic_actor_train` on a staged batch at an odd total_it: target values, the dynamics mask, the critic step
  stage2_actor      the same at an even total_it: additionally the actor step with the estimator's gradient and the Polyak updates
  llg1 / llg10      mobody_bosa_loglik_grad alone at num_samples 1 (the reference's config value) and 10
  torch_llg1 / 10   an eager PyTorch restatement on the same GPU: the estimator under autograd, torch.autograd.grad with respect to the action

Stage-2 calls run eagerly (they are not graph-captured).  The tool runs the shapes in the order given -- smallest first --, sizes every
workspace of a shape before it times anything (one untimed call of each leg), never retries a step and sets no pass threshold.  Run it
with each shape under a time limit of its own; a run of one shape merges its record into the JSON document of the others:

  timeout -k 10 300 python tools/bench_bosa_stage2.py --bs 128 && timeout -k 10 600 python tools/bench_bosa_stage2.py --bs 4096

Each leg is timed `--repeats` times (`--steps` calls between two device synchronisations, after `--warmup` calls), the legs alternating;
medians and the min / max spread are reported.  Results: profiles/bosa_stage2.json (`--out`) with the build's source fingerprint.

`--graph` times whole stage-2 train() calls instead -- the gather of both buffers included -- in three legs per call kind
(critic call, actor call), alternating with the same warm-up, repeats and reporting:

  eager_key0        config['critic_actor_graph'] unset: the torch composition between the launches, the call the parent commit makes (no
                    kernel it runs differs from the parent's: tools/isa_diff.py)
  eager_key1        the key set, replay held off: the same launches with the row-wise entries in place of the torch ops
  replay_key1       the key set: the call replays its HIP graph

and writes profiles/bosa_stage2_graph.json.  `--isa_diff` and `--bench_c2` take text to record in that document (the isa_diff line, the
alternating bench.py c2 figures)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_bosa import CFG, E, H  # noqa: E402
from bench_iql import S, A, TASK, timed  # noqa: E402

LAUNCHES = dict(loglik_grad="19: the estimator's 10, then k_bosa_llg_seed, 3 for the decoder's input gradient on n B rows, k_bosa_llg_enc, 3 for "
                            "the encoder's, k_bosa_llg_sum",
                actor="forward 3 (pi, critic_1, the statistics) and a copy; backward 6 (two row-wise seeds, two backwards in seed mode 0, the "
                      "weight gradients and their reduction)",
                stage2="target values (2 forwards + row-wise torch ops), the dynamics estimator 11, mobody_bosa_critic, and on an actor call the "
                       "actor phase, the estimator's gradient and two mobody_adam_polyak")


def torch_llg(dev, rows, n):
    """Eager PyTorch: d ll / d action of the policy VAE's importance-sampling estimator by autograd, `rows` fixed rows."""
    import torch
    import torch.distributions as td
    g = torch.Generator(device=dev); g.manual_seed(0)
    s, a = torch.randn(rows, S, device=dev, generator=g), (torch.rand(rows, A, device=dev, generator=g) * 2 - 1).requires_grad_(True)
    Lz = 2 * A
    lin = lambda i, o: (torch.randn(i, o, device=dev, generator=g) / i ** 0.5, torch.zeros(o, device=dev))
    enc, dec = [lin(S + A, H), lin(H, H), lin(H, 2 * Lz)], [lin(S + Lz, H), lin(H, H), lin(H, A)]

    def mlp(p, x):
        h = torch.relu(torch.addmm(p[0][1], x, p[0][0]))
        return torch.addmm(p[2][1], torch.relu(torch.addmm(p[1][1], h, p[1][0])), p[2][0])
    sd = (0.5 / 4) ** 0.5

    def run():
        o = mlp(enc, torch.cat([s, a], 1))
        mean, std = o[:, :Lz].repeat(n, 1), torch.exp(o[:, Lz:].clamp(-4, 15)).repeat(n, 1)
        z = mean + std * torch.randn_like(std)
        u = torch.tanh(mlp(dec, torch.cat([s.repeat(n, 1), z], 1)))
        w = (td.Normal(u, sd).log_prob(a.repeat(n, 1)).sum(-1) + td.Normal(0.0, 1.0).log_prob(z).sum(-1) - td.Normal(mean, std).log_prob(z).sum(-1))
        ll = w.reshape(n, rows).logsumexp(0) - float(torch.log(torch.tensor(float(n))))
        return torch.autograd.grad(ll.sum(), a)[0]
    return run


def make_legs(dev, bs, buffers):
    import numpy as np
    import torch
    from mobody_amd import ops
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    torch.manual_seed(0); np.random.seed(0)
    pol = call_algo("bosa", dict(CFG, rng="device", seed=0, batch_size=bs, vae_iteration=0, critic_actor=1), 3, dev)
    sd = pol.vae_dyna.state_dict()                 # EnsembleFC's unit-variance weights overflow at this width
    pol.vae_dyna.load_state_dict({k: (v / v.shape[1] ** 0.5 if k.endswith(".W") else v) for k, v in sd.items()})
    pol.train(src, tar, bs, None, None)            # stages a batch and sizes the stage's workspaces
    b = tuple(t.clone() for t in pol._batch)
    N = 2 * bs

    def stage2(total_it):
        def run():
            pol.total_it = total_it
            pol.critic_actor_train(b)
        return run

    def llg(n):
        vae = pol.vae_policy
        ll, dll = torch.empty(1, N, device=dev), torch.empty(N, A, device=dev)
        ws = ops.bosa_loglik_grad_workspace(vae.block(N, n), dev)      # sized here, before anything is timed
        call = [0]

        def run():
            call[0] += 1
            ops.bosa_loglik_grad(vae.block(N, n, state=b[0], action=b[1], seed=7, call=call[0], ll=ll, workspace=ws), dll)
        return run
    legs = dict(stage2_critic=stage2(0), stage2_actor=stage2(1), llg1=llg(1), llg10=llg(10), torch_llg1=torch_llg(dev, N, 1), torch_llg10=torch_llg(dev, N, 10))
    return legs, pol


GRAPH_LAUNCHES = dict(critic_call="gather 1 + mobody_bosa_target 4 + the dynamics estimator with mask_mean 11 + mobody_bosa_stage2_rows 1 + "
                                  "mobody_bosa_critic (fused) + mobody_bosa_stage2_words 1",
                      actor_call="gather 1 + target 4 + estimator 11 + rows 1 + mobody_bosa_critic (gradient form) + mobody_adam_polyak + "
                                 "mobody_bosa_actor_forward 3 and a copy + mobody_bosa_loglik_grad 19 + rows 1 + mobody_bosa_actor_backward 6 + "
                                 "mobody_adam_polyak + mobody_bosa_stage2_words 1",
                      eager_key0="the same without rows / words; about fifteen torch ops in their place, and mobody_rng_normal for the target noise")


def make_graph_legs(dev, bs, buffers):
    """{call kind: {leg: fn}} and the three objects.  A call's kind is chosen by the host from total_it, which each leg sets before its
    call (1 -> an actor call at update_interval 2, 2 -> a critic call; neither is on the health cadence)."""
    import numpy as np
    import torch
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    pols = {}
    for name, key in (("eager_key0", 0), ("eager_key1", 1), ("replay_key1", 1)):
        torch.manual_seed(0); np.random.seed(0)
        pol = call_algo("bosa", dict(CFG, rng="device", seed=0, batch_size=bs, vae_iteration=0, critic_actor=1, critic_actor_graph=key), 3, dev)
        sd = pol.vae_dyna.state_dict()
        pol.vae_dyna.load_state_dict({k: (v / v.shape[1] ** 0.5 if k.endswith(".W") else v) for k, v in sd.items()})
        pols[name] = pol

    def leg(name, total_it):
        pol = pols[name]

        def eager():                                   # _train_stage2's eager path: the gather, then the call
            pol.total_it = total_it
            pol._gather(src, tar, bs)
            pol.critic_actor_train(pol._batch)

        def replay():
            pol.total_it = total_it
            pol.train(src, tar, bs, None, None)
        return replay if name == "replay_key1" else eager
    for pol in pols.values():                          # sizes the buffers; with the key set, one eager call of each kind
        for total_it in (2, 1):
            pol.total_it = total_it
            pol.train(src, tar, bs, None, None)
    return dict(critic={n: leg(n, 2) for n in pols}, actor={n: leg(n, 1) for n in pols}), pols


def graph_main(args, dev, src, tar, fp):
    import torch
    out = args.out if args.out != os.path.join(ROOT, "profiles", "bosa_stage2.json") else os.path.join(ROOT, "profiles", "bosa_stage2_graph.json")
    runs = {}
    if os.path.exists(out):
        old = json.load(open(out))
        if old.get("src_fingerprint") == fp:
            runs = {r["bs"]: r for r in old.get("runs", [])}
    for bs in sorted(args.bs):
        kinds, pols = make_graph_legs(dev, bs, (src, tar))
        legs = {f"{kind}_{name}": fn for kind, d in kinds.items() for name, fn in d.items()}
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():
                ms[name].append(timed(fn, args.steps))
        rp = pols["replay_key1"]
        rec = dict(bs=bs, rows=2 * bs, hidden=H, members=E, replays=rp.stage2_replays, captures=rp.stage2_captures)
        for name, v in ms.items():
            rec[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
        for kind in kinds:
            base = rec[f"{kind}_eager_key0"]
            rec[f"{kind}_replay_over_eager_key0"] = rec[f"{kind}_replay_key1"]["median_ms"] / base["median_ms"]
            rec[f"{kind}_eager_key1_over_eager_key0"] = rec[f"{kind}_eager_key1"]["median_ms"] / base["median_ms"]
            rec[f"{kind}_replay_gain_beyond_spread"] = base["median_ms"] - rec[f"{kind}_replay_key1"]["median_ms"] > base["spread_ms"]
        runs[bs] = rec
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: (round(b, 4) if isinstance(b, float) else b) for a, b in v.items() if a != "runs_ms"})
                          for k, v in rec.items()}), flush=True)
        del kinds, legs, pols
    doc = dict(what="ms per stage-2 train() call (gather included), walker2d shapes S=17 A=6, VAEs 750 wide, E=5, 2 bs mixed rows: the eager call "
                    "with config['critic_actor_graph'] unset (the parent's call), the eager call with the key set, the replayed call; critic "
                    "calls and actor calls separately; medians over alternating repeats",
               launches=GRAPH_LAUNCHES, src_fingerprint=fp, device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, src_rows=args.src_rows, isa_diff=args.isa_diff, bench_c2=args.bench_c2, parent_tool=args.parent_tool)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(runs[k]) for k in sorted(runs)) + "\n ]\n}\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", action="store_true", help="time whole stage-2 train() calls: key unset | key set, eager | key set, replayed")
    ap.add_argument("--isa_diff", default=None, help="text recorded in the --graph document: the line of tools/isa_diff.py against the parent build")
    ap.add_argument("--bench_c2", default=None, help="text recorded in the --graph document: bench.py's c2 figures against the parent, alternating")
    ap.add_argument("--parent_tool", default=None, help="text recorded in the --graph document: the parent build's own run of this tool")
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 4096])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src_rows", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bosa_stage2.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bosa_stage2.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.src_rows, rng="device", seed=100), args.src_rows, TASK, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=5000, rng="device", seed=200), 5000, TASK, 1000)
    fp = bench.src_fingerprint()
    if args.graph:
        return graph_main(args, dev, src, tar, fp)
    runs = {}
    if os.path.exists(args.out):                                  # the other shapes' records of the same build
        old = json.load(open(args.out))
        if old.get("src_fingerprint") == fp:
            runs = {r["bs"]: r for r in old.get("runs", [])}
    for bs in sorted(args.bs):                                    # the smallest shape first
        legs, pol = make_legs(dev, bs, (src, tar))
        for fn in legs.values():                                  # sizes every workspace of the shape; nothing is timed yet
            fn()
        torch.cuda.synchronize()
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        ms = {k: [] for k in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():                         # alternating: every repeat times each leg once
                ms[name].append(timed(fn, args.steps))
        rec = dict(bs=bs, rows=2 * bs, hidden=H, members=E)
        for name, v in ms.items():
            rec[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
        med = lambda name: rec[name]["median_ms"]
        for a_, b_ in (("llg1", "torch_llg1"), ("llg10", "torch_llg10")):
            rec[f"{a_}_over_{b_}"] = med(a_) / med(b_)
        rec["actor_step_ms"] = med("stage2_actor") - med("stage2_critic")
        runs[bs] = rec
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"}) for k, v in rec.items()}),
              flush=True)
        del legs, pol
    doc = dict(what="ms per call, walker2d shapes S=17 A=6, VAEs 750 wide, E=5, 2 bs mixed rows, config['critic_actor']: a stage-2 call without and "
                    "with the actor step (eager) | mobody_bosa_loglik_grad at num_samples 1 and 10 | its eager PyTorch autograd form; medians over "
                    "alternating repeats; the VAEs in exact fp32 on both sides",
               launches=LAUNCHES, src_fingerprint=fp, device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, src_rows=args.src_rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(runs[k]) for k in sorted(runs)) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
