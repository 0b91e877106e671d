#!/usr/bin/env python
"""Policy evaluation in the learned model (one GPU): ms per evaluation of B episodes of H steps at walker2d shapes
(S = 17, A = 6), three legs alternating in one process:

  eager    one `mobody_ens_evaluate` call (MOBODYEnsembleDynamics.evaluate_policy, chunk=0): 5 launches per step
  graph    the same through the chunk graph (chunk=`--chunk` steps captured once, replayed H / chunk times)
  compose  what a user of the parent commit has to write: a Python loop of policy forward + `dynamics.step_device` under
           a carried alive mask with the per-row sums kept in torch ops on the device (no host synchronisation inside the
           loop: the form most favourable to it)

With `--head 0|1` (and `--members`) the eager and graph legs run through `mobody_ens_evaluate_policy` instead
(MOBODYEnsembleDynamics.evaluate_policy(head=, members=, entry='policy'): `entry='policy'` is what sends `--head 0` without
`--members`, which evaluate_policy would otherwise run through the old entry, through the NEW one; `--head 1` is a Gaussian
policy (S, 2A, 1), one launch more per step; `--members` rolls every one of the B start states once per elite, B x 5 rows, each
episode under one member) and the result is read through `mobody_eval_summary`; the compose leg is left out, and the default
`--out` becomes profiles/model_eval_policy_run.json.  Without `--head` the tool measures what it always did.

for B in {32, 1024} x H in {100, 1000} x mfma in {f16x2, f32}.  Every timed run ends in a synchronisation (the means are
read back) and is bracketed by the host clock; after `--warmup` runs of each leg the legs alternate `--repeats` times;
medians with the min / max spread are reported.  `below_compose`: the leg's median lies below compose's median by more
than the larger of the two spreads.  Results: one JSON document (`--out`, default profiles/model_eval.json) with the
build's source fingerprint; keys already in that file that this tool does not write are kept.

  python tools/bench_model_eval.py [--B 32 1024] [--H 100 1000] [--mfma f16x2 f32] [--chunk 50] [--warmup 1] [--repeats 5]
                                   [--head 0|1 [--members]]
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


def make_legs(dev, B, H, mfma, chunk, head=None, members=False):
    import numpy as np
    import torch
    from mobody_amd import engine, synthetic
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    from mobody_amd.algo.offline_offline.mobody import MOBODY
    torch.manual_seed(0); np.random.seed(0)
    cfg = engine.default_config(S, A, rng="device", seed=0, mfma=mfma)
    pol = MOBODY(cfg, dev)
    model = synthetic.alive_dynamics(MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg), TASK)
    dyn = pol.dynamics = MOBODYEnsembleDynamics(cfg, model, None, None, get_termination_fn(TASK), rng="device", seed=3)
    g = torch.Generator(device="cpu").manual_seed(1)
    init = (torch.from_numpy(synthetic.alive_mean(TASK, S)) + 0.1 * torch.randn(B, S, generator=g)).to(dev).contiguous()

    def compose():
        obs, alive = init, torch.ones(B, dtype=torch.uint8, device=dev)
        ret, pen = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
        length = torch.zeros(B, dtype=torch.int32, device=dev)
        for _ in range(H):
            act = pol.policy(obs).reshape(-1, A)
            r = dyn.step_device(obs, act, False, True, alive=alive)
            live = alive != 0
            ret = torch.where(live, ret + r["raw_reward"].flatten(), ret)
            pen = torch.where(live, pen + r["penalty"].flatten(), pen)
            length += live
            alive = (live & (r["terminal"].flatten() == 0)).to(torch.uint8)
            obs = r["next_obs"]
        return torch.stack([ret.mean(), length.float().mean(), pen.mean(), alive.float().mean()]).tolist()

    if head is not None:                                   # both legs through mobody_ens_evaluate_policy, whatever the head
        from mobody_amd.algo.offline_offline.iql import _GaussianPolicy
        net = pol.policy if head == 0 else _GaussianPolicy(S, A, 1.0, dev, pol.policy.precision)
        run = lambda c: dyn.evaluate_policy(net, init, H, chunk=c, head=head, members=members, entry="policy")
        return {"eager": lambda: run(0), "graph": lambda: run(chunk)}, dyn
    legs = {"eager": lambda: pol.evaluate_in_model(init, H, chunk=0), "graph": lambda: pol.evaluate_in_model(init, H, chunk=chunk),
            "compose": compose}
    return legs, dyn


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[32, 1024])
    ap.add_argument("--H", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--head", type=int, choices=[0, 1], default=None, help="run the legs through mobody_ens_evaluate_policy at this head")
    ap.add_argument("--members", action="store_true", help="with --head: every start state once per elite, one member per episode")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.members and args.head is None:
        ap.error("--members needs --head")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "model_eval.json" if args.head is None else "model_eval_policy_run.json")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_model_eval.py: no GPU (an evaluation time is a GPU measurement; there is no CPU fallback)")
    import bench
    dev = torch.device("cuda:0")
    runs = []
    for mfma in args.mfma:
        for B in args.B:
            for H in args.H:
                legs, dyn = make_legs(dev, B, H, mfma, args.chunk, args.head, args.members)
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                assert dyn.eval_captures == (1 if H > args.chunk > 0 else 0)
                ms = {k: [] for k in legs}
                for _ in range(args.repeats):
                    for k, fn in legs.items():            # alternating: every repeat times each leg once
                        ms[k].append(timed(fn))
                assert dyn.eval_captures == (1 if H > args.chunk > 0 else 0), "the chunk graph was captured again"
                rec = dict(B=B, H=H, mfma=mfma, chunk=args.chunk)
                if args.head is not None:
                    rec.update(head=args.head, members=args.members, rows=B * (len(dyn.model.elites_host()) if args.members else 1))
                for k, v in ms.items():
                    rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v,
                                  us_per_step=statistics.median(v) * 1e3 / H)
                for k in ("eager", "graph") if "compose" in rec else ():
                    gap = rec["compose"]["median_ms"] - rec[k]["median_ms"]
                    rec[k]["below_compose"] = gap > max(rec[k]["spread_ms"], rec["compose"]["spread_ms"])
                    rec[k]["compose_over_this"] = rec["compose"]["median_ms"] / rec[k]["median_ms"]
                runs.append(rec)
                print(json.dumps({k: (v if not isinstance(v, dict) else {a: (round(b, 4) if isinstance(b, float) else b)
                                                                         for a, b in v.items() if a != "runs_ms"})
                                  for k, v in rec.items()}), flush=True)
    what = ("one eager mobody_ens_evaluate call | chunk-graph replay | Python composition of policy forward + dynamics.step_device"
            if args.head is None else "one eager mobody_ens_evaluate_policy call | chunk-graph replay, read through mobody_eval_summary")
    doc = dict(what="ms per evaluation of B episodes x H steps in the learned model, walker2d shapes S=17 A=6: " + what +
                    "; host clock around runs that end in a synchronisation, medians over alternating repeats",
               src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), warmup=args.warmup,
               repeats=args.repeats, runs=runs)
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
