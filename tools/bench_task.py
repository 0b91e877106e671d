#!/usr/bin/env python
"""The analytic control task (mobody_amd/task.py) on one GPU: environment steps per second of `Task.evaluate` and `Task.collect` at
walker2d shapes (S = 17, A = 6).

  evaluate   B episodes of H steps of a policy net (head 0 / 1) or of the built-in expert controller (head 2), three legs:
               eager    one `mobody_task_evaluate` call (chunk = 0)
               graph    the chunk graph (`--chunk` steps captured once, replayed H / chunk times)
               compose  the Python loop a user would write: policy forward + `mobody_task_step` under a carried alive mask, the
                        per-row sums kept in torch ops on the device (no host synchronisation inside the loop)
  collect    lanes x 2000 steps of the expert controller through `mobody_task_collect` (one launch per step), with the copy to the host

Every timed run ends in a synchronisation and is bracketed by the host clock; after `--warmup` runs of each leg the legs alternate
`--repeats` times; medians with the min / max spread are reported.  steps/s counts B x H (lanes x L) environment steps per run,
finished rows included.  Results: one JSON document (`--out`, default profiles/task_rollout.json) with the build's source fingerprint.

  python tools/bench_task.py [--B 32 1024] [--H 1000] [--heads 0 1 2] [--lanes 10 500] [--chunk 50] [--warmup 1] [--repeats 5]
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

ENV, LEVEL = "walker2d-friction", "2.0"


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v, steps):
    med = statistics.median(v)
    return dict(median_ms=med, min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v, steps_per_s=steps / (med * 1e-3))


def evaluate_legs(task, net, head, B, H, chunk, mfma):
    import torch
    from mobody_amd import ops
    A = task.spec.A
    kw = dict(controller="expert") if head == 2 else {}
    legs = {"eager": lambda: task.evaluate(net, head, B, H, chunk=0, **kw), "graph": lambda: task.evaluate(net, head, B, H, chunk=chunk, **kw)}
    if head != 2:
        init = task.start_states(B, 1)

        def compose():
            obs, alive = init, torch.ones(B, dtype=torch.uint8, device=init.device)
            ret, length = torch.zeros(B, device=init.device), torch.zeros(B, dtype=torch.int32, device=init.device)
            for t in range(H):
                act = ops.mlp3_forward(net.blob, net.in_dim, net.out_dim, 1, obs, out_mode=1, max_action=1.0, blob_T=net.blob_T,
                                       precision=net.precision)[0][:, :A].contiguous()
                r = ops.task_step(task.params, obs, act, alive=alive, seed=1, call=1 + t)
                live = alive != 0
                ret = torch.where(live, ret + r["reward"], ret)
                length += live
                alive = (live & (r["terminal"] == 0)).to(torch.uint8)
                obs = r["next_obs"]
            return torch.stack([ret.mean(), length.float().mean(), alive.float().mean()]).tolist()

        legs["compose"] = compose
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[32, 1024])
    ap.add_argument("--H", type=int, nargs="+", default=[1000])
    ap.add_argument("--heads", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--lanes", type=int, nargs="+", default=[10, 500])
    ap.add_argument("--mfma", default="f16x2")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_rollout.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_task.py: no GPU (a rollout time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import ops
    from mobody_amd.algo.offline_offline.iql import _GaussianPolicy
    from mobody_amd.algo.offline_offline.mobody import _PackedNet
    from mobody_amd.task import LANE_STEPS, Task, TaskSpec
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    task = Task(TaskSpec.from_env(ENV, LEVEL, "target"), dev, seed=0)
    S, A = task.spec.S, task.spec.A
    prec = ops.prec_id(args.mfma)
    nets = {0: _PackedNet(S, A, 1, ("network.",), dev, out_mode=1, max_action=1.0, precision=prec), 1: _GaussianPolicy(S, A, 1.0, dev, prec), 2: None}
    runs = []
    for head in args.heads:
        for B in args.B:
            for H in args.H:
                legs = evaluate_legs(task, nets[head], head, B, H, args.chunk, args.mfma)
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                ms = {k: [] for k in legs}
                for _ in range(args.repeats):
                    for k, fn in legs.items():
                        ms[k].append(timed(fn))
                rec = dict(what="evaluate", head=head, B=B, H=H, chunk=args.chunk, mfma=args.mfma if head != 2 else None)
                rec.update({k: stats(v, B * H) for k, v in ms.items()})
                runs.append(rec)
                print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 3) for a, b in v.items() if a != "runs_ms"})
                                  for k, v in rec.items()}), flush=True)
    for lanes in args.lanes:
        rows = lanes * LANE_STEPS
        fn = lambda: task.collect("expert", rows, seed=1)
        for _ in range(args.warmup):
            fn()
        rec = dict(what="collect", kind="expert", lanes=lanes, L=LANE_STEPS, collect=stats([timed(fn) for _ in range(args.repeats)], rows))
        runs.append(rec)
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 3) for a, b in v.items() if a != "runs_ms"})
                          for k, v in rec.items()}), flush=True)
    doc = dict(what="environment steps per second of the analytic control task, walker2d shapes S=17 A=6 (walker2d-friction 2.0 target): "
                    "Task.evaluate eager | chunk-graph replay | Python loop over mobody_task_step, and Task.collect; host clock around runs "
                    "that end in a synchronisation, medians over alternating repeats",
               src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), warmup=args.warmup, repeats=args.repeats,
               runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
