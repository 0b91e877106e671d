#!/usr/bin/env python
"""Does a handful of target interactions help?  TD3_BC and IQL are trained briefly on one shifted task of `--synthetic 2`
(mobody_amd/task.py) with `expert` source data, three ways, and the TRUE target return of the trained policy is written side by side:

  mode1          `--mode 1`: the target buffer starts empty and gets one interaction of the current policy every
                 `--interval` steps (steps / interval target transitions in all)
  mode3_few      `--mode 3` with as many `medium` target rows as mode 1 collects
  mode3_many     `--mode 3` with `--many` `medium` target rows

A measurement: one seed, nothing is asserted about it.  Results: one JSON document (`--out`, default
profiles/task_online_check.json) with the build's source fingerprint.

  python tools/task_online_check.py [--env hopper-friction] [--shift_level 2.0] [--steps 5000] [--interval 10] [--many 20000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="hopper-friction")
    ap.add_argument("--shift_level", default="2.0")
    ap.add_argument("--policies", nargs="+", default=["TD3_BC", "IQL"])
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--many", type=int, default=20000)
    ap.add_argument("--src_rows", type=int, default=100000)
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_online_check.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("task_online_check.py: no GPU (there is no CPU fallback)")
    import bench
    from mobody_amd import train_mobody as tm
    few = args.steps // args.interval
    legs = dict(mode1=(1, few), mode3_few=(3, few), mode3_many=(3, args.many))
    runs = []
    for name in args.policies:
        rec = dict(policy=name, env=args.env, shift_level=args.shift_level, srctype="expert", tartype="medium", steps=args.steps,
                   batch_size=256, interval=args.interval, seed=args.seed, episodes=args.episodes)
        for leg, (mode, tar_rows) in legs.items():
            with tempfile.TemporaryDirectory() as tmp:
                argv = ["--policy", name, "--env", args.env, "--shift_level", args.shift_level, "--mode", str(mode), "--seed", str(args.seed),
                        "--synthetic", "2", "--srctype", "expert", "--tartype", "medium", "--rng", "device", "--src_rows", str(args.src_rows),
                        "--tar_rows", str(tar_rows), "--tar_env_interact_interval", str(args.interval), "--max_step", str(args.steps),
                        "--eval_freq", str(args.steps), "--log_every", str(args.steps), "--dir", tmp,
                        "--params", json.dumps(dict(batch_size=256, graph=1, task_eval_episodes=args.episodes))]
                t0 = time.time()
                tm.main(argv)
                torch.cuda.synchronize()
                secs = time.time() - t0
                rows = [ln.strip().split(",") for d, _, fs in os.walk(tmp) for f in fs if f == "scalars.csv" for ln in open(os.path.join(d, f))][1:]
            logged = {r[0]: float(r[2]) for r in rows if r[0].startswith(("test/source", "test/target", "data/", "train/"))}
            rec[leg] = dict(mode=mode, target_rows=tar_rows, seconds=secs, true_target_return=logged.get("test/target return"), logged=logged)
            print(json.dumps(dict(policy=name, leg=leg, **rec[leg])), flush=True)
        runs.append(rec)
    doc = dict(what="true target return (Task.evaluate through the CLI's test/target return) of policies trained briefly under --synthetic 2 "
                    "with expert source data: mode 1 (online target interactions) | mode 3 with as many medium target rows | mode 3 with "
                    "many; one seed, no assertion", src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
