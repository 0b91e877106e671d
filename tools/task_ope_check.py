#!/usr/bin/env python
"""The project's evaluators against the truth, for the first time: TD3_BC and MOBODY are trained briefly on one shifted task of
`--synthetic 2` (mobody_amd/task.py) and, for the trained policy, three figures are written side by side over the same start states
(episode starts of the target data):

  true_value        the discounted return in the TRUE target task, `Task.evaluate(discount = gamma)`
  fqe_value         fitted Q evaluation on the target data (`mobody_amd.fqe`, the CLI's `test/fqe value`)
  model_value       the discounted return in the learned target model (`evaluate_in_model(discount = gamma)`; TD3_BC gets the model
                    through `model_eval_dynamics`, an evaluator only)

plus the undiscounted true return and the data's.  A measurement: nothing is asserted about it.  Results: one JSON document (`--out`,
default profiles/task_ope_check.json) with the build's source fingerprint.

  python tools/task_ope_check.py [--env hopper-friction] [--shift_level 2.0] [--steps 5000] [--fqe_steps 2000] [--episodes 256]
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
    ap.add_argument("--srctype", default="expert")
    ap.add_argument("--tartype", default="medium")
    ap.add_argument("--policies", nargs="+", default=["TD3_BC", "MOBODY"])
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--fqe_steps", type=int, default=2000)
    ap.add_argument("--episodes", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=1000)
    ap.add_argument("--src_rows", type=int, default=100000)
    ap.add_argument("--tar_rows", type=int, default=20000)
    ap.add_argument("--dynamics_max_epochs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_ope_check.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("task_ope_check.py: no GPU (there is no CPU fallback)")
    import bench
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo import utils
    from mobody_amd.fqe import FQE
    from mobody_amd.task import Task, TaskSpec
    dev = torch.device("cuda:0")
    runs = []
    for name in args.policies:
        with tempfile.TemporaryDirectory() as tmp:
            argv = ["--policy", name, "--env", args.env, "--shift_level", args.shift_level, "--mode", "3", "--seed", str(args.seed),
                    "--synthetic", "2", "--srctype", args.srctype, "--tartype", args.tartype, "--rng", "device", "--src_rows", str(args.src_rows),
                    "--tar_rows", str(args.tar_rows), "--max_step", str(args.steps), "--eval_freq", str(args.steps), "--log_every",
                    str(args.steps), "--dir", tmp, "--dynamics_path", os.path.join(tmp, "dyn"), "--train_dynamics", "1",
                    "--dynamics_max_epochs", str(args.dynamics_max_epochs)]
            params = dict(batch_size=256, graph=1)
            if tm.uses_model(name):
                argv += ["--penalty_type", "none", "--src_rollout_batch_size", "4000", "--trg_rollout_batch_size", "1000"]
            else:
                params.update(model_eval_dynamics=1)
            t0 = time.time()
            pol = tm.main(argv + ["--params", json.dumps(params)])
            torch.cuda.synchronize()
            train_s = time.time() - t0
            rows = [ln.strip().split(",") for d, _, fs in os.walk(tmp) for f in fs if f == "scalars.csv" for ln in open(os.path.join(d, f))][1:]
            logged = {r[0]: float(r[2]) for r in rows if r[0].startswith(("test/source", "test/target", "data/"))}
        gamma = float(pol.discount)
        task = Task(TaskSpec.from_env(args.env, args.shift_level, "target"), dev, seed=args.seed)
        tar_ds = task.collect(args.tartype, args.tar_rows, seed=args.seed + 2)            # the run's target data, from its seed
        starts = tm.episode_starts(tar_ds["observations"], tar_ds["next_observations"], tar_ds["terminals"])
        s0 = torch.from_numpy(tar_ds["observations"][tm.model_eval_rows(starts, args.episodes, args.seed)]).to(dev)
        tar_rb = utils.ReplayBuffer(task.spec.S, task.spec.A, dev, rng="device", seed=args.seed + 2)
        tar_rb.convert_D4RL(tar_ds)
        true_d = pol.evaluate_in_task(task, s0.shape[0], args.horizon, discount=gamma, init_obs=s0)
        true_u = pol.evaluate_in_task(task, s0.shape[0], args.horizon, init_obs=s0)
        model_d = pol.evaluate_in_model(s0, args.horizon, discount=gamma)
        net, head = pol.eval_policy()
        fqe = FQE(net, head, task.spec.S, task.spec.A, 1.0, gamma, dev, net.precision, seed=args.seed, rng="device")
        fqe.prepare(warm_start=False)
        fitted = fqe.fit(tar_rb, args.fqe_steps)
        fv = fqe.value(s0) if fitted else dict(value=float("nan"), head_gap=float("nan"))
        rec = dict(policy=name, env=args.env, shift_level=args.shift_level, srctype=args.srctype, tartype=args.tartype, steps=args.steps,
                   gamma=gamma, episodes=int(s0.shape[0]), horizon=args.horizon, train_seconds=train_s,
                   true_value=true_d["return_mean"], fqe_value=fv["value"], fqe_head_gap=fv["head_gap"], fqe_steps=args.fqe_steps,
                   model_value=model_d["return_mean"], model_alive_frac=model_d["alive_frac"], model_length=model_d["length_mean"],
                   true_return=true_u["return_mean"], true_length=true_u["length_mean"], true_alive_frac=true_u["alive_frac"], logged=logged)
        runs.append(rec)
        print(json.dumps(rec), flush=True)
    doc = dict(what="true discounted value (Task.evaluate, discount = gamma) | fitted Q evaluation | discounted return in the learned target "
                    "model, of policies trained briefly under --synthetic 2, over the same episode-start states of the target data; one "
                    "seed, no assertion", src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
