#!/usr/bin/env python
"""One online interaction with the analytic control task (mobody_amd/task.py OnlineTask, csrc/task_online.hip) on one GPU, at
walker2d shapes (S = 17, A = 6), and what the online modes cost a training run.

  interaction  `--calls` interactions in a row at lanes 1 and 32, heads 0 and 1, three legs:
                 eager    `mobody_task_interact` called every time (3 launches)
                 replay   the captured call replayed (OnlineTask under rng = 'device')
                 composed the same interaction from the existing entry points through the host: `mobody_mlp3_forward`, torch noise and
                          clamp, `Task.step`, `ReplayBuffer.add_batch` (whose `_pull()` is a device-to-host read); episode
                          bookkeeping left out, so the leg is the composition's lower bound
               reported per interaction (run time / calls)
  training     gradient steps/s of TD3_BC at batch 256 over `--steps` steps through the CLI: mode 3, mode 1 (interval 10) and mode 2

Every timed run ends in a synchronisation and is bracketed by the host clock; after `--warmup` runs of each leg the legs alternate
`--repeats` times; medians with the min / max spread are reported.  Results: one JSON document (`--out`, default
profiles/task_online.json) with the build's source fingerprint.

  python tools/bench_task_online.py [--lanes 1 32] [--heads 0 1] [--calls 200] [--steps 2000] [--warmup 1] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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


def stats(v, per):
    med = statistics.median(v)
    return dict(median_us=med * 1e3 / per, min_us=min(v) * 1e3 / per, max_us=max(v) * 1e3 / per, runs_ms=v)


def interaction_legs(task, net, head, lanes, calls, expl):
    import torch
    from mobody_amd import ops
    from mobody_amd.algo import utils
    S, A, dev = task.spec.S, task.spec.A, task.device
    bufs = [utils.ReplayBuffer(S, A, dev, max_size=1 << 16, rng="device", seed=k) for k in range(3)]
    eager = task.online(bufs[0], lanes, 1000, expl, rng="numpy")
    replay = task.online(bufs[1], lanes, 1000, expl, rng="device")
    start = task.start_states(lanes, 7)
    obs = [start]

    def composed():
        obs[0] = start                                    # (no resets in this leg: every run starts where the first did)
        for _ in range(calls):
            out = ops.mlp3_forward(net.blob, S, net.out_dim, 1, obs[0], out_mode=1 if head == 0 else 0, max_action=1.0, blob_T=net.blob_T,
                                   precision=net.precision)[0]
            if head == 1:
                out = torch.tanh(out[:, :A] + torch.exp(out[:, A:].clamp(-20.0, 2.0)) * torch.randn(lanes, A, device=dev))
            if expl:
                out = (out + expl * torch.randn(lanes, A, device=dev)).clamp(-1.0, 1.0)
            r = task.step(obs[0], out.contiguous(), seed=1, call=1)
            bufs[2].add_batch(dict(obss=obs[0], actions=out, next_obss=r["next_obs"], rewards=r["reward"], terminals=r["terminal"]))
            obs[0] = r["next_obs"]

    def run(o):
        return lambda: [o.interact(net, head) for _ in range(calls)]

    return dict(eager=run(eager), replay=run(replay), composed=composed)


def train_cli(mode, steps, out_dir):
    return ["--policy", "TD3_BC", "--env", ENV, "--shift_level", LEVEL, "--mode", str(mode), "--seed", "1", "--synthetic", "2", "--rng", "device",
            "--srctype", "expert", "--tartype", "medium", "--src_rows", "20000", "--tar_rows", "20000", "--tar_env_interact_interval", "10",
            "--max_step", str(steps), "--eval_freq", str(10 * steps), "--log_every", str(10 * steps), "--scalars", "0", "--dir", out_dir,
            "--params", json.dumps(dict(batch_size=256, graph=1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--heads", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--mfma", default="f16x2")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "task_online.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_task_online.py: no GPU (an interaction time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import ops
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.iql import _GaussianPolicy
    from mobody_amd.algo.offline_offline.mobody import _PackedNet
    from mobody_amd.task import Task, TaskSpec
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    task = Task(TaskSpec.from_env(ENV, LEVEL, "target"), dev, seed=0)
    S, A = task.spec.S, task.spec.A
    prec = ops.prec_id(args.mfma)
    nets = {0: _PackedNet(S, A, 1, ("network.",), dev, out_mode=1, max_action=1.0, precision=prec), 1: _GaussianPolicy(S, A, 1.0, dev, prec)}
    show = lambda rec: print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 3) for a, b in v.items() if a != "runs_ms"})
                                         for k, v in rec.items()}), flush=True)
    runs = []
    for head in args.heads:
        for lanes in args.lanes:
            expl = 0.2 if head == 0 else 0.0                  # head 0 with mode 2's noise, head 1 with its own sample
            legs = interaction_legs(task, nets[head], head, lanes, args.calls, expl)
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            ms = {k: [] for k in legs}
            for _ in range(args.repeats):
                for k, fn in legs.items():
                    ms[k].append(timed(fn))
            rec = dict(what="interaction", head=head, lanes=lanes, expl=expl, calls=args.calls, mfma=args.mfma)
            rec.update({k: stats(v, args.calls) for k, v in ms.items()})
            runs.append(rec)
            show(rec)
    os.environ["MOBODY_MFMA"] = args.mfma
    ms = {3: [], 1: [], 2: []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.warmup + args.repeats):
            for mode in ms:
                t = timed(lambda: tm.main(train_cli(mode, args.steps, tmp)))     # set-up included: the same in the three modes
                t0 = timed(lambda: tm.main(train_cli(mode, 0, tmp)))
                if rep >= args.warmup:
                    ms[mode].append(t - t0)
    for mode, v in ms.items():
        med = statistics.median(v)
        rec = dict(what="training", policy="TD3_BC", batch_size=256, mode=mode, steps=args.steps, mfma=args.mfma,
                   steps_per_s=args.steps / (med * 1e-3), median_ms=med, min_ms=min(v), max_ms=max(v), runs_ms=v)
        runs.append(rec)
        show(rec)
    doc = dict(what="one online interaction with the analytic control task, walker2d shapes S=17 A=6: mobody_task_interact eager | captured "
                    "and replayed | composed from the existing entry points through the host, per interaction; and TD3_BC gradient steps/s "
                    "through the CLI in modes 3, 1 (interval 10) and 2 (run time minus the time of the same command at max_step 0); host "
                    "clock around runs that end in a synchronisation, medians over alternating repeats",
               src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), warmup=args.warmup, repeats=args.repeats,
               runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
