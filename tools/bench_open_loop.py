#!/usr/bin/env python
"""Open-loop model error over recorded windows (one GPU): ms per call of B windows of H steps at walker2d shapes
(S = 17, A = 6), two legs alternating in one process:

  fused    one `mobody_ens_replay` call (MOBODYEnsembleDynamics.open_loop_error): 4 launches per step
  compose  what a user of the parent commit has to write: a Python loop of torch gathers from the buffer +
           `dynamics.step_device` + torch error ops, the tables kept on the device (no host synchronisation inside the
           loop: the form most favourable to it)

for B in {256, 4096} x H in {10, 100} x mfma in {f16x2, f32}.  Every timed run ends in a synchronisation (the per-step
summaries are read back) and is bracketed by the host clock; after `--warmup` runs of each leg the legs alternate
`--repeats` times; medians with the min / max spread are reported.  `below_compose`: the fused median lies below compose's
median by more than the larger of the two spreads.  Results: one JSON document (`--out`, default profiles/open_loop.json)
with the build's source fingerprint; keys already in that file that this tool does not write are kept.

  python tools/bench_open_loop.py [--B 256 4096] [--H 10 100] [--mfma f16x2 f32] [--warmup 1] [--repeats 5]
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
ROWS = 20000


def make_legs(dev, B, H, mfma):
    import numpy as np
    import torch
    from mobody_amd import engine, synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    torch.manual_seed(0); np.random.seed(0)
    cfg = engine.default_config(S, A, rng="device", seed=0, mfma=mfma)
    model = synthetic.alive_dynamics(MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg), TASK)
    dyn = MOBODYEnsembleDynamics(cfg, model, None, None, get_termination_fn(TASK), rng="device", seed=3)
    buf = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=ROWS, rng="device", seed=2), ROWS, TASK, 1)
    row0 = np.sort(np.random.default_rng(1).integers(0, ROWS - H + 1, B)).astype(np.int64)
    rows = torch.from_numpy(row0).to(dev)

    def compose():
        obs = buf.state[rows]
        obs_err, rew_err, agree = [], [], []
        for t in range(H):
            r = rows + t
            out = dyn.step_device(obs, buf.action[r], False, True, call=1 + t, seed_offset=0x0B1E)
            obs = out["next_obs"]
            obs_err.append(torch.sqrt(torch.sum((obs - buf.next_state[r]) ** 2, dim=1)))
            rew_err.append(out["raw_reward"].flatten() - buf.reward[r].flatten())
            agree.append((out["terminal"].flatten() != 0) == (buf.not_done[r].flatten() == 0))
        e, w, g = torch.stack(obs_err), torch.stack(rew_err), torch.stack(agree)
        return torch.stack([e.mean(1), (w ** 2).mean(1), g.float().mean(1)]).tolist()

    def fused():
        o = dyn.open_loop_error(buf, row0, H)
        return torch.stack([o["obs_err_mean"], o["rew_mse"], o["term_agree"]]).tolist()

    return {"fused": fused, "compose": compose}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--H", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_loop.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_open_loop.py: no GPU (a call's time is a GPU measurement; there is no CPU fallback)")
    import bench
    dev = torch.device("cuda:0")
    runs = []
    for mfma in args.mfma:
        for B in args.B:
            for H in args.H:
                legs = make_legs(dev, B, H, mfma)
                for fn in legs.values():
                    for _ in range(args.warmup):
                        fn()
                ms = {k: [] for k in legs}
                for _ in range(args.repeats):
                    for k, fn in legs.items():            # alternating: every repeat times each leg once
                        ms[k].append(timed(fn))
                rec = dict(B=B, H=H, mfma=mfma)
                for k, v in ms.items():
                    rec[k] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v,
                                  us_per_step=statistics.median(v) * 1e3 / H)
                gap = rec["compose"]["median_ms"] - rec["fused"]["median_ms"]
                rec["fused"]["below_compose"] = gap > max(rec["fused"]["spread_ms"], rec["compose"]["spread_ms"])
                rec["fused"]["compose_over_this"] = rec["compose"]["median_ms"] / rec["fused"]["median_ms"]
                runs.append(rec)
                print(json.dumps({k: (v if not isinstance(v, dict) else {a: (round(b, 4) if isinstance(b, float) else b)
                                                                         for a, b in v.items() if a != "runs_ms"})
                                  for k, v in rec.items()}), flush=True)
    doc = dict(what="ms per open-loop error call of B windows x H steps over a recorded buffer, walker2d shapes S=17 A=6: one "
                    "mobody_ens_replay call | Python composition of torch gathers + dynamics.step_device + torch error ops; host "
                    "clock around runs that end in a synchronisation, medians over alternating repeats",
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
