#!/usr/bin/env python
"""Collect profiles/model_eval_policy.json from the per-process outputs of tools/bench_model_eval.py (no GPU needed).

The measurement alternates PROCESSES, because the parent build and this build cannot share one: for r in 1..N run, in turn,

  <parent tree>  python tools/bench_model_eval.py --B 64 256 320 --H 100 --mfma f16x2 --chunk 50 --warmup 2 --repeats 5 --out DIR/parent_r.json
  <this tree>    python tools/bench_model_eval.py  (the same arguments)                                   --out DIR/newold_r.json
  <this tree>    ... --head 0                                                                             --out DIR/h0_r.json
  <this tree>    ... --head 1                                                                             --out DIR/h1_r.json
  <this tree>    ... --B 64 --head 1 --members                                                            --out DIR/h1m_r.json

and optionally `python bench.py --gpus 1 --steps 200 --warmup 20 > DIR/bench_parent_r.log` / `DIR/bench_new_r.log` in both trees.
Each process's figure for a (rows, leg) is its median ms per evaluation divided by H; this tool reports, per leg, the median,
minimum and maximum of those figures over the N processes, and for bench.py the `value` of each run's last JSON line.

  python tools/collect_model_eval_policy.py DIR [--isa_diff 'text of tools/isa_diff.py parent new'] [--out profiles/model_eval_policy.json]
"""
import argparse
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEGS = (("parent_mobody_ens_evaluate", "parent"), ("new_build_mobody_ens_evaluate", "newold"), ("head0_new_entry", "h0"), ("head1", "h1"),
        ("head1_members_64x5", "h1m"))


def per_step(directory, prefix):
    out = {}
    for f in sorted(glob.glob(os.path.join(directory, prefix + "_[0-9]*.json"))):
        for r in json.load(open(f))["runs"]:
            for leg in ("eager", "graph"):
                out.setdefault((r.get("rows", r["B"]), leg), []).append(r[leg]["median_ms"] / r["H"])
    return out


def bench_values(directory, prefix):
    vals = []
    for f in sorted(glob.glob(os.path.join(directory, prefix + "_[0-9]*.log"))):
        lines = [ln for ln in open(f).read().splitlines() if ln.startswith("{")]
        if lines:
            rec = json.loads(lines[-1])
            vals.append({k: rec[k] for k in ("metric", "value", "unit") if k in rec})
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--isa_diff", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_eval_policy.json"))
    args = ap.parse_args()
    import bench
    legs = {}
    for name, prefix in LEGS:
        for (rows, leg), v in sorted(per_step(args.directory, prefix).items()):
            legs.setdefault(name, {})[f"rows{rows}_{leg}"] = dict(median_ms_per_step=round(statistics.median(v), 5), min=round(min(v), 5),
                                                                   max=round(max(v), 5), n=len(v))
    doc = dict(what="ms per evaluation STEP of the policy evaluation in the learned model, walker2d shapes S=17 A=6: mobody_ens_evaluate on "
                    "the parent build | the same entry on this build | head 0 through mobody_ens_evaluate_policy | head 1 | head 1 with members "
                    "(64 start states x 5 elites = 320 rows).  One process per leg and round, the legs alternating; each process's figure is "
                    "the median of its timed evaluations (host clock around a run that ends in a synchronisation) divided by H; median, min, "
                    "max over the processes.  eager = one call, graph = the chunk graph replayed.",
               tool="tools/bench_model_eval.py per process, tools/collect_model_eval_policy.py over their outputs",
               src_fingerprint=bench.src_fingerprint(), legs=legs)
    parent, new = bench_values(args.directory, "bench_parent"), bench_values(args.directory, "bench_new")
    doc["bench_py"] = dict(parent=parent, new=new) if parent or new else "not recorded"
    if args.isa_diff:
        doc["isa_diff"] = args.isa_diff
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
