#!/usr/bin/env python
"""IGDF step benchmark (one GPU): ms per `IGDF.train()` step at walker2d shapes (S = 17, A = 6) under graph replay, next to --
alternating in the same process --

  iql               the bare IQL step at the same bs (`IQL.train()`, graph replay): what IGDF's step adds to.  (IGDF's phases run on
                    N = k + bs rows, IQL's on 2 bs: at xi 0.75 the filter also makes the three phases a little shorter.)
  filter_fused      the filter alone on a staged batch, mobody_igdf_filter: one paired forward, the score kernel, the selection
                    with the compaction of the training batch (replayed from a graph, and eager)
  filter_composed   the same filter from what existed before: two mobody_mlp3_forward calls plus torch for the norms, argsort,
                    index_select, exp and the concatenation (eager: torch allocates)
  info_fused        one contrastive update, mobody_igdf_info with the fused Adam, with its two gathers (replay; eager without them)
  info_torch        the same update in eager PyTorch autograd (the reference's n^2-row form, torch.optim.Adam; bs <= 1024 only: at
                    4096 that form holds 17 GB per saved activation)
  torch             a PyTorch-eager restatement of the whole train() step on the same GPU

for bs in {128, 256, 4096} x mfma in {f16x2, f32}.  Each leg is timed `--repeats` times (`--steps` steps between two device
synchronisations, after `--warmup` steps of that leg), the legs alternating; medians and the min / max spread are reported.  Results:
one JSON document (`--out`, default profiles/igdf_step.json) with the build's source fingerprint.

  python tools/bench_igdf.py [--bs 128 256 4096] [--mfma f16x2 f32] [--steps 200] [--warmup 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_iql import CFG as IQL_CFG, S, A, TASK, timed  # noqa: E402

Z = 64
CFG = dict(IQL_CFG, info_update_step=1, repr_dim=Z, ensemble_size=1, repr_norm=False, repr_norm_temp=False, ortho_init=False,
           output_gain="None", importance_weight=1.0, xi=0.75)
LAUNCHES = dict(
    filter_fused="3: one paired forward reading state | action and next_state in place, k_igdf_score, k_igdf_select (rank by "
                 "counting + the compaction of the training batch)",
    filter_composed="2 forwards + torch: mul / sum, two norms, div, argsort, slice, 5 index_select, exp, 6 cat",
    info_fused="8: one paired forward (n and 2n-1 rows), k_igdf_contrast, per encoder the backward from dz3 in memory, the "
               "weight-gradient launch and the reduce + Adam launch (2 x 3)",
    igdf_step="the gather + 3 + IQL's 12",
)


def mlp_params(dev, g, i, o):
    import torch
    ps = []
    for a, b in ((i, 256), (256, 256), (256, o)):
        bound = a ** -0.5
        ps += [torch.empty(b, a, device=dev).uniform_(-bound, bound, generator=g).requires_grad_(True),
               torch.empty(b, device=dev).uniform_(-bound, bound, generator=g).requires_grad_(True)]
    return ps


def mlp(p, x):
    import torch
    import torch.nn.functional as F
    return F.linear(torch.relu(F.linear(torch.relu(F.linear(x, p[0], p[1])), p[2], p[3])), p[4], p[5])


def torch_legs(dev, bs, src, tar, lr=3e-4, gamma=0.99, tau=0.005, lam=0.7, temp=3.0, T_max=500000, xi=0.75, iw=1.0):
    """(one IGDF train() step, one update_info step) in eager PyTorch on the device."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator(device=dev); g.manual_seed(0)
    pol, vf, q1, q2 = mlp_params(dev, g, S, 2 * A), mlp_params(dev, g, S, 1), mlp_params(dev, g, S + A, 1), mlp_params(dev, g, S + A, 1)
    e_sa, e_ss = mlp_params(dev, g, S + A, Z), mlp_params(dev, g, S, Z)
    t1, t2 = [x.detach().clone() for x in q1], [x.detach().clone() for x in q2]
    opt_q, opt_v, opt_p = torch.optim.Adam(q1 + q2, lr=lr), torch.optim.Adam(vf, lr=lr), torch.optim.Adam(pol, lr=lr)
    opt_i = torch.optim.Adam(e_sa + e_ss, lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt_p, T_max)
    fields = [(rb.state, rb.action, rb.next_state, rb.reward, rb.not_done) for rb in (src, tar)]
    sizes = [int(src.size), int(tar.size)]
    k = int(bs * xi)

    def draw(which, n):
        i = torch.randint(0, sizes[which], (n,), device=dev, generator=g)
        return tuple(f[i] for f in fields[which])

    def step():
        ss, sa, ss2, sr, snd = draw(0, bs)
        ts, ta, ts2, tr_, tnd = draw(1, bs)
        with torch.no_grad():
            phi, psi = mlp(e_sa, torch.cat([ss, sa], 1)), mlp(e_ss, ss2)
            logits = torch.einsum("iz,jz->ij", phi, psi)
            info = torch.diag(logits).reshape(-1, 1) / (torch.linalg.norm(phi, dim=-1, keepdim=True) * torch.linalg.norm(psi, dim=-1, keepdim=True))
            top = torch.argsort(info[:, 0])[-k:]
            mask = torch.cat([torch.exp(info[top] * iw), torch.ones(bs, 1, device=dev)], 0)
        s, a, s2 = torch.cat([ss[top], ts], 0), torch.cat([sa[top], ta], 0), torch.cat([ss2[top], ts2], 0)
        r, nd = torch.cat([sr[top], tr_], 0), torch.cat([snd[top], tnd], 0)
        x = torch.cat([s, a], 1)
        with torch.no_grad():
            q_t = torch.min(mlp(t1, x), mlp(t2, x))
        adv = q_t - mlp(vf, s)
        v_loss = torch.mean(torch.abs(lam - (adv < 0).float()) * adv ** 2)
        opt_v.zero_grad(); v_loss.backward(); opt_v.step()
        with torch.no_grad():
            y = r + nd * gamma * mlp(vf, s2)
        q_loss = (mask * (mlp(q1, x) - y) ** 2).mean() + (mask * (mlp(q2, x) - y) ** 2).mean()
        opt_q.zero_grad(); q_loss.backward(); opt_q.step()
        with torch.no_grad():
            for t, p in zip(t1 + t2, q1 + q2):
                t.copy_(tau * p + (1.0 - tau) * t)
        w = torch.exp(temp * adv.detach()).clamp(max=100.0)
        pi_loss = torch.mean(w * (torch.tanh(mlp(pol, s)[:, :A]) - a) ** 2)
        opt_p.zero_grad(); pi_loss.backward(); opt_p.step(); sched.step()

    target = torch.zeros(bs, bs, device=dev); target[:, 0] = 1

    def info_step():                                      # igdf.py:424-447 as written: encoder_ss on bs^2 next states
        ts, ta, ts2, _, _ = draw(1, bs)
        src_ss = draw(0, bs - 1)[2]
        ssx = torch.cat((ts2.unsqueeze(1), src_ss.unsqueeze(0).expand(bs, -1, -1)), dim=1)
        phi, psi = mlp(e_sa, torch.cat([ts, ta], 1).unsqueeze(1)), mlp(e_ss, ssx)
        logits = torch.einsum("iaz,ijz->ij", phi, psi)
        loss = F.binary_cross_entropy_with_logits(logits, target)
        opt_i.zero_grad(); loss.backward(); opt_i.step()
    return step, info_step


def make_legs(dev, bs, mfma, buffers):
    import numpy as np
    import torch
    from mobody_amd import ops
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    cfg = dict(CFG, rng="device", seed=0, batch_size=bs, mfma=mfma)
    torch.manual_seed(0); np.random.seed(0)
    igdf = call_algo("igdf", dict(cfg, graph=1), 3, dev)
    iql = call_algo("iql", dict({k: v for k, v in IQL_CFG.items()}, rng="device", seed=0, batch_size=bs, mfma=mfma, graph=1), 3, dev)
    tr = lambda p: (lambda: p.train(src, tar, bs, None, None))
    t_step, t_info = torch_legs(dev, bs, src, tar)
    legs = {"igdf": tr(igdf), "iql": tr(iql), "torch": t_step}
    if bs <= 1024:                                        # the n^2-row form holds bs^2 x 256 activations: 17 GB apiece at bs 4096
        legs["info_torch"] = t_info
    # the filter alone, on the rows a first step left staged
    f = call_algo("igdf", dict(cfg, graph=0), 3, dev)
    f.train(src, tar, bs, None, None)
    k = f._kept.numel()
    torch.cuda.synchronize()
    fgraph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(fgraph):
        f._filter(bs, k)
    sa, ss = f._encs()

    def composed():
        st = f._stage
        phi = ops.mlp3_forward(sa.blob, S + A, Z, 1, st[0][:bs], st[1][:bs], blob_T=sa.blob_T, precision=f.precision)[0]
        psi = ops.mlp3_forward(ss.blob, S, Z, 1, st[2][:bs], blob_T=ss.blob_T, precision=f.precision)[0]
        score = (phi * psi).sum(1) / (torch.linalg.norm(phi, dim=-1) * torch.linalg.norm(psi, dim=-1))
        top = torch.argsort(score)[-k:]
        batch = tuple(torch.cat([x[:bs].index_select(0, top), x[bs:]], 0) for x in st)
        w = torch.cat([torch.exp(score[top] * f.importance_weight), torch.ones(bs, device=dev)], 0)
        return batch, w
    b, w = composed()
    torch.cuda.synchronize()
    f._filter(bs, k)
    torch.cuda.synchronize()
    # (the two paths round the scores differently: among thousands of rows two scores can lie closer than that, and then the
    #  two orders differ in those rows -- recorded, not asserted)
    same_rows = bool(all(torch.equal(x, y) for x, y in zip(b, f._batch)))
    legs.update(filter_fused_replay=fgraph.replay, filter_fused_eager=lambda: f._filter(bs, k), filter_composed=composed)
    # the info step
    i_g = call_algo("igdf", dict(cfg, graph=1, info_update_step=3), 3, dev)
    i_g.update_info(src, tar, bs, None)                   # one eager step, then the capture
    assert i_g._info_graph is not None

    def info_replay():
        i_g._info_graph.replay()
    i_e = call_algo("igdf", dict(cfg, graph=0), 3, dev)
    i_e.update_info(src, tar, bs, None)
    legs.update(info_fused_replay=info_replay, info_fused_eager=lambda: i_e._info_step(bs))
    return legs, igdf, iql, (f, fgraph, i_g, i_e, same_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 256, 4096])
    ap.add_argument("--mfma", nargs="+", default=["f16x2", "f32"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src_rows", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "igdf_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_igdf.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.src_rows, rng="device", seed=100), args.src_rows, TASK, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=5000, rng="device", seed=200), 5000, TASK, 1000)
    runs = []
    for bs in args.bs:
        for mfma in args.mfma:
            legs, igdf, iql, keep = make_legs(dev, bs, mfma, (src, tar))
            for name, fn in legs.items():
                for _ in range(args.warmup):
                    fn()
            assert igdf._graph is not None and iql._graph is not None
            ms = {k: [] for k in legs}
            for _ in range(args.repeats):
                for name, fn in legs.items():             # alternating: every repeat times each leg once
                    ms[name].append(timed(fn, args.steps))
            assert all(x == x for x in igdf.losses()), "non-finite losses"
            rec = dict(bs=bs, k=int(keep[0]._kept.numel()), N=int(igdf._batch[0].shape[0]), mfma=mfma, composed_filter_same_rows=keep[4])
            for name, v in ms.items():
                rec[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
            med = lambda name: rec[name]["median_ms"]
            rec["filter_in_step_ms"] = med("igdf") - med("iql")                      # what the replayed step pays on top of IQL's
            rec["iql_plus_filter_ms"] = med("iql") + med("filter_fused_replay")     # the expectation the step is reported against
            rec["igdf_over_iql_plus_filter"] = med("igdf") / rec["iql_plus_filter_ms"]
            rec["filter_fused_over_composed"] = med("filter_fused_replay") / med("filter_composed")
            rec["filter_fused_eager_over_composed"] = med("filter_fused_eager") / med("filter_composed")
            rec["info_fused_over_torch"] = med("info_fused_replay") / med("info_torch") if "info_torch" in rec else None
            rec["igdf_over_torch"] = med("igdf") / med("torch")
            rec["filter_fused_no_slower"] = bool(med("filter_fused_eager") <= med("filter_composed"))
            runs.append(rec)
            print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"})
                              for k, v in rec.items()}), flush=True)
            del legs, igdf, iql, keep
    doc = dict(what="ms per step, walker2d shapes S=17 A=6: IGDF.train (graph replay) | bare IQL.train at the same bs (graph replay) | the "
                    "filter alone, fused (replay / eager) and composed from two mobody_mlp3_forward calls + torch | one contrastive update, "
                    "fused (replay with its gathers / eager) and in PyTorch autograd | a PyTorch-eager restatement of the whole step; medians "
                    "over alternating repeats",
               launches=LAUNCHES, src_fingerprint=bench.src_fingerprint(), device=torch.cuda.get_device_name(0), steps=args.steps,
               warmup=args.warmup, repeats=args.repeats, src_rows=args.src_rows, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        runs_ = doc.pop("runs")                               # one line per run
        head = json.dumps(doc, indent=1)
        f.write(head[:head.rindex("}")].rstrip() + ',\n "runs": [\n  ' + ",\n  ".join(json.dumps(r) for r in runs_) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
