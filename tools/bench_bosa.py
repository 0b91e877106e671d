#!/usr/bin/env python
"""BOSA VAE-stage benchmark (one GPU): ms per call at walker2d shapes (S = 17, A = 6), the reference's widths (hidden 750, E = 5), for
batch sizes 128 (the reference's) and 4096 -- the mixed batch [tar | src] has 2 bs rows.  Legs, alternating in the same process:

  train_replay      `BOSA.train()` in the VAE stage under graph replay: both gathers, the policy-VAE step, the dynamics-VAE step
  train_eager       the same call eager
  vae_policy        mobody_bosa_vae (policy) alone on a staged batch, eager, with its Adam
  vae_dynamics      mobody_bosa_vae (dynamics) alone
  torch_policy      an eager PyTorch restatement of the policy-VAE step (autograd, torch.optim.Adam, rocBLAS) on the same GPU
  torch_dynamics    the same for the dynamics VAE (torch.baddbmm over the members)
  ll1 / ll10        `dyna_log_likelihood` at num_samples 1 and 10;  torch_ll1 / torch_ll10: its PyTorch form

Each leg is timed `--repeats` times (`--steps` calls between two device synchronisations, after `--warmup` calls of that leg), the legs
alternating; medians and the min / max spread are reported.  Also reported: the fp32 operations of the dynamics VAE's 750 x 750 layers
per step (forward, dZ W^T and X^T dZ of the two nets' middle layers: 3 x 2 x 2 x rows x 750 x 750 x E) over the dynamics step's time,
as a fraction of the fp32-MFMA peak (157.3 TFLOP/s): a whole-call rate, not a kernel's share of peak.  There is no pass threshold.
Results: one JSON document (`--out`, default profiles/bosa_vae_step.json) with the build's source fingerprint.

  python tools/bench_bosa.py [--bs 128 4096] [--steps 50] [--warmup 10] [--repeats 5]
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
from bench_iql import S, A, TASK, timed  # noqa: E402

H, E = 750, 5
PEAK_F32_MFMA = 157.3e12
CFG = dict(batch_size=128, actor_lr=3e-4, critic_lr=3e-4, gamma=0.99, state_dim=S, action_dim=A, hidden_sizes=256, max_action=1.0, tau=0.005,
           update_interval=2, expl_noise=0.2, noise_clip=0.5, vae_policy_lr=1e-3, vae_policy_hidden_dim=H, vae_policy_beta=0.5, vae_dyna_lr=1e-3,
           vae_dyna_ensemble=E, vae_dyna_hidden_dim=H, vae_dyna_beta=0.5, vae_iteration=10 ** 9, lamda_policy=0.1, lamda_dyna=0.1,
           epsilon_policy_exp=0.01, epsilon_dyna_exp=0.01, conservation_coef=0.1, num_samples=1)
LAUNCHES = dict(vae_step="26: per net forward 4 (concatenation, three products with their epilogues) and backward 6 (+1 with dX for the decoder), "
                         "k_bosa_reparam twice (forward + KL, then the seeds), k_bosa_recon, k_bosa_finish, k_wide_adam",
                loglik="10 (+1 with the mask's mean): two forwards, k_bosa_ll_sample, k_bosa_ll_reduce",
                train="the gather + 2 x 26 + the counter")


def torch_legs(dev, rows):
    """Eager PyTorch restatements: (policy-VAE step, dynamics-VAE step, dynamics estimator(n)) on `rows` fixed rows."""
    import torch
    g = torch.Generator(device=dev); g.manual_seed(0)
    s, a, s2 = torch.randn(rows, S, device=dev, generator=g), torch.rand(rows, A, device=dev, generator=g) * 2 - 1, torch.randn(rows, S, device=dev, generator=g)

    def net(members, dims):
        ps = []
        for i, o in dims:
            ps += [(torch.randn(members, i, o, device=dev, generator=g) / i ** 0.5).requires_grad_(True), torch.zeros(members, 1, o, device=dev, requires_grad=True)]
        return ps

    def mlp(p, x):
        h = torch.relu(torch.baddbmm(p[1], x, p[0]))
        return torch.relu(torch.baddbmm(p[3], h, p[2]))

    def vae(members, ein, Lz, din, dout, tanh):
        enc = net(members, ((ein, H), (H, H), (H, 2 * Lz)))
        dec = net(members, ((din, H), (H, H), (H, dout)))
        opt = torch.optim.Adam(enc + dec, lr=1e-3)

        def encode(x):
            o = torch.baddbmm(enc[5], mlp(enc, x), enc[4])
            return o[..., :Lz], torch.exp(o[..., Lz:].clamp(-4, 15))

        def decode(x):
            o = torch.baddbmm(dec[5], mlp(dec, x), dec[4])
            return torch.tanh(o) if tanh else o
        return enc, dec, opt, encode, decode
    rep = lambda t, m: t.unsqueeze(0).expand(m, -1, -1)
    _, _, p_opt, p_enc, p_dec = vae(1, S + A, 2 * A, S + 2 * A, A, True)
    _, _, d_opt, d_enc, d_dec = vae(E, 2 * S + A, 2 * S, 3 * S + A, S, False)

    def policy_step():
        mean, std = p_enc(torch.cat([s, a], 1).unsqueeze(0))
        u = p_dec(torch.cat([rep(s, 1), mean + std * torch.randn_like(std)], 2))
        loss = ((u - a) ** 2).mean() + 0.5 * (-0.5 * (1 + torch.log(std.pow(2)) - mean.pow(2) - std.pow(2)).mean())
        p_opt.zero_grad(); loss.backward(); p_opt.step()

    def dyna_step():
        mean, std = d_enc(rep(torch.cat([s, a, s2], 1), E))
        u = d_dec(torch.cat([rep(s, E), rep(a, E), mean + std * torch.randn_like(std)], 2))
        loss = ((u - s2) ** 2).mean() + 0.5 * (-0.5 * (1 + torch.log(std.pow(2)) - mean.pow(2) - std.pow(2)).mean())
        d_opt.zero_grad(); loss.backward(); d_opt.step()

    def dyna_ll(n):
        import torch.distributions as td
        sd = (0.5 / 4) ** 0.5

        def run():
            with torch.no_grad():
                mean, std = d_enc(rep(torch.cat([s, a, s2], 1), E))
                mean_n, std_n = mean.repeat(n, 1, 1, 1), std.repeat(n, 1, 1, 1)
                z = mean_n + std_n * torch.randn_like(std_n)
                x = torch.cat([rep(s, E).repeat(n, 1, 1, 1), rep(a, E).repeat(n, 1, 1, 1), z], 3)
                dec = d_dec(x.transpose(0, 1).reshape(E, n * rows, -1)).reshape(E, n, rows, S).transpose(0, 1)
                w = (td.Normal(dec, sd).log_prob(s2).sum(-1) + td.Normal(0.0, 1.0).log_prob(z).sum(-1) - td.Normal(mean_n, std_n).log_prob(z).sum(-1))
                return w.logsumexp(0) - float(torch.log(torch.tensor(float(n))))
        return run
    return policy_step, dyna_step, dyna_ll


def make_legs(dev, bs, buffers):
    import numpy as np
    import torch
    from mobody_amd.algo.call_algo import call_algo
    src, tar = buffers
    torch.manual_seed(0); np.random.seed(0)
    mk = lambda graph: call_algo("bosa", dict(CFG, rng="device", seed=0, batch_size=bs, graph=graph), 3, dev)
    g, e, one = mk(1), mk(0), mk(0)
    for p in (g, e, one):         # EnsembleFC's unit-variance weights overflow at this width: scale them by 1 / sqrt(fan_in)
        sd = p.vae_dyna.state_dict()
        p.vae_dyna.load_state_dict({k: (v / v.shape[1] ** 0.5 if k.endswith(".W") else v) for k, v in sd.items()})
    one.train(src, tar, bs, None, None)                       # stages a batch
    b = one._batch
    tr = lambda p: (lambda: p.train(src, tar, bs, None, None))

    def vae_alone(vae, opt, loss):
        def run():
            one._noise_calls += 1
            one._vae_step(vae, opt, b, loss)
        return run
    t_pol, t_dyn, t_ll = torch_legs(dev, 2 * bs)
    st = tuple(t.clone() for t in b[:3])
    legs = dict(train_replay=tr(g), train_eager=tr(e), vae_policy=vae_alone(one.vae_policy, one.vae_policy_optimizer, one._loss[0:3]),
                vae_dynamics=vae_alone(one.vae_dyna, one.vae_dyna_optimizer, one._loss[3:6]), torch_policy=t_pol, torch_dynamics=t_dyn,
                ll1=lambda: one.dyna_log_likelihood(*st, num_samples=1), ll10=lambda: one.dyna_log_likelihood(*st, num_samples=10),
                torch_ll1=t_ll(1), torch_ll10=t_ll(10))
    return legs, (g, e, one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 4096])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--src_rows", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bosa_vae_step.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_bosa.py: no GPU (a step time is a GPU measurement; there is no CPU fallback)")
    import bench
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    dev = torch.device("cuda:0")
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=args.src_rows, rng="device", seed=100), args.src_rows, TASK, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=5000, rng="device", seed=200), 5000, TASK, 1000)
    runs = []
    for bs in args.bs:
        legs, keep = make_legs(dev, bs, (src, tar))
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        assert keep[0]._graph is not None
        ms = {k: [] for k in legs}
        for _ in range(args.repeats):
            for name, fn in legs.items():                     # alternating: every repeat times each leg once
                ms[name].append(timed(fn, args.steps))
        rec = dict(bs=bs, rows=2 * bs, hidden=H, members=E)
        for name, v in ms.items():
            rec[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v), runs_ms=v)
        med = lambda name: rec[name]["median_ms"]
        flop_mid = 3 * 2 * 2.0 * (2 * bs) * H * H * E                     # the dynamics VAE's two 750 x 750 layers: fwd, dZ W^T, X^T dZ
        rec["dyn_750_layers_flop"] = flop_mid
        rec["dyn_750_layers_fraction_of_f32_mfma_peak"] = flop_mid / (med("vae_dynamics") * 1e-3) / PEAK_F32_MFMA
        for a_, b_ in (("vae_policy", "torch_policy"), ("vae_dynamics", "torch_dynamics"), ("ll1", "torch_ll1"), ("ll10", "torch_ll10")):
            rec[f"{a_}_over_{b_}"] = med(a_) / med(b_)
        rec["replay_over_eager"] = med("train_replay") / med("train_eager")
        runs.append(rec)
        print(json.dumps({k: (v if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items() if a != "runs_ms"}) for k, v in rec.items()}),
              flush=True)
        del legs, keep
    doc = dict(what="ms per call, walker2d shapes S=17 A=6, hidden 750, E=5, 2 bs mixed rows: BOSA.train in the VAE stage (graph replay | eager) | "
                    "each VAE step alone (eager) | eager PyTorch restatements of the two steps | dyna_log_likelihood at num_samples 1 and 10 and "
                    "its PyTorch form; medians over alternating repeats; exact fp32 on both sides",
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
