"""Dynamics pre-training throughput on the GPU box: optimizer steps per second of
MOBODYEnsembleDynamics.learn at the reference's batch size (256 rows per member, 7 members), walker2d shapes by default,
through the mirror (`_learn_indexed`: bootstrap gather + mobody_pretrain (gradient form) + mobody_pretrain_adam), next to the CPU
oracle (`oracle.dyn_learn_step`, torch CPU fp32 autograd).  One JSON line.

FLOPs per step (useful): per member and row, forward MACs of the three big nets are enc 2x, dec 4x, reward 2x
(S*256+65536+8192 | 4096+65536+256*S | (2S+A)*256+65536+512); forward + backward = 3x  ->  x 7 members x b rows x 2.

--mopo: the MOPO ablation (config mopo = 1) instead -- ms per optimizer step of its learn() step (graph replay and eager
fused, f16x2 and f32), the default latent step timed the same way in the same process, kernels per step, useful FLOPs, and a
PyTorch-eager restatement of the mopo loss on the same GPU; one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def flops_per_step(S, A, b):
    enc = S * 256 + 65536 + 256 * 32
    dec = 16 * 256 + 65536 + 256 * S
    rw = (2 * S + A) * 256 + 65536 + 512
    return 2.0 * 3.0 * 7 * b * (2 * enc + 4 * dec + 2 * rw)


def mopo_flops_per_step(S, A, b):
    """MOPO ablation: the MLP (S+A -> 256 -> 256 -> S) on b rows, the reward head on 2b rows; forward + backward = 3x."""
    mlp = (S + A) * 256 + 65536 + 256 * S
    rw = (2 * S + A) * 256 + 65536 + 512
    return 2.0 * 3.0 * 7 * b * (mlp + 2 * rw)


def _time_learn(dyn, data, idx, warm, b, steps):
    dyn._learn_indexed(True, data, warm, b)
    dyn._learn_indexed(True, data, idx, b)              # (graph path: captures the graph of this index matrix once, untimed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = dyn._learn_indexed(True, data, idx, b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, stats


def _launches_per_step(dyn, data, idx, b, n=8):
    """Kernels per eager optimizer step, counted by the torch profiler (None when it records no device activity)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            dyn._learn_indexed(True, data, idx[:, :n * b].contiguous(), b)
            torch.cuda.synchronize()
        k = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return len(k) / n if k else None
    except Exception:
        return None


def _eager_torch_mopo(S, A, b, data, idx, steps, lr=1e-3):
    """The mopo loss restated in PyTorch eager on the same GPU (the reference's arithmetic: EnsembleLinear bmm, Swish, the
    ensemble std, torch.optim.Adam) -- ms per optimizer step."""
    dev = data[0].device
    g = torch.Generator(device="cpu").manual_seed(1)
    P = {}
    for pre, dims in (("za_src", ((S + A, 256), (256, 256), (256, S))), ("reward_model", ((2 * S + A, 256), (256, 256), (256, 2)))):
        for k, (i, o) in enumerate(dims, 1):
            P[f"{pre}{k}.weight"] = (torch.randn(7, i, o, generator=g) / (2 * i ** 0.5)).to(dev).requires_grad_()
            P[f"{pre}{k}.bias"] = torch.zeros(7, 1, o, device=dev, requires_grad=True)
    opt = torch.optim.Adam(P.values(), lr=lr)

    def mlp(pre, x):
        h = torch.nn.functional.silu(torch.bmm(x, P[pre + "1.weight"]) + P[pre + "1.bias"])
        h = torch.nn.functional.silu(torch.bmm(h, P[pre + "2.weight"]) + P[pre + "2.bias"])
        return torch.bmm(h, P[pre + "3.weight"]) + P[pre + "3.bias"]

    def step(k):
        sel = idx[:, k * b:(k + 1) * b].long()
        s, a, s2, r = (x[sel] for x in data)
        mu = s + mlp("za_src", torch.cat([s, a], -1))
        T = ((mu - s2) ** 2).mean(dim=(1, 2)).sum()
        kl = lambda x: 0.05 * (-0.5 * (1 + x - x.pow(2) - x.exp())).mean(dim=(1, 2)).sum()
        enc = kl(s) + kl(s2) + T
        fake = mu + torch.randn_like(mu) * torch.std(mu, dim=0, keepdim=True)
        rh = lambda nxt: mlp("reward_model", torch.cat([s, a, nxt], -1))[..., :1]
        R = ((rh(fake) - r) ** 2).mean(dim=(1, 2)).sum() + ((rh(s2) - r) ** 2).mean(dim=(1, 2)).sum()
        loss = T + 5.0 * enc + R
        opt.zero_grad()
        loss.backward()
        opt.step()

    for k in range(10):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main_mopo(args):
    """--mopo: ms per optimizer step of the MOPO ablation's learn() step (graph replay and eager fused) in f16x2 and f32,
    next to the default latent step timed the same way in this process and a PyTorch-eager restatement on the GPU."""
    from mobody_amd import engine, synthetic
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    S, A, b = args.S, args.A, args.b
    dev = torch.device("cuda:0")
    task = "walker2d-medium-v2" if S == 17 else "ant-medium-v2" if S == 111 else "pen-human-v1"
    g = torch.Generator().manual_seed(0)
    mu = torch.from_numpy(synthetic.alive_mean(task, S))
    n = args.rows
    data = [(mu + 0.1 * torch.randn(n, S, generator=g)).to(dev), (torch.rand(n, A, generator=g) * 2 - 1).to(dev),
            (mu + 0.1 * torch.randn(n, S, generator=g)).to(dev), torch.randn(n, 1, generator=g).to(dev)]
    idx = torch.randint(n, (7, args.steps * b), generator=g).to(device=dev, dtype=torch.int32).contiguous()
    warm = idx[:, :20 * b].contiguous()
    out = dict(metric="dynamics pre-training ms per optimizer step, MOPO ablation vs default latent model", S=S, A=A,
               rows_per_member=b, steps=args.steps, ms={}, launches_per_step={},
               useful_flops_per_step=dict(mopo=mopo_flops_per_step(S, A, b), latent=flops_per_step(S, A, b)))
    kinds, paths = (("mopo",), ("graph",)) if args.mopo_only else (("mopo", "latent"), ("graph", "eager"))
    for mfma in ("f16x2", "f32"):
        for kind in kinds:
            for path in paths:
                cfg = engine.default_config(S, A, no_vae=0, inverse_sep_reward_loss=0, train_together=0, train_with_src_threshold=1,
                                            dynamics_lr=1e-3, mfma=mfma, mopo=int(kind == "mopo"), train_graph=int(path == "graph"))
                m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg)
                dyn = MOBODYEnsembleDynamics(cfg, m, None, None, get_termination_fn(task), penalty_coef=0.1, rng="device", seed=1)
                ms, stats = _time_learn(dyn, data, idx, warm, b, args.steps)
                out["ms"][f"{kind}_{path}_{mfma}"] = ms
                if path == "eager" and mfma == "f16x2":
                    out["launches_per_step"][kind] = _launches_per_step(dyn, data, idx, b)
                if kind == "mopo" and path == "graph":
                    out[f"mopo_mean_losses_{mfma}"] = stats
    ms = out["ms"]
    if args.mopo_only:                                  # (a kernel-trace run: the library's kernels only, no torch work timed)
        print(json.dumps(out))
        return
    ms["torch_eager_mopo_f32"] = _eager_torch_mopo(S, A, b, data, idx, min(args.steps, 200))
    out["mopo_ms_per_step"] = ms["mopo_graph_f16x2"]
    out["mopo_over_latent"] = {m_: ms[f"mopo_graph_{m_}"] / ms[f"latent_graph_{m_}"] for m_ in ("f16x2", "f32")}
    out["torch_eager_over_mopo"] = {m_: ms["torch_eager_mopo_f32"] / ms[f"mopo_graph_{m_}"] for m_ in ("f16x2", "f32")}
    out["useful_tflops_mopo_f16x2"] = mopo_flops_per_step(S, A, b) / (ms["mopo_graph_f16x2"] * 1e-3) / 1e12
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=17); ap.add_argument("--A", type=int, default=6)
    ap.add_argument("--b", type=int, default=256); ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--no_cpu", action="store_true")
    ap.add_argument("--mfma", default="f16x2", choices=["f32", "f16x2"])
    ap.add_argument("--mopo", action="store_true", help="the MOPO ablation's step (config mopo = 1) against the latent step")
    ap.add_argument("--mopo_only", action="store_true", help="with --mopo: time the mopo graph-replay step only (kernel traces)")
    args = ap.parse_args()
    if args.mopo:
        return main_mopo(args)
    from mobody_amd import engine, synthetic
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn
    S, A, b = args.S, args.A, args.b
    dev = torch.device("cuda:0")
    task = "walker2d-medium-v2" if S == 17 else "ant-medium-v2" if S == 111 else "pen-human-v1"
    cfg = engine.default_config(S, A, no_vae=0, inverse_sep_reward_loss=0, train_together=0, train_with_src_threshold=1, dynamics_lr=1e-3,
                                mfma=args.mfma)
    m = MOBODYModule(S, A, 256, 7, 5, device=dev, config=cfg)
    dyn = MOBODYEnsembleDynamics(cfg, m, None, None, get_termination_fn(task), penalty_coef=0.1, rng="device", seed=1)
    g = torch.Generator().manual_seed(0)
    mu = torch.from_numpy(synthetic.alive_mean(task, S))
    n = args.rows
    data = [(mu + 0.1 * torch.randn(n, S, generator=g)).to(dev), (torch.rand(n, A, generator=g) * 2 - 1).to(dev),
            (mu + 0.1 * torch.randn(n, S, generator=g)).to(dev), torch.randn(n, 1, generator=g).to(dev)]
    idx = torch.randint(n, (7, args.steps * b), generator=g).to(device=dev, dtype=torch.int32).contiguous()
    warm = idx[:, :20 * b].contiguous()
    dyn._learn_indexed(True, data, warm, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = dyn._learn_indexed(True, data, idx, b)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = dict(metric="dynamics pre-training optimizer steps/sec", S=S, A=A, rows_per_member=b, steps=args.steps,
               steps_per_sec=args.steps / dt, ms_per_step=dt / args.steps * 1e3, samples_per_sec=args.steps * b / dt,
               useful_tflops=flops_per_step(S, A, b) * args.steps / dt / 1e12, frac_f32_mfma_peak=flops_per_step(S, A, b) * args.steps / dt / 157.3e12,
               mean_losses=stats)
    if not args.no_cpu:
        from oracle import mobody_oracle as O
        threads = min(16, len(os.sched_getaffinity(0)))
        torch.set_num_threads(threads)
        rng = np.random.default_rng(0)
        p = {k: v.cpu().numpy() for k, v in m.state_dict().items()}
        st = O.DynTrainState(p)
        rows = [x[:7 * b].reshape(7, b, -1).cpu().numpy() for x in data]
        nz = [rng.standard_normal((7, b, 16)).astype(np.float32) for _ in range(6)] + [rng.standard_normal((7, b, S)).astype(np.float32)]
        O.dyn_learn_step(st, *rows, nz, True)
        t0 = time.time(); k = 0
        while time.time() - t0 < 8.0 or k < 3:
            O.dyn_learn_step(st, *rows, nz, True); k += 1
        out["cpu_baseline"] = dict(steps_per_sec=k / (time.time() - t0), cores=threads, kind="port",
                                   sample=f"{k} oracle learn steps (torch CPU fp32 autograd, {threads} threads)")
        out["gpu_over_cpu"] = out["steps_per_sec"] / out["cpu_baseline"]["steps_per_sec"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
