"""Generate the IQL fixtures (g24) by running the REAL reference `IQL` (algo/offline_offline/iql.py).

Same conventions as make_golden_td3bc.py: runs only where the reference checkout is available, stores the reference's outputs
and small explicit inputs, regenerates the weights from `gen_inputs.mlp_params` (checksums stored).  S = 17, A = 6, bs = 32
(N = 64); the policy is the S -> 2 A net.  The output layer of both Q nets is scaled by `q_scale` (stored) so that the
advantages straddle the clamp of the policy weight: the script asserts that, in the first step of every variant, at least one row
has temp * adv above ln 100 and at least one below.

  g24_iql_default        lam 0.7, temp 3, max_step 500000; two train() steps
  g24_iql_lam09_temp10   lam 0.9, temp 10; two train() steps
  g24_iql_short          max_step 8, six train() steps: the policy's learning rate at each step (`lr`) and its parameters after
                         each -- two steps at max_step 500000 move the rate by 1e-11 and pin nothing of the schedule

Per step: `v_loss`, `q_loss`, `pi_loss`, `s{step}_adv` (all N rows), every parameter gradient thinned by sub() plus its fp64
[sum, sum of squares] (`s{step}_{v,q,actor}_g::*`, `..._gsum::*`), post-step parameters of the four nets
(`s{step}_{v,q,qt,actor}_p::*`; `short` stores the policy's alone), the optimizers' step counts (`opt_steps`: v, q, policy) and the
sample() call counts.

Usage:  python tests/golden/make_golden_iql.py
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (puts the reference on sys.path)
from make_golden import FixedRB, gi, sub, save, load_mlp  # noqa: E402
from algo.offline_offline.iql import IQL  # noqa: E402

VARIANTS = dict(default=dict(), lam09_temp10=dict(lam=0.9, temp=10.0), short=dict(max_step=8))
STEPS = dict(default=2, lam09_temp10=2, short=6)
SEED, Q_SCALE = 431, 16.0


def iql_cfg(S, A, **over):
    cfg = dict(gamma=0.99, tau=0.005, update_interval=2, state_dim=S, action_dim=A, hidden_sizes=256, max_action=1.0,
               critic_lr=3e-4, actor_lr=3e-4, lam=0.7, temp=3.0, max_step=500000)
    cfg.update(over)
    return cfg


def iql_params(S, A, seed=SEED, q_scale=Q_SCALE):
    pa = {"network." + k: v for k, v in gi.mlp_params(seed, S, 2 * A).items()}
    pq = {}
    for j, sd_ in ((1, seed + 1), (2, seed + 2)):
        p = gi.mlp_params(sd_, S + A, 1)
        p["network.4.weight"] = (p["network.4.weight"] * np.float32(q_scale)).astype(np.float32)
        p["network.4.bias"] = (p["network.4.bias"] * np.float32(q_scale)).astype(np.float32)
        pq.update({f"network{j}." + k: v for k, v in p.items()})
    pv = {"network." + k: v for k, v in gi.mlp_params(seed + 3, S, 1).items()}
    return pa, pq, pv


def g24():
    S, A, bs = 17, 6, 32
    for tag, over in VARIANTS.items():
        cfg = iql_cfg(S, A, **over)
        pol = IQL(cfg, torch.device("cpu"))
        pa, pq, pv = iql_params(S, A)
        load_mlp(pol.policy, pa); load_mlp(pol.q_funcs, pq); load_mlp(pol.target_q_funcs, pq); load_mlp(pol.v_func, pv)
        out = dict(S=S, A=A, bs=bs, seed=SEED, q_scale=Q_SCALE, wsum_actor=gi.checksum(pa), wsum_q=gi.checksum(pq),
                   wsum_v=gi.checksum(pv), cfg_keys=np.array(sorted(over)), cfg_vals=np.array([str(over[k]) for k in sorted(over)]))
        src = FixedRB(gi.batch(501, 64, S, A)); tar = FixedRB(gi.batch(502, 64, S, A))
        rec = dict(v_loss=[], q_loss=[], pi_loss=[], adv=[], lr=[])
        o_v, o_q, o_pi = pol.update_v_function, pol.update_q_functions, pol.update_policy

        def uv(*a, **k):
            loss, adv = o_v(*a, **k)
            rec["v_loss"].append(float(loss.detach())); rec["adv"].append(adv.detach().numpy().reshape(-1).copy())
            return loss, adv

        def uq(*a, **k):
            o = o_q(*a, **k); rec["q_loss"].append(float(o.detach())); return o

        def up(*a, **k):
            o = o_pi(*a, **k); rec["pi_loss"].append(float(o.detach())); return o

        pol.update_v_function, pol.update_q_functions, pol.update_policy = uv, uq, up
        short = tag == "short"
        for step in range(1, STEPS[tag] + 1):
            rec["lr"].append(pol.policy_optimizer.param_groups[0]["lr"])
            torch.manual_seed(5 + step)
            pol.train(src, tar, bs, None, None)
            out[f"s{step}_adv"] = rec["adv"][-1]
            nets = (("actor", pol.policy),) if short else (("v", pol.v_func), ("q", pol.q_funcs), ("qt", pol.target_q_funcs), ("actor", pol.policy))
            for nm, mod in nets:
                for k, v in mod.state_dict().items():
                    out[f"s{step}_{nm}_p::{k}"] = sub(v.numpy())
            if short:
                continue
            for nm, mod in (("v", pol.v_func), ("q", pol.q_funcs), ("actor", pol.policy)):
                for k, v in mod.named_parameters():
                    g = v.grad.numpy()
                    out[f"s{step}_{nm}_g::{k}"] = sub(g)
                    out[f"s{step}_{nm}_gsum::{k}"] = np.array([g.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()])
        x = cfg["temp"] * rec["adv"][0]
        assert (x > math.log(100.0)).any() and (x < math.log(100.0)).any(), (tag, x.min(), x.max())
        for k in ("v_loss", "q_loss", "pi_loss", "lr"):
            out[k] = np.array(rec[k], np.float64)
        out["opt_steps"] = np.array([opt.state_dict()["state"][0]["step"] for opt in (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer)])
        out["last_epoch"] = pol.policy_lr_schedule.last_epoch
        out["calls_src"] = np.array(src.calls); out["calls_tar"] = np.array(tar.calls); out["total_it"] = pol.total_it
        print("iql", tag, "v", rec["v_loss"][:2], "q", rec["q_loss"][:2], "pi", rec["pi_loss"][:2], "temp*adv", x.min(), x.max(),
              "clamped rows", int((x > math.log(100.0)).sum()), "lr", rec["lr"])
        save(f"g24_iql_{tag}", **out)


if __name__ == "__main__":
    g24()
