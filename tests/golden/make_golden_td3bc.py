"""Generate the TD3_BC fixtures (g23) by running the REAL reference `TD3BC` (algo/offline_offline/td3_bc.py) for two
`train()` steps.

Same conventions as make_golden.py (whose helpers it imports and which it leaves unchanged): runs only where the reference
checkout is available, stores the reference's outputs and small explicit inputs, regenerates the weights from
`gen_inputs.mlp_params` (checksums stored).  S = 17, A = 6, bs = 32 and the weights of g7().

  g23_td3bc_default     advantage=0, bc_coef=1, trg_ratio=1 (N = 64)
  g23_td3bc_adv         advantage=1: BC weighted by min(exp(q/mean|q|), 100), gradient through the weight
  g23_td3bc_adv_bc05    advantage=1, bc_coef=0.05, trg_ratio=0.5 (N = 48: a ragged 32-row tile)
  g23_td3bc_dara        penalty_type='dara': update_classifier every step + 0.1 * penalty on the source rewards; the
                        classifier's weights are g9()'s; per step the permutation and both noise draws are stored
                        (`s{step}_perm`, `s{step}_noise_sas`, `s{step}_noise_sa`; rows = src[:bs] | tar[:bs], labels 0 | 1
                        before the permutation), the rewards that reached the critic (`s{step}_reward`) and the classifier's
                        post-step parameters (`s{step}_cls_p::*`)

Per step: `q_loss`, `pi_loss`, every parameter gradient thinned by sub() plus its fp64 [sum, sum of squares]
(`s{step}_{q,actor}_g::*`, `..._gsum::*`), post-step parameters of actor, twin-Q and target (`s{step}_{q,actor,qt}_p::*`) and
the sample() call counts (`calls_src`, `calls_tar`).

Usage:  python tests/golden/make_golden_td3bc.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (puts the reference on sys.path)
from make_golden import FixedRB, RngTap, gi, sub, save, load_mlp, policy_cfg  # noqa: E402
from algo.offline_offline.td3_bc import TD3BC  # noqa: E402

VARIANTS = dict(default={}, adv=dict(advantage=1), adv_bc05=dict(advantage=1, bc_coef=0.05, trg_ratio=0.5),
                dara=dict(penalty_type="dara"))
SEED = 401


def g23():
    S, A, bs = 17, 6, 32
    for tag, over in VARIANTS.items():
        cfg = policy_cfg(S, A, **over)
        pol = TD3BC(cfg, torch.device("cpu"))
        pa = {"network." + k: v for k, v in gi.mlp_params(SEED, S, A).items()}
        pq = {}
        for j, sd_ in ((1, SEED + 1), (2, SEED + 2)):
            pq.update({f"network{j}." + k: v for k, v in gi.mlp_params(sd_, S + A, 1).items()})
        load_mlp(pol.policy, pa); load_mlp(pol.q_funcs, pq); load_mlp(pol.target_q_funcs, pq)
        out = dict(S=S, A=A, bs=bs, seed=SEED, wsum_actor=gi.checksum(pa), wsum_q=gi.checksum(pq),
                   cfg_keys=np.array(sorted(over)), cfg_vals=np.array([str(over[k]) for k in sorted(over)]))
        dara = cfg["penalty_type"] == "dara"
        if dara:
            pc = {}
            pc.update({"sa_classifier." + k: v for k, v in gi.mlp_params(701, S + A, 2).items()})
            pc.update({"sas_classifier." + k: v for k, v in gi.mlp_params(702, 2 * S + A, 2).items()})
            load_mlp(pol.classifier, pc)
            out.update(seed_sa=701, seed_sas=702, wsum_cls=gi.checksum(pc))
        src = FixedRB(gi.batch(501, 64, S, A)); tar = FixedRB(gi.batch(502, 64, S, A))
        rec = dict(q_loss=[], pi_loss=[], reward=[])
        o_q, o_pi = pol.update_q_functions, pol.update_policy

        def uq(state, action, reward, *a, **k):
            rec["reward"].append(reward.detach().numpy().copy())
            o = o_q(state, action, reward, *a, **k); rec["q_loss"].append(float(o.detach())); return o

        def up(*a, **k):
            o = o_pi(*a, **k); rec["pi_loss"].append(float(o.detach())); return o

        pol.update_q_functions, pol.update_policy = uq, up
        for step in (1, 2):
            taps = dict(perm=None, noise=[])
            o_perm, o_randn = torch.randperm, torch.randn_like

            def randperm(n, **k):
                p = o_perm(n, **k); taps["perm"] = p.numpy().copy(); return p

            def randn_like(x, **k):
                e = o_randn(x); taps["noise"].append(e.numpy().copy()); return e

            torch.randperm, torch.randn_like = randperm, randn_like
            try:
                np.random.seed(9)
                torch.manual_seed(5 + step)
                with RngTap(600 + step):
                    pol.train(src, tar, bs, None, None)
            finally:
                torch.randperm, torch.randn_like = o_perm, o_randn
            if dara:
                assert len(taps["noise"]) == 2, len(taps["noise"])        # the noise-free pass of the penalty draws none
                out[f"s{step}_perm"] = taps["perm"]; out[f"s{step}_noise_sas"] = taps["noise"][0]
                out[f"s{step}_noise_sa"] = taps["noise"][1]; out[f"s{step}_reward"] = rec["reward"][-1]
                for k, v in pol.classifier.named_parameters():
                    out[f"s{step}_cls_p::{k}"] = sub(v.detach().numpy())
            for nm, mod in (("q", pol.q_funcs), ("actor", pol.policy), ("qt", pol.target_q_funcs)):
                for k, v in mod.state_dict().items():
                    out[f"s{step}_{nm}_p::{k}"] = sub(v.numpy())
            for nm, mod in (("q", pol.q_funcs), ("actor", pol.policy)):
                for k, v in mod.named_parameters():
                    g = v.grad.numpy()
                    out[f"s{step}_{nm}_g::{k}"] = sub(g)
                    out[f"s{step}_{nm}_gsum::{k}"] = np.array([g.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()])
        out["q_loss"] = np.array(rec["q_loss"]); out["pi_loss"] = np.array(rec["pi_loss"])
        out["calls_src"] = np.array(src.calls); out["calls_tar"] = np.array(tar.calls); out["total_it"] = pol.total_it
        print("td3bc", tag, "q_loss", rec["q_loss"], "pi_loss", rec["pi_loss"], "calls", src.calls, tar.calls)
        save(f"g23_td3bc_{tag}", **out)


if __name__ == "__main__":
    g23()
