"""Generate the MOPO-ablation pre-training fixtures (g20 / g21) by running the REAL reference with config mopo = 1.

Same conventions as make_golden.py (whose helpers it imports and which it leaves unchanged): runs only where the
reference checkout is available, stores the reference's outputs and small explicit inputs, regenerates the weights from
`gen_inputs.dyn_params(seed, S, A, mopo=True)` (checksum stored as `wsum`) and the fake-next-state noise from
`gen_inputs.noise_stream(noise_seed)` (NoiseTap).

  g20_pretrain_mopo_{walker,ant}   four learn() calls (src, trg, src, trg): losses, every gradient, post-step parameters,
                                   has_grad, Adam step counts, noise shapes
  g20_pretrain_mopo_walker_novae   the walker run with no_vae = 1
  g21_dyn_train_mopo               train() end to end (max_epochs = 2, 150 + 90 rows, batch 32), as g13
  g21_mopo_dynamics_pth.json       key -> shape of the reference mopo module's state_dict

Usage:  python tests/golden/make_golden_mopo.py [g20] [g21]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path)
from make_golden import NoiseTap, CudaAlias, sub101, save, gi  # noqa: E402
from algo.dynamics.mobody_module import MOBODYModule  # noqa: E402
from algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics  # noqa: E402
from algo.mb_utils.terminal_funs import get_termination_fn  # noqa: E402

MOPO_CFG = dict(mg.PRE_CFG, mopo=1)


def make_mopo_trainer(S, A, seed, lr=1e-3, **cfg_over):
    p = gi.dyn_params(seed, S, A, mopo=True)
    cfg = dict(MOPO_CFG, **cfg_over)
    m = MOBODYModule(S, A, 256, 7, 5, device="cpu", config=dict(cfg))
    sd = m.state_dict()
    for k, v in p.items():
        assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
        sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd)
    opt = torch.optim.Adam(m.parameters(), lr=lr)                 # train_mobody.py:801-804
    dyn = MOBODYEnsembleDynamics(dict(cfg), m, opt, None, get_termination_fn("walker2d-medium-v2"), penalty_coef=0.1)
    dyn.total_steps = 0
    return dyn, m, p


def g20():
    for tag, S, A, b, seed, over in (("walker", 17, 6, 24, 311, {}), ("ant", 111, 8, 20, 312, {}),
                                     ("walker_novae", 17, 6, 24, 311, dict(no_vae=1))):
        dyn, m, p = make_mopo_trainer(S, A, seed, **over)
        out = dict(S=S, A=A, b=b, seed=seed, wsum=gi.checksum(p), noise_seed=2200 + seed, lr=1e-3,
                   no_vae=int(over.get("no_vae", 0)))
        with NoiseTap(2200 + seed) as tap, CudaAlias():
            for step, use_trg in enumerate((False, True, False, True)):
                rows = gi.pretrain_batch(4000 + 10 * seed + step, b, S, A)
                res = dyn.learn(use_trg, *[torch.from_numpy(x) for x in rows], b, 0.01)
                out[f"s{step}_losses"] = np.array(res, np.float64)
                for k, v in m.named_parameters():
                    # post-step values of the trained layers only: the others must stay bit-identical to the regenerated
                    # weights (the tests check that against gen_inputs directly)
                    if v.grad is not None and not k.startswith(("max_", "min_", "elites")):
                        g = v.grad.numpy()
                        out[f"s{step}_g::{k}"] = sub101(g)
                        out[f"s{step}_gsum::{k}"] = np.array([g.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()])
                        out[f"s{step}_p::{k}"] = sub101(v.detach().numpy())
                out[f"s{step}_has_grad"] = np.array(sorted(k for k, v in m.named_parameters() if v.grad is not None))
        out["noise_shapes"] = np.array([",".join(map(str, sh)) for sh in tap.shapes])
        st = dyn.optim.state_dict()["state"]
        names = [k for k, _ in m.named_parameters()]
        out["adam_steps"] = np.array([f"{names[i]}={int(float(v['step']))}" for i, v in st.items()])
        print("pretrain mopo", tag, [out[f"s{k}_losses"][0] for k in range(4)], "noise calls", len(tap.shapes))
        save(f"g20_pretrain_mopo_{tag}", **out)


def g21():
    S, A, bs, seed = 17, 6, 32, 321
    dyn, m, p = make_mopo_trainer(S, A, seed)
    src = gi.batch(911, 150, S, A); trg = gi.batch(912, 90, S, A)
    rec = []
    o_val = dyn.validate

    def validate(*a, **k):
        r = o_val(*a, **k); rec.append(np.array([r[0], r[1]], np.float64)); return r

    dyn.validate = validate
    torch.manual_seed(43); np.random.seed(43)
    with NoiseTap(2300) as tap, CudaAlias():
        dyn.train(tuple(torch.from_numpy(x) for x in src), tuple(torch.from_numpy(x) for x in trg), max_epochs=2, batch_size=bs)
    sd = m.state_dict()
    out = dict(S=S, A=A, bs=bs, seed=seed, wsum=gi.checksum(p), noise_seed=2300, rng_seed=43, lr=1e-3, n_src=150, n_trg=90,
               validate=np.stack(rec), elites=sd["elites"].numpy(), n_noise=len(tap.shapes), total_steps=dyn.total_steps)
    for k, v in sd.items():
        if k.split(".")[0] in ("za_src1", "za_src2", "za_src3", "reward_model1", "reward_model2", "reward_model3"):
            out["sd::" + k] = sub101(v.numpy())
    print("train mopo: elites", out["elites"], "validate calls", len(rec), "noise calls", len(tap.shapes), "steps", dyn.total_steps)
    save("g21_dyn_train_mopo", **out)
    sd = MOBODYModule(S, A, 256, 7, 5, device="cpu", config=dict(MOPO_CFG)).state_dict()
    js = dict(S=S, A=A, keys=[dict(name=k, shape=list(v.shape), dtype=str(v.dtype).replace("torch.", "")) for k, v in sd.items()])
    path = os.path.join(HERE, "g21_mopo_dynamics_pth.json")
    with open(path, "w") as f:
        json.dump(js, f, indent=1)
    print("wrote g21_mopo_dynamics_pth", "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    for w in sys.argv[1:] or ["g20", "g21"]:
        globals()[w]()
