"""Generate the fixtures of BOSA's critic / actor stage (g28) by running the REAL reference `BOSA` (algo/offline_offline/bosa.py) on the CPU.

Same conventions as make_golden_bosa.py.  Variants `small` and `tiny` of bosa_ref.VARIANTS; vae_iteration = 0, so the first train() call
is already a stage-2 call; four calls, the actor steps at calls 2 and 4 (update_interval 2).  The VAE weights come from
bosa_ref.vae_params (1 / sqrt(fan_in) scaling, as g27's), the actor's and the two critics' from gen_inputs.mlp_params; `torch.randn_like`
is recorded per call (`c{call}_noise_target` raw, `_dynamics`, `_policy`); the rows are fixed (FixedRB).  FixedRB hands the rows'
fifth column to the reference as `done`, so the not_done the step sees is 1 - that column (`not_done`).  Per call: the reference's
logged scalars (`c{call}_log::*`, its local log_dict, read when train() returns), the mask computed as the reference computes it from
its own fp32 ll (`c{call}_mask`), `total_it`, and the parameters of the five nets thinned by sub() (`c{call}_p::{net}::{name}`).

epsilon_dyna_exp: a first run records the fp64 min-ll of the four calls (the draws do not depend on the threshold); the threshold is the
middle of the widest gap of the pooled values around their median (bosa_ref.mask_threshold); the second run uses it.

Asserted, and stored as measured (the script walks seeds 951, 952, ... and the log_std head's (bias, scale) until all hold in fp64):
  (a) on each call between 25 % and 75 % of the rows pass the mask and no row's min_ll lies within ten estimator tolerances of
      log(epsilon_dyna_exp) (`mask_margin`: the smallest distance over that tolerance; `mask_ratio` per call);
  (b) no pre-clamp log_std of either VAE lies within 1e-3 of -4 or 15 and values fall on both sides of -4 (`clamp_margin`);
  (c) the restatement (tests/bosa2_ref.stage2_call) gives the reference's masks exactly, its scalars within half of rtol 1e-5 and its
      parameters within 0.05 lr, g27's bound (`restate_param`, in lr; `restate_scalar`, over half of rtol 1e-5).

Usage:  python tests/golden/make_golden_bosa2.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (puts the reference on sys.path)
from make_golden import FixedRB, gi, sub, save  # noqa: E402
import algo.offline_offline.bosa as ref_bosa  # noqa: E402

for p_ in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import bosa2_ref as B2  # noqa: E402
import bosa_ref as BR  # noqa: E402
from make_golden_bosa import Miss, load  # noqa: E402

SETTINGS = ((-4.0, 2.0), (-4.5, 2.0), (-5.0, 4.0), (-3.5, 1.0))
TAGS = ("small", "tiny")
LR = 3e-4


def nets_of(pol):
    return {"actor": pol.actor, "actor_target": pol.actor_target, "critic_1": pol.critic_1, "critic_2": pol.critic_2,
            "critic_1_target": pol.critic_1_target, "critic_2_target": pol.critic_2_target}


def run_reference(tag, seed, setting, eps_exp):
    """Four calls of the reference; (per-call records, inputs)."""
    S, A, H, E, bs = BR.VARIANTS[tag]
    cfg = BR.bosa_cfg(S, A, H, E, vae_iteration=0, epsilon_dyna_exp=eps_exp)
    torch.manual_seed(seed)
    pol = ref_bosa.BOSA(cfg, torch.device("cpu"))
    vae = {"policy": BR.vae_params(seed, "policy", S, A, H, 1, *setting), "dynamics": BR.vae_params(seed + 50, "dynamics", S, A, H, E, *setting)}
    load(pol.vae_policy, BR.state_dict(*vae["policy"], "policy"))
    load(pol.vae_dyna, BR.state_dict(*vae["dynamics"], "dynamics"))
    actor_sd = gi.mlp_params(seed + 1, S, A)
    q_sd = {"network%d.%s" % (j, k): v for j in (1, 2) for k, v in gi.mlp_params(seed + 1 + j, S + A, 1).items()}
    as_ref = lambda sd, pre: {k[len(pre):].replace("network.", "net."): torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}
    pol.actor.load_state_dict(as_ref(actor_sd, "")); pol.actor_target.load_state_dict(as_ref(actor_sd, ""))
    for j, (c, ct) in enumerate(((pol.critic_1, pol.critic_1_target), (pol.critic_2, pol.critic_2_target)), 1):
        c.load_state_dict(as_ref(q_sd, "network%d." % j)); ct.load_state_dict(as_ref(q_sd, "network%d." % j))
    rows_src, rows_tar = gi.batch(501, 64, S, A), gi.batch(502, 64, S, A)
    mixed = [np.concatenate([t[:bs], s[:bs]]) for s, t in zip(rows_src, rows_tar)]
    mixed[4] = (1.0 - mixed[4]).astype(np.float32)                    # the fifth column reaches the reference as `done`
    noise, o_randn, lls, logs = [], torch.randn_like, [], []

    def randn_like(t, *a, **kw):
        e = o_randn(t, *a, **kw)
        noise.append(e.numpy().copy())
        return e
    o_ll = pol.vae_dyna.importance_sampling_estimator
    pol.vae_dyna.importance_sampling_estimator = lambda *a, **kw: (lls.append(o_ll(*a, **kw)), lls[-1])[1]
    code = ref_bosa.BOSA.train.__code__

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is code:
            logs.append(dict(frame.f_locals.get("log_dict", {})))
    src, tar = FixedRB(rows_src), FixedRB(rows_tar)
    calls = []
    torch.randn_like = randn_like
    try:
        for call in (1, 2, 3, 4):
            del noise[:], lls[:], logs[:]
            sys.setprofile(prof)
            try:
                pol.train(src, tar, bs, None)
            finally:
                sys.setprofile(None)
            assert len(noise) == (3 if call % 2 == 0 else 2) and len(lls) == 1 and len(logs) == 1, (len(noise), len(lls), len(logs))
            lo = lls[0].min(dim=0)[0].numpy()
            rec = dict(total_it=pol.total_it, log=logs[0], mask=(lo > np.log(eps_exp)).astype(np.float32),
                       noise=dict(target=noise[0], dynamics=noise[1], **({"policy": noise[2]} if call % 2 == 0 else {})),
                       params={n: {k: v.numpy().copy() for k, v in m.state_dict().items()} for n, m in nets_of(pol).items()})
            calls.append(rec)
    finally:
        torch.randn_like = o_randn
    return calls, dict(cfg=cfg, vae=vae, actor_sd=actor_sd, q_sd=q_sd, mixed=mixed)


def restate(calls, inp):
    """The restatement over the recorded noise: per-call logs and the state after each call."""
    st = B2.stage2_init(inp["actor_sd"], inp["q_sd"])
    out = []
    for rec in calls:
        logs = B2.stage2_call(st, inp["vae"]["policy"], inp["vae"]["dynamics"], inp["mixed"], rec["noise"], inp["cfg"])
        out.append((logs, {k: {q: v.copy() for q, v in st[k].items()} for k in B2.ACTOR_KEYS + B2.CRITIC_KEYS}))
    return out


def ref_params(rec):
    """The reference's parameters of one call in the restatement's form: {net: parameter dict}."""
    as_sd = lambda sd, pre: {pre + k.replace("net.", "network."): v for k, v in sd.items()}
    p = rec["params"]
    out = {"actor": B2.twin_from_state_dict(as_sd(p["actor"], ""), ("",)), "actor_target": B2.twin_from_state_dict(as_sd(p["actor_target"], ""), ("",))}
    for name, suffix in (("critic", ""), ("critic_target", "_target")):
        sd = dict(as_sd(p["critic_1" + suffix], "network1."), **as_sd(p["critic_2" + suffix], "network2."))
        out[name] = B2.twin_from_state_dict(sd)
    return out


def run_variant(tag, seed, setting):
    S, A, H, E, bs = BR.VARIANTS[tag]
    calls, inp = run_reference(tag, seed, setting, 0.01)              # first run: where the min-ll values lie
    pooled, tols = [], []
    for rec in calls:
        ll64, w64 = BR.loglik(*inp["vae"]["dynamics"], "dynamics", *inp["mixed"][:3], rec["noise"]["dynamics"], 0.5)
        pooled.append(ll64)
        tols.append(BR.estimator_tolerance(ll64, w64))
    thr, gap, _ = BR.mask_threshold(np.concatenate(pooled, 1), np.concatenate(tols, 1))
    eps_exp = float(np.exp(thr))
    calls, inp = run_reference(tag, seed, setting, eps_exp)
    res = restate(calls, inp)
    worst = dict(param=0.0, scalar=0.0, mask_margin=np.inf, clamp=np.inf)
    ratios = []
    for call, (rec, (logs, state), ll64, tol) in enumerate(zip(calls, res, pooled, tols), 1):
        ratio = float(logs["mask"].mean())
        ratios.append(ratio)
        margin = float((np.abs(logs["min_ll"] - np.log(eps_exp)) / tol.max(0)).min())
        if not (0.25 <= ratio <= 0.75 and margin > 10.0):
            raise Miss(f"(a) call {call}: mask ratio {ratio:.2f}, margin {margin:.1f} tolerances")
        worst["mask_margin"] = min(worst["mask_margin"], margin)
        pres = [BR.encode(inp["vae"]["dynamics"][0], "dynamics", *inp["mixed"][:3])[1]]
        if "pi" in logs:
            pres.append(BR.encode(inp["vae"]["policy"][0], "policy", inp["mixed"][0], logs["pi"], None)[1])
        for pre in pres:
            m = float(min(np.abs(pre + 4).min(), np.abs(pre - 15).min()))
            if not (m > 1e-3 and (pre < -4).any() and (pre > -4).any()):
                raise Miss(f"(b) call {call}: margin {m:.2e}, below {(pre < -4).sum()} of {pre.size}")
            worst["clamp"] = min(worst["clamp"], m)
        if not np.array_equal(rec["mask"], logs["mask"].astype(np.float32)):
            raise Miss(f"(c) call {call}: masks differ")
        for k, v in rec["log"].items():
            worst["scalar"] = max(worst["scalar"], abs(float(logs[k]) - v) / (0.5e-5 * abs(v) + 1e-300))
        want = ref_params(rec)
        for net in want:
            lr = inp["cfg"]["actor_lr" if net.startswith("actor") else "critic_lr"]
            for q in want[net]:
                worst["param"] = max(worst["param"], float(np.abs(state[net][q] - want[net][q]).max() / lr))
        if worst["scalar"] > 1.0 or worst["param"] > 0.05:
            raise Miss(f"(c) call {call}: scalar {worst['scalar']:.2f} of half rtol 1e-5, param {worst['param']:.4f} lr")
        assert rec["total_it"] == call and set(rec["log"]) == set(B2.STAGE2_SCALARS[:4] + (B2.STAGE2_SCALARS[4:] if call % 2 == 0 else ()))
    out = dict(S=S, A=A, hidden=H, E=E, bs=bs, seed=seed, log_std_bias=setting[0], log_std_scale=setting[1], epsilon_dyna_exp=eps_exp,
               not_done=inp["mixed"][4], mask_ratio=np.array(ratios), mask_margin=worst["mask_margin"], clamp_margin=worst["clamp"],
               restate_param=worst["param"], restate_scalar=worst["scalar"],
               wsum_actor=gi.checksum(inp["actor_sd"]), wsum_critic=gi.checksum(inp["q_sd"]))
    for call, rec in enumerate(calls, 1):
        out[f"c{call}_total_it"], out[f"c{call}_mask"] = rec["total_it"], rec["mask"]
        for k, v in rec["noise"].items():
            out[f"c{call}_noise_{k}"] = v
        for k, v in rec["log"].items():
            out[f"c{call}_log::{k}"] = v
        for net, sd in rec["params"].items():
            for k, v in sd.items():
                out[f"c{call}_p::{net}::{k}"] = sub(v)
    return out


def main():
    for tag in TAGS:
        done = None
        for seed in range(951, 1011):
            for setting in SETTINGS:
                try:
                    done = run_variant(tag, seed, setting)
                    break
                except Miss as m:
                    print(f"  {tag} seed {seed} {setting}: {m}")
            if done is not None:
                break
        assert done is not None, tag
        print(f"{tag}: seed {done['seed']} (bias, scale) ({done['log_std_bias']}, {done['log_std_scale']}), epsilon_dyna_exp {done['epsilon_dyna_exp']:.4g}: "
              f"mask ratios {done['mask_ratio']}, mask margin {done['mask_margin']:.1f} tolerances, clamp margin {done['clamp_margin']:.2e}, "
              f"restatement scalars {done['restate_scalar']:.3f} of half rtol 1e-5, parameters {done['restate_param']:.4f} lr")
        save("g28_bosa2_" + tag, **done)


if __name__ == "__main__":
    main()
