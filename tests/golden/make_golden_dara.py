"""Generate the DARA fixtures (g25) by running the REAL reference `DARA` (algo/offline_offline/dara.py) on the CPU.

Same conventions as make_golden_iql.py: runs only where the reference checkout is available, stores the reference's outputs and
small explicit inputs, regenerates the weights from `gen_inputs.mlp_params` (checksums stored).  S = 17, A = 6, bs = 32 (N = 64);
policy, twin-Q and V are g24's (same seed, same `q_scale`); the classifier's heads are `mlp_params(701, S + A, 2)` and
`mlp_params(702, 2 S + A, 2)` with their output layers scaled by `c_scale` (stored), so that |p1 - p0| of the heads spans a real
range and the relabel moves the rewards: the script asserts that in step 1 of every variant max |eta * penalty| exceeds 1e-3, and
that |penalty| <= 2 everywhere (head probabilities lie in [0, 1]: the reference's +-10 clamp cannot bind).

The trajectory must be one that arithmetic can follow.  Adam's update of an entry whose gradient lies near its eps (1e-8) is
lr g / (|g| + eps): a rounding difference of 5e-10 in g moves the parameter by 0.05 lr.  The two-class seed sums to zero up to its
own fp32 rounding (dz3[:, 0] + dz3[:, 1] ~ 1e-10), so a layer-2 unit k whose two output weights nearly agree gets
dz2[:, k] = d (W3[0][k] - W3[1][k]) + that residue, a whole row of W2 in this regime, and from step 2 on dW3 = dz3^T h2 of the
reference's own fp32 run differs from ANY other correct evaluation by ~1e-6 against a scale of 0.03 -- 30 x the tests' gradient
tolerance.  Whether the drawn weights hold such a unit is a property of the seeds: of the pairs (701 + 2 i, 702 + 2 i), i = 0 .. 15,
seven do (the fp64 restatement of tests/dara_ref.py leaves the reference's step 2 .. 6 gradients by 3 to 80 x the tolerance; i = 0
by 7.6 x) and nine do not (at most 0.45 x).  The script takes the first pair that does not, (703, 704), and asserts
it: in every variant and step the restatement reproduces the reference's classifier gradients within HALF of rtol 1e-5, atol 1e-5 x
the head's largest entry (measured 0.08), its post-step parameters within 0.05 lr (measured 0.003 lr) and its penalties within 5e-6
(measured 4e-7).  For the same reason c_scale is 2 and not larger (at (701, 702) and c_scale 8 the reference lies 0.25 lr and 2e-5 in
the penalties from the restatement after step 1).  The criterion reads the reference and the fp64 restatement only.

  g25_dara_default   eta 0.1, dara_eta 0; two train() steps
  g25_dara_eta2      dara_eta 2.0 (overrides eta); two train() steps
  g25_dara_short     max_step 8; six train() steps

Per step: the classifier's `randperm` and both noise draws as the reference drew them (`s{step}_perm`, `s{step}_noise_sas`,
`s{step}_noise_sa`: row i of the noise belongs to batch row perm[i] of src[:bs] | tar[:bs]), the two classifier losses
(`cls_loss_sas`, `cls_loss_sa`), the classifier's gradients thinned by sub() plus their fp64 [sum, sum of squares]
(`s{step}_cls_g::*`, `..._gsum::*`) and post-step parameters (`s{step}_cls_p::*`), the penalty of all bs source rows
(`s{step}_penalty`), the rewards that reached the critic (`s{step}_reward`, all N rows) and what g24 stores for V, Q and the policy.
`ckpt_*`: the key lists of the six files the reference's save() writes.

Usage:  python tests/golden/make_golden_dara.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (puts the reference on sys.path)
from make_golden import FixedRB, gi, sub, save, load_mlp  # noqa: E402
from make_golden_iql import iql_cfg, iql_params, SEED, Q_SCALE  # noqa: E402
import algo.offline_offline.dara as ref_dara  # noqa: E402

VARIANTS = dict(default=dict(), eta2=dict(dara_eta=2.0), short=dict(max_step=8))
STEPS = dict(default=2, eta2=2, short=6)
SEED_SA, SEED_SAS, C_SCALE = 703, 704, 2.0


def dara_cfg(S, A, **over):
    cfg = iql_cfg(S, A, gaussian_noise_std=1.0, eta=0.1, dara_eta=0)
    cfg.update(over)
    return cfg


def classifier_params(S, A, c_scale=C_SCALE):
    pc = {}
    for pre, sd_, n_in in (("sa_classifier.", SEED_SA, S + A), ("sas_classifier.", SEED_SAS, 2 * S + A)):
        p = gi.mlp_params(sd_, n_in, 2)
        p["network.4.weight"] = (p["network.4.weight"] * np.float32(c_scale)).astype(np.float32)
        p["network.4.bias"] = (p["network.4.bias"] * np.float32(c_scale)).astype(np.float32)
        pc.update({pre + k: v for k, v in p.items()})
    return pc


def assert_reproducible(tag, out, cfg, rows, bs, S, A):
    """The fp64 restatement of the same steps (tests/dara_ref.py) follows the reference's run: see the module docstring."""
    for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dara_ref as DR
    st = DR.ClassifierState(classifier_params(S, A), cfg["actor_lr"])
    worst = dict(grad=0.0, param=0.0, pen=0.0)
    for step in range(1, STEPS[tag] + 1):
        res = st.step(rows, DR.step_noise(out, step), cfg["gaussian_noise_std"])
        for pre in DR.HEADS:
            ks = [k for k in res["grads"] if k.startswith(pre)]
            scale = max(np.abs(out[f"s{step}_cls_g::{k}"]).max() for k in ks)
            for k in ks:
                want = out[f"s{step}_cls_g::{k}"].astype(np.float64)
                worst["grad"] = max(worst["grad"], float((np.abs(sub(res["grads"][k]) - want) / (1e-5 * scale + 1e-5 * np.abs(want))).max()))
        worst["param"] = max(worst["param"], max(float(np.abs(sub(st.p[k]) - out[f"s{step}_cls_p::{k}"]).max()) for k in st.p) / cfg["actor_lr"])
        pen = DR.relabel(st.p, rows, bs, 1.0)[0]
        worst["pen"] = max(worst["pen"], float(np.abs(pen - out[f"s{step}_penalty"]).max()))
    print("dara", tag, "fp64 restatement vs the reference: gradients %.3g x tolerance, parameters %.3g lr, penalties %.3g" %
          (worst["grad"], worst["param"], worst["pen"]))
    assert worst["grad"] <= 0.5 and worst["param"] <= 0.05 and worst["pen"] <= 5e-6, (tag, worst)


def g25():
    S, A, bs = 17, 6, 32
    for tag, over in VARIANTS.items():
        cfg = dara_cfg(S, A, **over)
        pol = ref_dara.DARA(cfg, torch.device("cpu"))
        pa, pq, pv = iql_params(S, A)
        pc = classifier_params(S, A)
        load_mlp(pol.policy, pa); load_mlp(pol.q_funcs, pq); load_mlp(pol.target_q_funcs, pq); load_mlp(pol.v_func, pv)
        load_mlp(pol.classifier, pc)
        out = dict(S=S, A=A, bs=bs, seed=SEED, q_scale=Q_SCALE, c_scale=C_SCALE, seed_sa=SEED_SA, seed_sas=SEED_SAS, eta=pol.eta,
                   wsum_actor=gi.checksum(pa), wsum_q=gi.checksum(pq), wsum_v=gi.checksum(pv), wsum_cls=gi.checksum(pc),
                   cfg_keys=np.array(sorted(over)), cfg_vals=np.array([str(over[k]) for k in sorted(over)]))
        rows_src, rows_tar = gi.batch(501, 64, S, A), gi.batch(502, 64, S, A)
        src = FixedRB(rows_src); tar = FixedRB(rows_tar)
        rec = dict(v_loss=[], q_loss=[], pi_loss=[], adv=[], lr=[], reward=[], cls_loss=[], cls_grad=[])
        o_v, o_q, o_pi = pol.update_v_function, pol.update_q_functions, pol.update_policy

        def uv(*a, **k):
            loss, adv = o_v(*a, **k)
            rec["v_loss"].append(float(loss.detach())); rec["adv"].append(adv.detach().numpy().reshape(-1).copy())
            return loss, adv

        def uq(state, action, reward, *a, **k):
            rec["reward"].append(reward.detach().numpy().reshape(-1).copy())
            o = o_q(state, action, reward, *a, **k); rec["q_loss"].append(float(o.detach())); return o

        def up(*a, **k):
            o = o_pi(*a, **k); rec["pi_loss"].append(float(o.detach())); return o

        pol.update_v_function, pol.update_q_functions, pol.update_policy = uv, uq, up
        o_step = pol.classifier_optimizer.step

        def cls_step(*a, **k):                         # the gradients the one optimizer over both heads is about to apply
            rec["cls_grad"].append({n: p.grad.numpy().copy() for n, p in pol.classifier.named_parameters()})
            return o_step(*a, **k)

        pol.classifier_optimizer.step = cls_step
        short = tag == "short"
        for step in range(1, STEPS[tag] + 1):
            rec["lr"].append(pol.policy_optimizer.param_groups[0]["lr"])
            taps = dict(perm=None, noise=[], ce=[])
            o_perm, o_randn, o_ce = torch.randperm, torch.randn_like, ref_dara.F.cross_entropy

            def randperm(n, **k):
                p = o_perm(n, **k); taps["perm"] = p.numpy().copy(); return p

            def randn_like(x, **k):
                e = o_randn(x); taps["noise"].append(e.numpy().copy()); return e

            def cross_entropy(*a, **k):
                o = o_ce(*a, **k); taps["ce"].append(float(o.detach())); return o

            torch.randperm, torch.randn_like, ref_dara.F.cross_entropy = randperm, randn_like, cross_entropy
            try:
                torch.manual_seed(5 + step)
                pol.train(src, tar, bs, None, None)
            finally:
                torch.randperm, torch.randn_like, ref_dara.F.cross_entropy = o_perm, o_randn, o_ce
            assert len(taps["noise"]) == 2 and len(taps["ce"]) == 2       # the noise-free pass of the relabel draws none
            out[f"s{step}_perm"] = taps["perm"]; out[f"s{step}_noise_sas"] = taps["noise"][0]; out[f"s{step}_noise_sa"] = taps["noise"][1]
            rec["cls_loss"].append(taps["ce"])                              # (loss_sas, loss_sa), the order of dara.py:218-219
            # the penalty of the source rows, from the reference's own classifier (unchanged since the relabel of this step)
            with torch.no_grad():
                s, a, s2 = [torch.from_numpy(np.asarray(x[:bs])) for x in rows_src[:3]]
                sas_p, sa_p = pol.classifier(s, a, s2, with_noise=False)
                ls, la = torch.log(torch.softmax(sas_p, -1) + 1e-10), torch.log(torch.softmax(sa_p, -1) + 1e-10)
                pen = (ls[:, 1] - la[:, 1] - ls[:, 0] + la[:, 0]).numpy()
            assert np.abs(pen).max() <= 2.0, np.abs(pen).max()
            r0 = np.asarray(rows_src[3][:bs]).reshape(-1)
            np.testing.assert_allclose(rec["reward"][-1][:bs], r0 + pol.eta * pen, rtol=1e-5, atol=1e-6)
            assert np.array_equal(rec["reward"][-1][bs:], np.asarray(rows_tar[3][:bs]).reshape(-1))
            if step == 1:
                assert np.abs(pol.eta * pen).max() > 1e-3, (tag, np.abs(pol.eta * pen).max())
            out[f"s{step}_penalty"] = pen; out[f"s{step}_reward"] = rec["reward"][-1]; out[f"s{step}_adv"] = rec["adv"][-1]
            for k, v in pol.classifier.state_dict().items():
                out[f"s{step}_cls_p::{k}"] = sub(v.numpy())
            for k, g in rec["cls_grad"][-1].items():
                out[f"s{step}_cls_g::{k}"] = sub(g)
                out[f"s{step}_cls_gsum::{k}"] = np.array([g.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()])
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
        for k in ("v_loss", "q_loss", "pi_loss", "lr"):
            out[k] = np.array(rec[k], np.float64)
        out["cls_loss_sas"] = np.array([c[0] for c in rec["cls_loss"]], np.float64)
        out["cls_loss_sa"] = np.array([c[1] for c in rec["cls_loss"]], np.float64)
        opts = (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer, pol.classifier_optimizer)
        out["opt_steps"] = np.array([opt.state_dict()["state"][0]["step"] for opt in opts])
        out["last_epoch"] = pol.policy_lr_schedule.last_epoch
        out["calls_src"] = np.array(src.calls); out["calls_tar"] = np.array(tar.calls); out["total_it"] = pol.total_it
        with tempfile.TemporaryDirectory() as tmp:      # what torch writes for the reference class: file names and key lists
            pol.save(os.path.join(tmp, "model"))
            out["ckpt_files"] = np.array(sorted(os.listdir(tmp)))
            cl = torch.load(os.path.join(tmp, "model_classifier"))
            co = torch.load(os.path.join(tmp, "model_classifier_optimizer"))
            out["ckpt_classifier_keys"] = np.array(list(cl))
            out["ckpt_classifier_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in cl.values()])
            out["ckpt_cls_opt_params"] = np.array(co["param_groups"][0]["params"])
            out["ckpt_cls_opt_state_keys"] = np.array(sorted(co["state"]))
            out["ckpt_cls_opt_group_keys"] = np.array(sorted(co["param_groups"][0]))
            out["ckpt_cls_opt_entry_keys"] = np.array(sorted(co["state"][0]))
            out["ckpt_cls_opt_shapes"] = np.array(["x".join(str(d) for d in co["state"][i]["exp_avg"].shape) for i in sorted(co["state"])])
        print("dara", tag, "cls", rec["cls_loss"][:2], "max|eta pen|", np.abs(pol.eta * out["s1_penalty"]).max(), "v", rec["v_loss"][:2],
              "q", rec["q_loss"][:2], "pi", rec["pi_loss"][:2], "calls", src.calls, tar.calls)
        rows = tuple(np.concatenate([np.asarray(x[:bs]), np.asarray(y[:bs])], 0) for x, y in zip(rows_src, rows_tar))
        assert_reproducible(tag, {k: np.asarray(v) for k, v in out.items()}, cfg, rows, bs, S, A)
        save(f"g25_dara_{tag}", **out)


if __name__ == "__main__":
    g25()
