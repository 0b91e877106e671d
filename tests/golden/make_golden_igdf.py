"""Generate the IGDF fixtures (g26) by running the REAL reference `IGDF` (algo/offline_offline/igdf.py) on the CPU.

Same conventions as make_golden_dara.py: runs only where the reference checkout is available, stores the reference's outputs and
small explicit inputs, regenerates the weights from `gen_inputs.mlp_params` (checksums stored).  S = 17, A = 6; policy, twin-Q and V
are g24's (same seed, same `q_scale`); the two encoders are `mlp_params(seed_sa, S + A, 64)` and `mlp_params(seed_ss, S, 64)` with
their output layers scaled by `e_scale` (stored).  Every variant runs `update_info` (three steps, tar(bs) then src(bs - 1) of the
fixed rows) and then its train() steps.

  g26_igdf_default   xi 0.75, importance_weight 1.0, bs 32 -> k 24, N 56; two train() steps
  g26_igdf_all       xi 1.0: nothing dropped, all rows re-ordered
  g26_igdf_one       xi 0.04 -> k = 1; importance_weight 3.0
  g26_igdf_odd       bs 33 -> k 24, N 57; the contrast runs on 33 + 32 rows (crosses the 32-row tile)
  g26_igdf_short     max_step 8; six train() steps

Two conditions are asserted; they read the reference's results and the fp64 restatement (tests/igdf_ref.py) only.
  * Selection gap.  The selection is discontinuous: in every step of every variant adjacent scores in sorted order, among the kept
    rows and across the keep / drop boundary, differ by at least 1e-4 -- ten times the fp32 parity tolerance (atol 1e-5) on a
    quantity in [-1, 1].  The score is a cosine, so the output layers' scale does not move it: the gap is a property of the seeds.
  * A trajectory arithmetic can follow (the lesson of g25 about Adam near its eps): the restatement reproduces the reference's
    encoder gradients within HALF of rtol 1e-5, atol 1e-5 x the encoder's largest entry, and its post-step parameters within
    0.05 lr.
The script walks the seed pairs (801 + 2 i, 802 + 2 i) and takes the first that meets both at bs 32 and bs 33; what it measured is
printed and stored (`gap_min`, `restate_grad`, `restate_param`).

Per info step (variants default and odd; the other variants run the same three steps on the same rows as default): the loss
(`info_loss`), the encoders' gradients thinned by sub() plus their fp64 [sum, sum of squares] (`i{step}_g::*`, `i{step}_gsum::*`)
and post-step parameters (`i{step}_p::*`).  Per train() step: the scores of all bs source rows (`s{step}_score`), the kept
positions in the order they reached the critic (`s{step}_kept`), the row weights (`s{step}_w`), the rows and rewards that reached
the critic (`s{step}_state` thinned, `s{step}_reward`), and what g24 stores for V, Q and the policy.

Usage:  python tests/golden/make_golden_igdf.py
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
from make_golden_iql import iql_params, SEED, Q_SCALE  # noqa: E402
import algo.offline_offline.igdf as ref_igdf  # noqa: E402

for p_ in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import igdf_ref as GR  # noqa: E402

E_SCALE = 4.0
GAP = 1e-4


def run_variant(tag, seed_sa, seed_ss, S=17, A=6):
    """The reference's run of one variant; returns the fixture dict and the measured (gap, gradient, parameter) figures."""
    over, bs = GR.VARIANTS[tag], GR.BS[tag]
    cfg = GR.igdf_cfg(S, A, **over)
    torch.manual_seed(0)
    pol = ref_igdf.IGDF(cfg, torch.device("cpu"))
    pa, pq, pv = iql_params(S, A)
    pe = GR.info_params(S, A, seed_sa, seed_ss, cfg["repr_dim"], E_SCALE)
    load_mlp(pol.policy, pa); load_mlp(pol.q_funcs, pq); load_mlp(pol.target_q_funcs, pq); load_mlp(pol.v_func, pv)
    load_mlp(pol.info, pe)
    assert [k for k, _ in pol.info.named_parameters()] == list(GR.PARAM_ORDER)
    k = GR.kept_rows(bs, cfg["xi"])
    out = dict(S=S, A=A, bs=bs, k=k, seed=SEED, q_scale=Q_SCALE, e_scale=E_SCALE, seed_sa=seed_sa, seed_ss=seed_ss,
               wsum_actor=gi.checksum(pa), wsum_q=gi.checksum(pq), wsum_v=gi.checksum(pv), wsum_info=gi.checksum(pe),
               cfg_keys=np.array(sorted(over)), cfg_vals=np.array([str(over[x]) for x in sorted(over)]))
    rows_src, rows_tar = gi.batch(501, 64, S, A), gi.batch(502, 64, S, A)
    src, tar = FixedRB(rows_src), FixedRB(rows_tar)
    # ---- update_info: three steps --------------------------------------------------------------------------------------------
    rec = dict(loss=[], grad=[], param=[])
    o_step, o_bce = pol.info_optimizer.step, torch.nn.functional.binary_cross_entropy_with_logits

    def info_opt_step(*a, **kw):
        rec["grad"].append({n: p.grad.numpy().copy() for n, p in pol.info.named_parameters()})
        r = o_step(*a, **kw)
        rec["param"].append({n: p.detach().numpy().copy() for n, p in pol.info.named_parameters()})
        return r

    def bce(*a, **kw):
        o = o_bce(*a, **kw); rec["loss"].append(float(o.detach())); return o

    pol.info_optimizer.step = info_opt_step
    torch.nn.functional.binary_cross_entropy_with_logits = bce
    try:
        pol.update_info(src, tar, bs, None)
    finally:
        torch.nn.functional.binary_cross_entropy_with_logits = o_bce
        pol.info_optimizer.step = o_step
    assert len(rec["loss"]) == GR.INFO_STEPS and src.calls == [bs - 1] * GR.INFO_STEPS and tar.calls == [bs] * GR.INFO_STEPS
    out["info_loss"] = np.array(rec["loss"], np.float64)
    st = GR.InfoState(pe, cfg["actor_lr"])
    tar_rows, src_s2 = [np.asarray(x[:bs]) for x in rows_tar], np.asarray(rows_src[2][:bs - 1])
    worst = dict(grad=0.0, param=0.0, loss=0.0)
    for step in range(1, GR.INFO_STEPS + 1):
        res = st.step(tar_rows, src_s2)
        g, p = rec["grad"][step - 1], rec["param"][step - 1]
        worst["loss"] = max(worst["loss"], abs(res["loss"] - rec["loss"][step - 1]) / abs(res["loss"]))
        for pre in GR.ENCS:
            ks = [x for x in g if x.startswith(pre)]
            scale = max(np.abs(g[x]).max() for x in ks)
            for x in ks:
                want = g[x].astype(np.float64)
                worst["grad"] = max(worst["grad"], float((np.abs(res["grads"][x] - want) / (1e-5 * scale + 1e-5 * np.abs(want))).max()))
                worst["param"] = max(worst["param"], float(np.abs(st.p[x] - p[x]).max()) / cfg["actor_lr"])
        if tag in ("default", "odd"):
            for x in g:
                out[f"i{step}_g::{x}"] = sub(g[x])
                out[f"i{step}_gsum::{x}"] = np.array([g[x].astype(np.float64).sum(), (g[x].astype(np.float64) ** 2).sum()])
                out[f"i{step}_p::{x}"] = sub(p[x])
    # ---- train(): the filter and IQL's three phases ---------------------------------------------------------------------------
    tr = dict(v_loss=[], q_loss=[], pi_loss=[], adv=[], lr=[], reward=[], state=[], w=[], score=[], order=[])
    o_v, o_q, o_pi = pol.update_v_function, pol.update_q_functions, pol.update_policy

    def uv(*a, **kw):
        loss, adv = o_v(*a, **kw)
        tr["v_loss"].append(float(loss.detach())); tr["adv"].append(adv.detach().numpy().reshape(-1).copy())
        return loss, adv

    def uq(state, action, reward, nextstate, not_done, mask, *a, **kw):
        tr["state"].append(state.detach().numpy().copy()); tr["reward"].append(reward.detach().numpy().reshape(-1).copy())
        tr["w"].append(mask.detach().numpy().reshape(-1).copy())
        o = o_q(state, action, reward, nextstate, not_done, mask, *a, **kw); tr["q_loss"].append(float(o.detach())); return o

    def up(*a, **kw):
        o = o_pi(*a, **kw); tr["pi_loss"].append(float(o.detach())); return o

    pol.update_v_function, pol.update_q_functions, pol.update_policy = uv, uq, up
    src.calls, tar.calls = [], []
    short = tag == "short"
    gap_min = np.inf
    for step in range(1, GR.STEPS[tag] + 1):
        tr["lr"].append(pol.policy_optimizer.param_groups[0]["lr"])
        o_argsort = torch.argsort

        def argsort(x, *a, **kw):
            o = o_argsort(x, *a, **kw); tr["score"].append(x.detach().numpy().copy()); tr["order"].append(o.numpy().copy()); return o

        torch.argsort = argsort
        try:
            pol.train(src, tar, bs, None)
        finally:
            torch.argsort = o_argsort
        score, kept = tr["score"][-1], tr["order"][-1][bs - k:]
        srt = np.sort(score.astype(np.float64))
        gaps = np.diff(srt[max(bs - k - 1, 0):])                    # among the kept rows and across the keep / drop boundary
        if len(gaps):
            gap_min = min(gap_min, float(gaps.min()))
        out[f"s{step}_score"] = score; out[f"s{step}_kept"] = kept.astype(np.int32); out[f"s{step}_w"] = tr["w"][-1]
        out[f"s{step}_state"] = sub(tr["state"][-1]); out[f"s{step}_reward"] = tr["reward"][-1]; out[f"s{step}_adv"] = tr["adv"][-1]
        # what reached the critic is [kept src rows | tar rows], the weights exp(iw score) | 1
        assert np.array_equal(tr["state"][-1], np.concatenate([np.asarray(rows_src[0])[kept], np.asarray(rows_tar[0][:bs])], 0))
        np.testing.assert_allclose(tr["w"][-1][:k], np.exp(cfg["importance_weight"] * score[kept].astype(np.float64)), rtol=1e-6)
        assert np.array_equal(tr["w"][-1][k:], np.ones(bs, np.float32))
        nets = (("actor", pol.policy),) if short else (("v", pol.v_func), ("q", pol.q_funcs), ("qt", pol.target_q_funcs), ("actor", pol.policy))
        for nm, mod in nets:
            for x, v in mod.state_dict().items():
                out[f"s{step}_{nm}_p::{x}"] = sub(v.numpy())
        if short:
            continue
        for nm, mod in (("v", pol.v_func), ("q", pol.q_funcs), ("actor", pol.policy)):
            for x, v in mod.named_parameters():
                g = v.grad.numpy()
                out[f"s{step}_{nm}_g::{x}"] = sub(g)
                out[f"s{step}_{nm}_gsum::{x}"] = np.array([g.astype(np.float64).sum(), (g.astype(np.float64) ** 2).sum()])
    for x in ("v_loss", "q_loss", "pi_loss", "lr"):
        out[x] = np.array(tr[x], np.float64)
    opts = (pol.v_optimizer, pol.q_optimizer, pol.policy_optimizer, pol.info_optimizer)
    out["opt_steps"] = np.array([opt.state_dict()["state"][0]["step"] for opt in opts])
    out["last_epoch"] = pol.policy_lr_schedule.last_epoch
    out["calls_src"] = np.array(src.calls); out["calls_tar"] = np.array(tar.calls); out["total_it"] = pol.total_it
    with tempfile.TemporaryDirectory() as tmp:      # what torch writes for the reference class: the file names (no encoder)
        pol.save(os.path.join(tmp, "model"))
        out["ckpt_files"] = np.array(sorted(os.listdir(tmp)))
    out["info_keys"] = np.array(list(pol.info.state_dict()))
    out["info_shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in pol.info.state_dict().values()])
    # the restatement's filter on the encoders it arrived at: the same rows in the same order
    sc = GR.scores(st.p, [np.asarray(x[:bs]) for x in rows_src])
    assert np.array_equal(GR.select(sc, k), out["s1_kept"]), tag
    np.testing.assert_allclose(sc, out["s1_score"], rtol=0, atol=5e-6)
    out["gap_min"], out["restate_grad"], out["restate_param"] = gap_min, worst["grad"], worst["param"]
    return out, dict(gap=gap_min, **worst)


def g26():
    for i in range(32):
        seeds = (801 + 2 * i, 802 + 2 * i)
        try:
            figs = {tag: run_variant(tag, *seeds)[1] for tag in ("all", "odd")}     # every row kept: the whole score vector counts
        except AssertionError as exc:
            print("seeds", seeds, "refused:", str(exc)[:120]); continue
        print("seeds", seeds, figs)
        if all(f["gap"] >= GAP and f["grad"] <= 0.5 and f["param"] <= 0.05 for f in figs.values()):
            break
    else:
        raise SystemExit("no seed pair meets the two conditions")
    for tag in GR.VARIANTS:
        out, f = run_variant(tag, *seeds)
        print("igdf", tag, "seeds", seeds, "k", int(out["k"]), "info loss", out["info_loss"], "min gap %.3g" % f["gap"],
              "restatement: gradients %.3g x tolerance, parameters %.3g lr, loss %.3g" % (f["grad"], f["param"], f["loss"]),
              "v", out["v_loss"][:2], "q", out["q_loss"][:2], "pi", out["pi_loss"][:2])
        assert f["gap"] >= GAP and f["grad"] <= 0.5 and f["param"] <= 0.05, (tag, f)
        save(f"g26_igdf_{tag}", **out)


if __name__ == "__main__":
    g26()
