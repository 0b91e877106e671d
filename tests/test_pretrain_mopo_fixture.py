"""Pre-training of the MOPO ablation (config mopo = 1), CPU side: a torch autograd restatement of one learn() step of the
reference (mobody_dynamics.py:300-390,594-653 with mobody_module.py:218-219,251-254,264-266,288-289) against fixture g20,
the set of trained parameters, and the C-ABI layout of the mopo training blob (csrc/pretrain.hip MobodyPretrainMopoLayout)
against a pack / unpack round trip.  The restatement (`mopo_loss`) is also the fp64 arbiter of the GPU tests."""
import numpy as np
import pytest
import torch

import golden_util as gu

TRAINED = ["reward_model1.bias", "reward_model1.weight", "reward_model2.bias", "reward_model2.weight", "reward_model3.bias",
           "reward_model3.weight", "za_src1.bias", "za_src1.weight", "za_src2.bias", "za_src2.weight", "za_src3.bias",
           "za_src3.weight"]


def mopo_params_g20(g):
    """The weights a g20 / g21 fixture was produced with, checksum verified."""
    S, A = int(g["S"]), int(g["A"])
    p = gu.gi.dyn_params(int(g["seed"]), S, A, mopo=True)
    assert abs(gu.gi.checksum(p) - float(g["wsum"])) <= 1e-9 * abs(float(g["wsum"])), "weight generator drifted from the fixture"
    return p


def _mlp(P, pre, x):
    sw = lambda z: z * torch.sigmoid(z)                 # Swish (mobody_module.py:9-15); EnsembleLinear: x @ W + b per member
    h = sw(torch.bmm(x, P[pre + "1.weight"]) + P[pre + "1.bias"])
    h = sw(torch.bmm(h, P[pre + "2.weight"]) + P[pre + "2.bias"])
    return torch.bmm(h, P[pre + "3.weight"]) + P[pre + "3.bias"]


def mopo_loss(P, s, a, s2, r, eps, use_trg, encoder_loss_coef=1.0, no_vae=False):
    """(loss, transition_loss, encoder_loss, kl_loss) of one learn() batch; P: the trained tensors (za_src1-3,
    reward_model1-3), s / a / s2 [7, b, .], r [7, b, 1], eps [7, b, S] the fake-next-state draw."""
    mu = s + _mlp(P, "za_src", torch.cat([s, a], -1))                     # forward_src == forward_trg
    T = ((mu - s2) ** 2).mean(dim=(1, 2)).sum()
    kl = lambda x: 0.05 * (-0.5 * (1 + x - x.pow(2) - x.exp())).mean(dim=(1, 2)).sum()
    KL = kl(s) + kl(s2)
    enc = 100 * 0.0 + KL + T                            # recon = 0, latent consistency = T
    fake = mu + eps * torch.std(mu, dim=0, keepdim=True)
    rh = lambda nxt: _mlp(P, "reward_model", torch.cat([s, a, nxt], -1))[..., :1]
    R = ((rh(fake) - r) ** 2).mean(dim=(1, 2)).sum() + ((rh(s2) - r) ** 2).mean(dim=(1, 2)).sum()
    loss = T + (0.0 if no_vae else (5.0 if use_trg else 1.0) * encoder_loss_coef * enc) + (1.0 if use_trg else 0.01) * R
    return loss, T, enc, KL


def mopo_step_grads(p, rows, eps, use_trg, dtype=torch.float32, **kw):
    """Losses and gradients of the restatement at weights p (numpy dict) in `dtype`."""
    P = {k: torch.tensor(np.asarray(p[k]), dtype=dtype, requires_grad=True) for k in TRAINED}
    t = lambda x: torch.tensor(np.asarray(x), dtype=dtype)
    s, a, s2, r = rows
    out = mopo_loss(P, t(s), t(a), t(s2), t(r), t(eps), use_trg, **kw)
    out[0].backward()
    return [float(x.detach()) for x in out], {k: P[k].grad.numpy() for k in TRAINED}


@pytest.mark.parametrize("tag", ["walker", "ant", "walker_novae"])
def test_torch_restatement_reproduces_the_reference_step(tag):
    g = gu.load(f"g20_pretrain_mopo_{tag}")
    S, A, b, seed = int(g["S"]), int(g["A"]), int(g["b"]), int(g["seed"])
    no_vae = bool(int(g["no_vae"]))
    p = mopo_params_g20(g)
    rng = gu.gi.noise_stream(int(g["noise_seed"]))
    rows = gu.gi.pretrain_batch(4000 + 10 * seed, b, S, A)
    eps = rng.standard_normal((7, b, S)).astype(np.float32)
    (loss, T, enc, KL), grads = mopo_step_grads(p, rows, eps, False, no_vae=no_vae)
    want = g["s0_losses"]
    if no_vae:                                          # learn()'s aliasing: (total, total, 0, 0, 0)
        np.testing.assert_allclose([loss, loss], want[:2], rtol=1e-5)
        assert (want[2:] == 0).all()
    else:
        np.testing.assert_allclose([loss, T, enc, 0.0, KL], want, rtol=1e-5, atol=1e-7)
    for k in TRAINED:
        w = g[f"s0_g::{k}"]
        scale = max(float(np.abs(g[f"s0_g::{kk}"]).max()) for kk in TRAINED if kk.split(".")[0][:3] == k[:3])
        np.testing.assert_allclose(gu.sub101(grads[k]), w, rtol=1e-5, atol=1e-5 * scale, err_msg=k)
        s64 = g[f"s0_gsum::{k}"]
        np.testing.assert_allclose((grads[k].astype(np.float64) ** 2).sum(), s64[1], rtol=1e-4, err_msg=k)


@pytest.mark.parametrize("tag", ["walker", "ant", "walker_novae"])
def test_only_the_mlp_and_the_reward_head_train(tag):
    g = gu.load(f"g20_pretrain_mopo_{tag}")
    for step in range(4):                               # both domains: encode_trg_action delegates to encode_src_action
        assert [str(x) for x in g[f"s{step}_has_grad"]] == TRAINED
    steps = {x.split("=")[0]: int(x.split("=")[1]) for x in g["adam_steps"]}
    assert steps == {k: 4 for k in steps} and sorted(steps) == TRAINED       # one Adam count, every step
    S, b = int(g["S"]), int(g["b"])
    assert [str(x) for x in g["noise_shapes"]] == [f"7,{b},{S}"] * 4          # one randn_like per step: the fake draw


@pytest.mark.parametrize("S,A", [(17, 6), (111, 8), (45, 24)])
def test_mopo_layout_matches_pack_unpack_round_trip(S, A):
    from mobody_amd import _lib, packing
    L = _lib.pretrain_mopo_layout(S, A)
    dyn, rw = _lib.mlp_layout(S + A, S, 7), _lib.mlp_layout(2 * S + A, 2, 7)
    for got, want in ((L.dyn, dyn), (L.rw, rw)):
        assert [getattr(got, f) for f, _ in got._fields_] == [getattr(want, f) for f, _ in want._fields_]
    al = lambda n: (n + 3) // 4 * 4
    assert (L.S, L.A, L.off_dyn, L.off_rw) == (S, A, 0, al(dyn.total_floats))
    assert L.total_floats == al(dyn.total_floats) + al(rw.total_floats)
    assert (L.t_off_dyn, L.t_off_rw, L.t_total_floats) == (0, al(dyn.t_total_floats), al(dyn.t_total_floats) + al(rw.t_total_floats))
    p = {k: torch.from_numpy(v) for k, v in gu.gi.dyn_params(9, S, A, mopo=True).items()}
    blob = packing.pack_pretrain_mopo(p, S, A, "cpu")
    assert blob.shape == (L.total_floats,)
    back = packing.unpack_pretrain_mopo(blob, S, A)
    assert sorted(back) == TRAINED
    for k in TRAINED:
        assert torch.equal(back[k], p[k]), k
    # the MLP region is the inference path's mopo blob (MOBODYModule.packed_mopo): one format for training and rollouts
    members = [{f"network.{li}.weight": p[f"za_src{k}.weight"][e].t() for li, k in ((0, 1), (2, 2), (4, 3))}
               | {f"network.{li}.bias": p[f"za_src{k}.bias"][e, 0] for li, k in ((0, 1), (2, 2), (4, 3))} for e in range(7)]
    assert torch.equal(blob[L.off_dyn:L.off_dyn + dyn.total_floats], packing.pack_mlp(members, S + A, S, "cpu"))
    into = {k: torch.zeros_like(v) for k, v in p.items()}
    packing.unpack_pretrain_mopo(blob, S, A, into=into)
    assert all(torch.equal(into[k], p[k]) for k in TRAINED) and not into["zs1.weight"].any()
