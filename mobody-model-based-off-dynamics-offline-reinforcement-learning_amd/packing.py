"""Reference state_dict tensors <-> the packed weight blobs the HIP kernels stream.

Plumbing only (torch pad/transposes, run once per load/save): the layouts come from the C
ABI (`mobody_dyn_layout`, `mobody_mlp_layout`), so there is one source of truth.

  dynamics : `<layer>.weight [E,in,out]`, `<layer>.bias [E,1,out]`  (mobody_module.py:383-389)
             -> per layer W[E][Kp][Np] (zero padded; only the inference halves of the
                latent / reward heads), bias[E][Np]
  MLP      : `network.{0,2,4}.weight [out,in]`, `.bias [out]`        (mobody.py:35-48)
             -> per member W1[Kp1][256] b1 W2[256][256] b2 W3[256][Np3] b3  (W = weight.T)
"""
import torch

from . import _lib

MLP_KEYS = ("network.0", "network.2", "network.4")


def wide_pack(W):
    """[..., K, 256] row-major -> the kernels' K-interleaved-by-4 storage [..., K/4, 256, 4] (csrc/tile.h wide_idx)."""
    *lead, K, N = W.shape
    assert N == 256 and K % 4 == 0
    return W.reshape(*lead, K // 4, 4, N).transpose(-1, -2).contiguous()


def wide_unpack(flat, K):
    """Inverse of wide_pack for one matrix: flat [K*256] -> [K, 256]."""
    return flat.reshape(K // 4, 256, 4).transpose(-1, -2).reshape(K, 256)


def pack_dynamics(params, S, A, device):
    """params: dict name -> array/tensor in the reference layout. Returns a flat fp32 device blob."""
    L = _lib.dyn_layout(S, A)
    blob = torch.zeros(L.total_floats, dtype=torch.float32, device=device)
    for li, name in enumerate(_lib.DL_NAMES):
        lay = L.layer[li]
        W = torch.as_tensor(params[name + ".weight"], dtype=torch.float32).to(device)
        b = torch.as_tensor(params[name + ".bias"], dtype=torch.float32).to(device)
        E, K, _ = W.shape
        assert E == L.E and K == lay.in_dim, (name, tuple(W.shape), lay.in_dim)
        n = lay.out_dim                                    # leading `out_dim` columns = the half inference uses
        Wp = torch.zeros(E, lay.Kp, lay.Np, dtype=torch.float32, device=device)
        Wp[:, :K, :n] = W[:, :, :n]
        bp = torch.zeros(E, lay.Np, dtype=torch.float32, device=device)
        bp[:, :n] = b[:, 0, :n]
        if lay.Np == 256:                                   # 256-wide matrices use the interleaved storage
            Wp = wide_pack(Wp)
        blob[lay.w_off:lay.w_off + Wp.numel()] = Wp.reshape(-1)
        blob[lay.b_off:lay.b_off + bp.numel()] = bp.reshape(-1)
    return blob


def pack_mlp(member_params, in_dim, out_dim, device, prefixes=None):
    """member_params: list (one per member) of dicts with `network.{0,2,4}.{weight,bias}` keys
    (nn.Linear layout), or one dict plus `prefixes` (e.g. ['network1.', 'network2.'] for twin-Q)."""
    if prefixes is not None:
        member_params = [{k[len(p):]: v for k, v in member_params.items() if k.startswith(p)} for p in prefixes]
    M = len(member_params)
    L = _lib.mlp_layout(in_dim, out_dim, M)
    blob = torch.zeros(L.total_floats, dtype=torch.float32, device=device)
    for m, p in enumerate(member_params):
        base = m * L.member_floats
        g = lambda k: torch.as_tensor(p[k], dtype=torch.float32).to(device)
        W1, W2, W3 = g("network.0.weight"), g("network.2.weight"), g("network.4.weight")
        assert W1.shape == (256, in_dim) and W2.shape == (256, 256) and W3.shape == (out_dim, 256), \
            "packed MLPs are in->256->256->out (hidden_sizes must be 256)"
        w1 = torch.zeros(L.Kp1, 256, device=device); w1[:in_dim] = W1.t()
        w3 = torch.zeros(256, L.Np3, device=device); w3[:, :out_dim] = W3.t()
        b3 = torch.zeros(L.Np3, device=device); b3[:out_dim] = g("network.4.bias")
        for off, t in ((L.w1, wide_pack(w1)), (L.b1, g("network.0.bias")), (L.w2, wide_pack(W2.t().contiguous())),
                       (L.b2, g("network.2.bias")), (L.w3, w3), (L.b3, b3)):
            blob[base + off:base + off + t.numel()] = t.reshape(-1)
    return blob


def unpack_mlp(blob, in_dim, out_dim, members):
    """Inverse of pack_mlp: list of dicts in nn.Linear layout (clones)."""
    L = _lib.mlp_layout(in_dim, out_dim, members)
    out = []
    for m in range(members):
        base = m * L.member_floats
        v = lambda off, n: blob[base + off:base + off + n]
        out.append({
            "network.0.weight": wide_unpack(v(L.w1, L.Kp1 * 256), L.Kp1)[:in_dim].t().contiguous(),
            "network.0.bias": v(L.b1, 256).clone(),
            "network.2.weight": wide_unpack(v(L.w2, 65536), 256).t().contiguous(),
            "network.2.bias": v(L.b2, 256).clone(),
            "network.4.weight": v(L.w3, 256 * L.Np3).view(256, L.Np3)[:, :out_dim].t().contiguous(),
            "network.4.bias": v(L.b3, L.Np3)[:out_dim].clone(),
        })
    return out


# ---- dynamics pre-training blob (csrc/pretrain.hip, MobodyPretrainLayout) ------------------------------------------
PRETRAIN_NETS = (("enc", ("zs1", "zs2", "zs3")), ("tr", ("transition1", "transition2", "transition3")),
                 ("rw", ("reward_model1", "reward_model2", "reward_model3")))
ZA_NETS = (("off_za_src", "za_src"), ("off_za_trg", "za_trg"))


def pack_pretrain(params, S, A, device):
    """Reference state_dict tensors (`<layer>.weight [7,in,out]`, `.bias [7,1,out]`) -> the training blob."""
    L = _lib.pretrain_layout(S, A)
    g = lambda k: torch.as_tensor(params[k], dtype=torch.float32).to(device)
    blob = torch.zeros(L.total_floats, dtype=torch.float32, device=device)
    for nm, (l1, l2, l3) in PRETRAIN_NETS:
        ml = getattr(L, nm)
        members = []
        for e in range(7):                              # EnsembleLinear stores [in, out]; pack_mlp wants nn.Linear's [out, in]
            members.append({"network.0.weight": g(l1 + ".weight")[e].t(), "network.0.bias": g(l1 + ".bias")[e, 0],
                            "network.2.weight": g(l2 + ".weight")[e].t(), "network.2.bias": g(l2 + ".bias")[e, 0],
                            "network.4.weight": g(l3 + ".weight")[e].t(), "network.4.bias": g(l3 + ".bias")[e, 0]})
        off = getattr(L, "off_" + nm)
        blob[off:off + ml.total_floats] = pack_mlp(members, ml.in_dim, ml.out_dim, device)
    for off_name, pre in ZA_NETS:
        off = getattr(L, off_name)
        W1, b1, W2, b2 = g(pre + "1.weight"), g(pre + "1.bias"), g(pre + "2.weight"), g(pre + "2.bias")
        z = torch.zeros(7, L.za_member_floats, dtype=torch.float32, device=device)
        z[:, L.za_w1:L.za_w1 + L.za_in * 32] = W1.reshape(7, -1)
        z[:, L.za_b1:L.za_b1 + 32] = b1[:, 0]
        z[:, L.za_w2:L.za_w2 + 512] = W2[:, :, :16].reshape(7, -1)          # mu half only
        z[:, L.za_b2:L.za_b2 + 16] = b2[:, 0, :16]
        blob[off:off + z.numel()] = z.reshape(-1)
    return blob


def unpack_pretrain(blob, S, A, into=None):
    """Inverse of pack_pretrain.  Returns {name: tensor} in the reference layout; `into` (a state-dict-like mapping of
    full-size tensors) supplies the halves the blob does not hold (logvar half of za_*2) and is updated in place."""
    L = _lib.pretrain_layout(S, A)
    out = {}
    for nm, names in PRETRAIN_NETS:
        ml = getattr(L, nm)
        off = getattr(L, "off_" + nm)
        ms = unpack_mlp(blob[off:off + ml.total_floats], ml.in_dim, ml.out_dim, 7)
        for li, lname in zip((0, 2, 4), names):
            out[lname + ".weight"] = torch.stack([m[f"network.{li}.weight"].t() for m in ms]).contiguous()
            out[lname + ".bias"] = torch.stack([m[f"network.{li}.bias"] for m in ms]).unsqueeze(1).contiguous()
    for off_name, pre in ZA_NETS:
        off = getattr(L, off_name)
        z = blob[off:off + 7 * L.za_member_floats].view(7, L.za_member_floats)
        out[pre + "1.weight"] = z[:, L.za_w1:L.za_w1 + L.za_in * 32].reshape(7, L.za_in, 32).clone()
        out[pre + "1.bias"] = z[:, L.za_b1:L.za_b1 + 32].reshape(7, 1, 32).clone()
        W2mu = z[:, L.za_w2:L.za_w2 + 512].reshape(7, 32, 16)
        b2mu = z[:, L.za_b2:L.za_b2 + 16].reshape(7, 1, 16)
        if into is not None:
            W2, b2 = into[pre + "2.weight"].clone(), into[pre + "2.bias"].clone()
            W2[:, :, :16] = W2mu; b2[:, :, :16] = b2mu
            out[pre + "2.weight"], out[pre + "2.bias"] = W2, b2
        else:
            out[pre + "2.weight.mu"], out[pre + "2.bias.mu"] = W2mu.clone(), b2mu.clone()
    if into is not None:
        for k, v in out.items():
            into[k] = v
    return out


# ---- MOPO ablation pre-training blob (MobodyPretrainMopoLayout) ----------------------------------------------------
PRETRAIN_MOPO_NETS = (("dyn", ("za_src1", "za_src2", "za_src3")), ("rw", ("reward_model1", "reward_model2", "reward_model3")))


def _ens_members(g, names):
    """EnsembleLinear `[7, in, out]` / `[7, 1, out]` tensors of a 3-layer net -> pack_mlp's per-member nn.Linear dicts."""
    l1, l2, l3 = names
    return [{"network.0.weight": g(l1 + ".weight")[e].t(), "network.0.bias": g(l1 + ".bias")[e, 0],
             "network.2.weight": g(l2 + ".weight")[e].t(), "network.2.bias": g(l2 + ".bias")[e, 0],
             "network.4.weight": g(l3 + ".weight")[e].t(), "network.4.bias": g(l3 + ".bias")[e, 0]} for e in range(7)]


def pack_pretrain_mopo(params, S, A, device):
    """Reference state_dict tensors of a mopo model (za_src1-3, reward_model1-3) -> the mopo training blob."""
    L = _lib.pretrain_mopo_layout(S, A)
    g = lambda k: torch.as_tensor(params[k], dtype=torch.float32).to(device)
    blob = torch.zeros(L.total_floats, dtype=torch.float32, device=device)
    for nm, names in PRETRAIN_MOPO_NETS:
        ml, off = getattr(L, nm), getattr(L, "off_" + nm)
        blob[off:off + ml.total_floats] = pack_mlp(_ens_members(g, names), ml.in_dim, ml.out_dim, device)
    return blob


def unpack_pretrain_mopo(blob, S, A, into=None):
    """Inverse of pack_pretrain_mopo: {name: tensor} in the reference layout; `into` (a state-dict-like mapping) is updated
    in place when given."""
    L = _lib.pretrain_mopo_layout(S, A)
    out = {}
    for nm, names in PRETRAIN_MOPO_NETS:
        ml, off = getattr(L, nm), getattr(L, "off_" + nm)
        ms = unpack_mlp(blob[off:off + ml.total_floats], ml.in_dim, ml.out_dim, 7)
        for li, lname in zip((0, 2, 4), names):
            out[lname + ".weight"] = torch.stack([m[f"network.{li}.weight"].t() for m in ms]).contiguous()
            out[lname + ".bias"] = torch.stack([m[f"network.{li}.bias"] for m in ms]).unsqueeze(1).contiguous()
    if into is not None:
        for k, v in out.items():
            into[k] = v
    return out


# ---- wide MLPs (csrc/wide.hip, MobodyWideLayout): BOSA's VAE nets --------------------------------------------------------
def pack_wide(W1, b1, W2, b2, W3, b3, device):
    """W_i [E, in, out], b_i [E, out] (EnsembleFC's orientation; an nn.Linear weight goes in as weight.t()[None]) -> the flat
    zero-padded blob of mobody_wide_layout(in, hidden, out, E)."""
    g = lambda t: torch.as_tensor(t, dtype=torch.float32).to(device)
    W1, b1, W2, b2, W3, b3 = (g(t) for t in (W1, b1, W2, b2, W3, b3))
    E, in_dim, hidden = W1.shape
    out_dim = W3.shape[2]
    assert W2.shape == (E, hidden, hidden) and W3.shape == (E, hidden, out_dim), (tuple(W2.shape), tuple(W3.shape))
    assert b1.shape == (E, hidden) and b2.shape == (E, hidden) and b3.shape == (E, out_dim)
    L = _lib.wide_layout(in_dim, hidden, out_dim, E)
    blob = torch.zeros(E, L.member_floats, dtype=torch.float32, device=device)
    for off, t, K, N in ((L.w1, W1, L.Kp1, L.Hp), (L.w2, W2, L.Hp, L.Hp), (L.w3, W3, L.Hp, L.Np3)):
        blob[:, off:off + K * N].view(E, K, N)[:, :t.shape[1], :t.shape[2]] = t
    for off, t in ((L.b1, b1), (L.b2, b2), (L.b3, b3)):
        blob[:, off:off + t.shape[1]] = t
    return blob.reshape(-1)


def unpack_wide(blob, in_dim, hidden, out_dim, members):
    """Inverse of pack_wide: (W1, b1, W2, b2, W3, b3) as clones, W_i [E, in, out], b_i [E, out].  Works on any tensor in blob
    layout (a gradient, an Adam moment)."""
    L = _lib.wide_layout(in_dim, hidden, out_dim, members)
    blob = blob.reshape(members, L.member_floats)
    W = lambda off, K, N, k, n: blob[:, off:off + K * N].view(members, K, N)[:, :k, :n].clone()
    b = lambda off, n: blob[:, off:off + n].clone()
    return (W(L.w1, L.Kp1, L.Hp, in_dim, hidden), b(L.b1, hidden), W(L.w2, L.Hp, L.Hp, hidden, hidden), b(L.b2, hidden),
            W(L.w3, L.Hp, L.Np3, hidden, out_dim), b(L.b3, out_dim))


def wide_padding_mask(in_dim, hidden, out_dim, members, device="cpu"):
    """Bool tensor in blob layout: True on the padding entries (the ones no reference parameter maps to)."""
    ones = lambda *s: torch.ones(*s)
    used = pack_wide(ones(members, in_dim, hidden), ones(members, hidden), ones(members, hidden, hidden), ones(members, hidden),
                     ones(members, hidden, out_dim), ones(members, out_dim), device)
    return used == 0


# BOSA's VAEs (bosa.py:23-133, :203-327) are two wide nets each: the encoder with the `mean` and `log_std` heads packed as ONE
# output layer (columns [0, L) mean, [L, 2L) log_std), and the decoder.
def pack_bosa_vae_policy(sd, device):
    """VAE_Policy.state_dict() -> (encoder blob, decoder blob)."""
    g = lambda k: torch.as_tensor(sd[k], dtype=torch.float32)
    lin = lambda p: (g(p + ".weight").t()[None], g(p + ".bias")[None])
    (W1, b1), (W2, b2) = lin("encoder_shared.0"), lin("encoder_shared.2")
    (Wm, bm), (Ws, bs) = lin("mean"), lin("log_std")
    enc = pack_wide(W1, b1, W2, b2, torch.cat([Wm, Ws], 2), torch.cat([bm, bs], 1), device)
    (D1, d1), (D2, d2), (D3, d3) = lin("decoder.0"), lin("decoder.2"), lin("decoder.4")
    return enc, pack_wide(D1, d1, D2, d2, D3, d3, device)


def unpack_bosa_vae_policy(enc, dec, S, A, hidden, latent=None):
    """Inverse of pack_bosa_vae_policy (any tensors in blob layout): a dict with VAE_Policy's keys, nn.Linear orientation."""
    Lz = 2 * A if latent is None else latent
    W1, b1, W2, b2, W3, b3 = unpack_wide(enc, S + A, hidden, 2 * Lz, 1)
    D1, d1, D2, d2, D3, d3 = unpack_wide(dec, S + Lz, hidden, A, 1)
    out = {}
    for p, W, b in (("encoder_shared.0", W1, b1), ("encoder_shared.2", W2, b2), ("mean", W3[:, :, :Lz], b3[:, :Lz]),
                    ("log_std", W3[:, :, Lz:], b3[:, Lz:]), ("decoder.0", D1, d1), ("decoder.2", D2, d2), ("decoder.4", D3, d3)):
        out[p + ".weight"] = W[0].t().contiguous()
        out[p + ".bias"] = b[0].contiguous()
    return out


def pack_bosa_vae_dynamics(sd, device):
    """VAE_Dynamics_Ensemble.state_dict() (`<layer>.W [E, in, out]`, `<layer>.b [E, 1, out]`) -> (encoder blob, decoder blob)."""
    g = lambda k: torch.as_tensor(sd[k], dtype=torch.float32)
    fc = lambda p: (g(p + ".W"), g(p + ".b")[:, 0])
    (W1, b1), (W2, b2) = fc("encoder_shared.0"), fc("encoder_shared.2")
    (Wm, bm), (Ws, bs) = fc("mean"), fc("log_std")
    enc = pack_wide(W1, b1, W2, b2, torch.cat([Wm, Ws], 2), torch.cat([bm, bs], 1), device)
    (D1, d1), (D2, d2), (D3, d3) = fc("decoder.0"), fc("decoder.2"), fc("decoder.4")
    return enc, pack_wide(D1, d1, D2, d2, D3, d3, device)


def unpack_bosa_vae_dynamics(enc, dec, S, A, hidden, members, latent=None):
    """Inverse of pack_bosa_vae_dynamics: a dict with VAE_Dynamics_Ensemble's keys and shapes."""
    Lz = 2 * S if latent is None else latent
    W1, b1, W2, b2, W3, b3 = unpack_wide(enc, 2 * S + A, hidden, 2 * Lz, members)
    D1, d1, D2, d2, D3, d3 = unpack_wide(dec, S + A + Lz, hidden, S, members)
    out = {}
    for p, W, b in (("encoder_shared.0", W1, b1), ("encoder_shared.2", W2, b2), ("mean", W3[:, :, :Lz], b3[:, :Lz]),
                    ("log_std", W3[:, :, Lz:], b3[:, Lz:]), ("decoder.0", D1, d1), ("decoder.2", D2, d2), ("decoder.4", D3, d3)):
        out[p + ".W"] = W.contiguous()
        out[p + ".b"] = b[:, None, :].contiguous()
    return out
