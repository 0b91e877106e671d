"""The (S, A) edges of the dynamics layout (mobody_dyn_layout: S in [2, 127], A in [1, 64], 2S + A <= 256) and the fp64 /
fp32 restatements tests/test_hip_dyn_shapes.py holds the kernels to.  Pure CPU: nothing here touches the GPU or the library.

Where the code dispatches on shape:
  Np  = round_up(S, 16)        transition head: NT3 = 1 / 2 / 3 / 7 for Np = 16 / 32 / 48 / 112, every other width the generic
                               narrow_layer branch of k_dyn_fwd (and of the fused MLP forwards / backward for a head that wide)
  Kp  = round_up(2S + A, 8)    reward-head input, at most 256
  Kza = round_up(16 + A, 8)    action-encoder input, 24 .. 80
  rpb = min(256 // S, 64)      whole rows per workgroup of k_dyn_sample
Every reference is computed once per (shape, size) and shared (functools.lru_cache); callers must not write into them."""
import functools

import numpy as np
import torch

import golden_util as gu
from oracle import mobody_oracle as O
from test_pretrain_mopo_fixture import TRAINED as MOPO_TRAINED, _mlp, mopo_step_grads
from test_uncertainty_fixture import penalty_f64

SHAPES = [
    (2, 1),      # smallest layout; rpb capped at 64; S - 1 = 1 dim under the penalty sum; Kza 24 with 7 pad columns
    (3, 64),     # rpb cap with 192 live threads; Kza = 80, the maximum
    (4, 8),      # rpb = 64 without the cap; 16 + A a multiple of 8
    (16, 16),    # Np = 16 with no padded head column; S a multiple of 8
    (32, 9),     # Np = 32 exact; Kza = 32
    (48, 1),     # Np = 48 exact (narrow_run_wide); A = 1
    (49, 33),    # first generic width, Np = 64 with 15 pad columns
    (60, 9),     # generic Np = 64, kitchen-sized
    (64, 64),    # generic, Np = 64 exact; 2S + A = 192
    (85, 2),     # generic Np = 96; rpb = 3, 255 live threads
    (86, 3),     # rpb = 2, 172 live threads
    (96, 64),    # generic Np = 96 exact; 2S + A = 256, Kp with no pad
    (97, 8),     # NT3 = 7 with 15 pad columns
    (112, 32),   # NT3 = 7 exact; 2S + A = 256
    (127, 2),    # largest reachable S; generic Np = 128; 2S + A = 256
    (127, 1),    # 2S + A = 255, one reward-head pad column
]
MOPO_SHAPES = [(2, 1), (49, 33), (64, 64), (127, 2)]
PAD_SHAPES = [(2, 1), (49, 33), (97, 8), (127, 1)]
RNG_SHAPES = [(2, 1), (85, 2), (127, 2)]
PRETRAIN_CASES = [(S, A, 9) for S, A in SHAPES] + [(60, 9, 33), (127, 2, 33)]
MOPO_PRETRAIN_CASES = [(S, A, 9) for S, A in MOPO_SHAPES] + [(127, 2, 33)]
ALL_MODES = ("pairwise-diff", "aleatoric", "ensemble_std")
COEF = 0.25


def np_head(S):
    return (S + 15) // 16 * 16


def is_generic(S):
    return np_head(S) not in (16, 32, 48, 112)


# validate(): the generic-head entries, the 2S + A = 256 entries, the smallest layout
VALIDATE_SHAPES = [(S, A) for S, A in SHAPES if is_generic(S) or 2 * S + A == 256 or (S, A) == (2, 1)]
ANT_SHAPE = (112, 32)


def tasks_for(S, A):
    """(name the oracle resolves, termination id) pairs the step test runs on this shape."""
    out = [("halfcheetah", 1), ("walker2d", 4)]
    if (S, A) == ANT_SHAPE:
        out.append(("ant", 3))
    if S > 26:
        out.append(("pen", 6))
    return out


def ident(shape):
    return "S%d_A%d" % shape[:2] + ("_b%d" % shape[2] if len(shape) > 2 else "")


# ------------------------------------------------------------------------------------------------- parameters and inputs
@functools.lru_cache(maxsize=None)
def params(S, A, mopo=False):
    """gen_inputs' weights; the first state dim lifted into walker2d's alive band so the predicates see both outcomes."""
    p = gu.gi.dyn_params(1000 + 7 * S + A, S, A, mopo=mopo)
    p[("za_src3" if mopo else "transition3") + ".bias"][:, 0, 0] += np.float32(-0.35 if mopo else 0.85)
    return p


def mopo_inference_params(p, A):
    """A mopo model's parameters with the latent action-encoder slots of the inference layout as zeros (what
    MOBODYModule.packed() packs: the reward head is all the inference blob of a mopo model is read for)."""
    q = {k: v for k, v in p.items() if not k.startswith("za_")}
    for pre in ("za_src", "za_trg"):
        for name, (i, o) in ((pre + "1", (16 + A, 32)), (pre + "2", (32, 32))):
            q[name + ".weight"] = np.zeros((7, i, o), np.float32)
            q[name + ".bias"] = np.zeros((7, 1, o), np.float32)
    return q


@functools.lru_cache(maxsize=None)
def step_inputs(S, A, B):
    rng = np.random.default_rng(100000 + 1000 * S + 10 * A + B)
    obs = gu.gi.walker_like_obs(rng, B, S)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    eps = rng.standard_normal((7, B, S)).astype(np.float32)
    idx = rng.integers(0, 5, B)
    return obs, act, eps, idx


# ------------------------------------------------------------------------------------------------- forward
def _means(p, obs, act, use_trg, dtype):
    with torch.no_grad():
        if O.is_mopo(p):
            P = {k: torch.tensor(p[k], dtype=dtype) for k in MOPO_TRAINED}
            x = lambda v: torch.tensor(v, dtype=dtype).unsqueeze(0).repeat(7, 1, 1)
            return (x(obs) + _mlp(P, "za_src", torch.cat([x(obs), x(act)], -1))).numpy()
        return O.dyn_forward(O.to_torch(p, dtype), O.T(obs, dtype), O.T(act, dtype), use_trg, dtype=dtype)[0].numpy()


@functools.lru_cache(maxsize=None)
def forward_ref(S, A, B, use_trg, mopo=False):
    """(fp64 means [7, B, S], the fp32 torch restatement's means) on step_inputs(S, A, B)."""
    obs, act, _, _ = step_inputs(S, A, B)
    p = params(S, A, mopo)
    return _means(p, obs, act, use_trg, torch.float64), _means(p, obs, act, use_trg, torch.float32)


def forward_bound(f64, t32, mode):
    """Largest |hip - f64| allowed over the case: exact fp32 is held to the measured form of test_mopo_grads_vs_fp64_restatement
    (3 x the fp32 restatement's own error + 1e-6 of the output scale), the split modes to tests/test_hip_precision.py's TOL."""
    scale = float(np.abs(f64).max())
    if mode == "f32":
        return 3.0 * float(np.abs(t32.astype(np.float64) - f64).max()) + 1e-6 * scale
    return 1e-5 * scale


# ------------------------------------------------------------------------------------------------- step, on given means
def step_ref(p, obs, act, mean, eps, idx, next_obs, mode, dtype=np.float64):
    """std / sample / penalty from the means `mean` [7, B, S] and the reward head on [s, a, next_obs] (shared by the members,
    mobody_dynamics.py:235), in `dtype`.  next_obs: the rows the reward head is fed (the kernel's own sample)."""
    B = mean.shape[1]
    m = np.asarray(mean, dtype)
    std = m.std(axis=0, ddof=1, dtype=dtype)
    nxt = m[idx, np.arange(B)] + np.asarray(eps, dtype)[idx, np.arange(B)] * std
    if dtype == np.float64:
        pen = penalty_f64(mode, m)
    else:                                                   # the same formulas carried in fp32
        var = m.var(axis=0, ddof=1, dtype=dtype)
        d = m[..., :-1] - m[..., :-1].mean(axis=0, dtype=dtype)
        pen = {"aleatoric": np.sqrt(var.sum(axis=1, dtype=dtype)), "ensemble_std": np.sqrt(var[:, :-1].mean(axis=1, dtype=dtype)),
               "pairwise-diff": np.sqrt((d * d).sum(axis=2, dtype=dtype)).max(axis=0)}[mode][:, None]
    td = torch.float64 if dtype == np.float64 else torch.float32
    with torch.no_grad():
        P = {k: torch.tensor(p[k], dtype=td) for k in p if k.startswith("reward_model")}
        raw = O.dyn_reward(P, O.T(obs, td), O.T(act, td), O.T(next_obs, td))[0].mean(0).numpy()
    return dict(next_obs=nxt, penalty=pen, raw_reward=raw)


def ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is np.testing.assert_allclose's pass."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


# ------------------------------------------------------------------------------------------------- validate()
@functools.lru_cache(maxsize=None)
def validate_inputs(S, A, B):
    s, a, s2, r, _ = gu.gi.batch(2000 + S + A + B, B, S, A)
    return s, a, s2, r


@functools.lru_cache(maxsize=None)
def validate_ref(S, A, B, use_trg, mopo=False):
    """fp64 per-member transition MSE [7] and reward MSE [7] (mobody_dynamics.py:1113-1140): the reward head on [s, a, mean_e]."""
    s, a, s2, r = validate_inputs(S, A, B)
    p = params(S, A, mopo)
    mean = torch.from_numpy(_means(p, s, a, use_trg, torch.float64))
    x = lambda v: torch.tensor(v, dtype=torch.float64).unsqueeze(0).repeat(7, 1, 1)
    with torch.no_grad():
        P = {k: torch.tensor(p[k], dtype=torch.float64) for k in p if k.startswith("reward_model")}
        rr = O.dyn_reward(P, x(s), x(a), mean)[0]
        return ((mean - x(s2)) ** 2).mean(dim=(1, 2)).numpy(), ((rr - x(r)) ** 2).mean(dim=(1, 2)).numpy()


# ------------------------------------------------------------------------------------------------- pre-training
def noise7(rng, b, S):
    return [rng.standard_normal((7, b, 16)).astype(np.float32) for _ in range(6)] + [rng.standard_normal((7, b, S)).astype(np.float32)]


@functools.lru_cache(maxsize=None)
def pretrain_inputs(S, A, b):
    rows = gu.gi.pretrain_batch(3000 + S + A + b, b, S, A)
    return rows, noise7(np.random.default_rng(S + A + b), b, S)


@functools.lru_cache(maxsize=None)
def pretrain_ref(S, A, b, use_trg):
    """(fp64, fp32) results of O.dyn_learn_step(apply=False) at params(S, A): dict(losses, grads {name: ndarray or None})."""
    rows, nz = pretrain_inputs(S, A, b)
    out = []
    for dtype in (torch.float64, torch.float32):
        w = O.dyn_learn_step(O.DynTrainState(params(S, A)), *rows, nz, use_trg, apply=False, dtype=dtype)
        out.append(dict(losses=np.array(w["losses"]), grads={k: None if v is None else v.numpy() for k, v in w["grads"].items()}))
    return tuple(out)


SUBNET = dict(zs="enc", tr="tr", re="rw", za="za")


def pretrain_grad_ratios(got, want):
    """Worst |got - want| / (1e-5 |want| + 1e-5 max|g| of the tensor's sub-network) over the tensors with a gradient (the rule
    of test_pretrain_grads_vs_oracle_shapes), as {tensor name: ratio}.  got: {name: ndarray}."""
    scale = {}
    for k, v in want.items():
        if v is not None:
            scale[SUBNET[k[:2]]] = max(scale.get(SUBNET[k[:2]], 0.0), float(np.abs(v).max()))
    return {k: ratio(got[k], v, 1e-5, 1e-5 * scale[SUBNET[k[:2]]]) for k, v in want.items() if v is not None}


@functools.lru_cache(maxsize=None)
def mopo_pretrain_inputs(S, A, b):
    rows = gu.gi.pretrain_batch(4000 + S + A + b, b, S, A)
    return rows, np.random.default_rng(S + A + b).standard_normal((7, b, S)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mopo_pretrain_ref(S, A, b, use_trg):
    """((losses, grads) in fp64, the same in fp32) of the torch restatement of one mopo learn() step at params(S, A, True)."""
    rows, eps = mopo_pretrain_inputs(S, A, b)
    return tuple(mopo_step_grads(params(S, A, True), rows, eps, use_trg, dtype=d) for d in (torch.float64, torch.float32))


# ------------------------------------------------------------------------------------------------- padding masks
def ones_like_params(p):
    return {k: np.ones_like(v) for k, v in p.items()}
