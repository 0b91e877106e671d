"""Thin torch-tensor front end of the C ABI (allocation + pointer plumbing only).

Every function here enqueues HIP kernels from libmobody_hip.so on torch's current stream;
none of them computes anything in PyTorch.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import check, cur_stream, load, ptr
from ._lib import BLOCK_BYTES as _BYTES


def _f32(t, device=None):
    t = torch.as_tensor(t, dtype=torch.float32)
    if device is not None:
        t = t.to(device)
    return t.contiguous()


def rng_normal(seed, stream_id, call, n, device):
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(load().mobody_rng_normal(seed, stream_id, call, n, ptr(out), cur_stream()), "mobody_rng_normal")
    return out


def rng_index(seed, stream_id, call, n, bound, device):
    out = torch.empty(n, dtype=torch.int32, device=device)
    check(load().mobody_rng_index(seed, stream_id, call, n, bound, ptr(out), cur_stream()), "mobody_rng_index")
    return out


def prec_id(mfma):
    """'f32' | 'bf16' | 'bf16x2' | 'bf16x3' | 'f16x2' (or the integer id) -> MobodyHyper.precision."""
    return mfma if isinstance(mfma, int) else _lib.PRECISIONS[mfma]


def unc_id(mode):
    """'pairwise-diff' | 'aleatoric' | 'ensemble_std' (or the integer id) -> MOBODY_UNC_* (mobody_dynamics.py:241-252)."""
    if isinstance(mode, int):
        return mode
    if mode not in _lib.UNCERTAINTY_MODES:
        raise ValueError(f"uncertainty_mode {mode!r}: expected one of {sorted(_lib.UNCERTAINTY_MODES)}")
    return _lib.UNCERTAINTY_MODES[mode]


def default_mfma():
    """MFMA mode when a config does not name one: exact fp32, unless MOBODY_MFMA says otherwise (how the whole parity
    suite is re-run in a split-precision mode: `MOBODY_MFMA=bf16x3 pytest -m gpu`)."""
    import os
    return os.environ.get("MOBODY_MFMA", "f32")


F16_W_LIMIT = 65504.0 / 2 ** 8      # 'f16x2' weight planes hold w * 2^8 (csrc/tile_bf.h F16_WSHIFT): |w| at or above this is Inf


def _check_f16_weights(blocks, what):
    """Refuse to build 'f16x2' planes of 256 x 256 weights that fp16 cannot hold after the 2^8 pre-scale (they would silently
    poison every output of the layer).  Runs where planes are (re)built -- set-up, checkpoint load, change of mode -- not per
    step; skipped inside a stream capture, where the host cannot read the device (the capture's builder was checked eagerly)."""
    if torch.cuda.is_current_stream_capturing():
        return
    m = max(float(b.abs().max()) for b in blocks)
    if m >= F16_W_LIMIT:
        raise ValueError(f"{what}: a 256 x 256 weight of magnitude {m:g} does not fit the f16x2 planes "
                         f"(|w| < 65504 / 2^8 = {F16_W_LIMIT}); use precision 'f32' or 'bf16x3'")


# ------------------------------------------------------------------------------------------------
# device health words (include/mobody_hip.h): f16x2 range faults and non-finite optimizer results
# ------------------------------------------------------------------------------------------------
F16_GUARDS = ("raise", "fallback", "off")
_health_blocks = {}                 # device index -> the int32[HEALTH_WORDS] block bound there


def check_f16_guard(value, distributed=False):
    """Validate config['f16_guard'] ('raise' | 'fallback' | 'off'); needs no GPU.  'fallback' re-builds one replica's planes in
    another mode, which data-parallel replicas cannot do independently: refused under a process group."""
    if value not in F16_GUARDS:
        raise ValueError(f"f16_guard {value!r}: expected one of {F16_GUARDS}")
    if value == "fallback" and distributed:
        raise ValueError("f16_guard='fallback' is not supported under a process group (replicas raise together under 'raise')")
    return value


def health_bind(words):
    """Bind an int32[>= HEALTH_WORDS] device tensor as the current device's health words (None unbinds).  Launches enqueued
    -- or captured -- afterwards report into it and freeze their optimizer steps once a bit is set."""
    if words is not None:
        assert words.dtype == torch.int32 and words.is_cuda and words.is_contiguous() and words.numel() >= _lib.HEALTH_WORDS
        with torch.cuda.device(words.device):
            check(load().mobody_health_bind(ptr(words)), "mobody_health_bind")
        _health_blocks[words.device.index] = words
    else:
        check(load().mobody_health_bind(None), "mobody_health_bind")
        _health_blocks.pop(torch.cuda.current_device(), None)


def health_block(device):
    """The block bound on `device`, allocated (zeroed) and bound on first use: one per device, shared by every object there."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _health_blocks:
        health_bind(torch.zeros(_lib.HEALTH_WORDS, dtype=torch.int32, device=torch.device("cuda", idx)))
    return _health_blocks[idx]


def health_bound(device=None):
    """The block bound on `device` (default: the current one) through this module, or None."""
    idx = torch.cuda.current_device() if device is None or torch.device(device).index is None else torch.device(device).index
    return _health_blocks.get(idx)


def health_clear():
    """Zero the bound block on the current stream (updates apply again)."""
    check(load().mobody_health_clear(cur_stream()), "mobody_health_clear")


def health_read(words=None):
    """(mask, step) of the bound block -- the fault bits and the Adam step count of the first faulting optimizer launch (0:
    none recorded).  The only health call that synchronises."""
    w = words if words is not None else _health_blocks.get(torch.cuda.current_device())
    if w is None:
        return 0, 0
    h = w[:2].tolist()
    return int(h[0]), int(h[1])


def health_bits(mask):
    return [n for n, b in (("F16_RANGE", _lib.HEALTH_F16_RANGE), ("NONFINITE", _lib.HEALTH_NONFINITE)) if mask & b]


def _mlp_w2(blob, L, members):
    return blob[:members * L.member_floats].view(members, L.member_floats)[:, L.w2:L.w2 + 65536]


def dyn_planes(blob, S, A, out=None, precision=3):
    """16-bit planes of zs2 / transition2 / reward_model2 in the format of the split-precision mode `precision`
    (modes 1-3 share the three bf16 planes; 'f16x2' has its own two fp16 planes)."""
    if prec_id(precision) == 4:
        L = _lib.dyn_layout(S, A)
        lays = [L.layer[_lib.DL_NAMES.index(n)] for n in ("zs2", "transition2", "reward_model2")]
        _check_f16_weights([blob[y.w_off:y.w_off + L.E * y.Kp * y.Np] for y in lays], "dyn_planes")
    pl = out if out is not None else torch.empty(load().mobody_dyn_planes_floats(), dtype=torch.float32, device=blob.device)
    check(load().mobody_dyn_planes(ptr(blob), S, A, ptr(pl), prec_id(precision), cur_stream()), "mobody_dyn_planes")
    return pl


def dyn_forward(blob, S, A, obs, act, use_trg=True, planes=None, precision=0):
    obs, act = _f32(obs), _f32(act)
    B = obs.shape[0]
    mean = torch.empty(7, B, S, dtype=torch.float32, device=obs.device)
    check(load().mobody_dyn_forward(ptr(blob), ptr(planes), prec_id(precision), S, A, ptr(obs), ptr(act), B, int(use_trg),
                                    ptr(mean), cur_stream()), "mobody_dyn_forward")
    return mean


def dyn_step(blob, S, A, task_id, obs, act, noise=None, elite_idx=None, alive=None, elites=(0, 1, 2, 3, 4), seed=0,
             call=0, penalty_coef=0.0, use_penalty=True, use_trg=True, want_mean=False, workspace=None, out=None,
             planes=None, precision=0, mopo=None, call_dev=None, uncertainty_mode=0):
    """Returns dict(next_obs[B,S], reward[B,1], terminal uint8[B,1], penalty[B,1], raw_reward[B,1], mean?).
    mopo = (blob, blob_T) of the 7-member MLP za_src1..3: the MOPO ablation's step.
    call_dev: device int64[1] added to `call` (graph replay).  uncertainty_mode: name or MOBODY_UNC_* id (mobody_ens_step)."""
    obs, act = _f32(obs), _f32(act)
    dev, B = obs.device, obs.shape[0]
    if noise is not None:
        noise = _f32(noise, dev)
        assert noise.shape == (7, B, S)
    if elite_idx is not None:
        elite_idx = torch.as_tensor(elite_idx).to(device=dev, dtype=torch.int32).contiguous()
    workspace = _workspace("mobody_dyn_step_workspace", dev, S, A, B, ws=workspace)
    o = out or {}
    nxt = o.get("next_obs", None)
    if nxt is None:
        nxt = torch.empty(B, S, dtype=torch.float32, device=dev)
    rew = o["reward"] if "reward" in o else torch.empty(B, 1, dtype=torch.float32, device=dev)
    term = o["terminal"] if "terminal" in o else torch.empty(B, 1, dtype=torch.uint8, device=dev)
    pen = o["penalty"] if "penalty" in o else torch.empty(B, 1, dtype=torch.float32, device=dev)
    raw = o["raw_reward"] if "raw_reward" in o else torch.empty(B, 1, dtype=torch.float32, device=dev)
    mean = torch.empty(7, B, S, dtype=torch.float32, device=dev) if want_mean else None
    model = _model_fields(blob, planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg)
    a = _lib.MobodyEnsStep(struct_bytes=_BYTES[_lib.MobodyEnsStep], obs=ptr(obs), act=ptr(act), B=B, noise=ptr(noise),
                           elite_idx=ptr(elite_idx), alive=ptr(alive), call=call, use_penalty=int(bool(use_penalty)),
                           penalty_coef=float(penalty_coef), next_obs=ptr(nxt), reward=ptr(rew), terminal=ptr(term),
                           penalty=ptr(pen), raw_reward=ptr(raw), mean_out=ptr(mean), workspace=ptr(workspace), **model)
    check(load().mobody_ens_step(C.byref(a), cur_stream()), "mobody_ens_step")
    res = dict(next_obs=nxt, reward=rew, terminal=term, penalty=pen, raw_reward=raw)
    if want_mean:
        res["mean"] = mean
    return res


def mlp3_forward(blob, in_dim, out_dim, members, src0, src1=None, out_mode=0, max_action=1.0, save=False, blob_T=None,
                 precision=0):
    """out[members, rows, out_dim] (+ saved (x, h1, h2) when save=True)."""
    src0 = _f32(src0)
    rows, n0 = src0.shape
    n1 = 0
    if src1 is not None:
        src1 = _f32(src1)
        n1 = src1.shape[1]
    dev = src0.device
    out = torch.empty(members, rows, out_dim, dtype=torch.float32, device=dev)
    sx = sh1 = sh2 = None
    if save:
        L = _lib.mlp_layout(in_dim, out_dim, members)
        sx = torch.empty(rows, L.Kp1, dtype=torch.float32, device=dev)
        sh1 = torch.empty(members, rows, 256, dtype=torch.float32, device=dev)
        sh2 = torch.empty(members, rows, 256, dtype=torch.float32, device=dev)
    check(load().mobody_mlp3_forward(ptr(blob), ptr(blob_T), prec_id(precision), in_dim, out_dim, members, ptr(src0), n0, ptr(src1), n1, rows, out_mode,
                                     float(max_action), ptr(out), ptr(sx), ptr(sh1), ptr(sh2), cur_stream()),
          "mobody_mlp3_forward")
    return (out, sx, sh1, sh2) if save else out


# ------------------------------------------------------------------------------------------------
# training step
# ------------------------------------------------------------------------------------------------
def train_dims(S, A, N, Nt, N_global=None, Nt_global=None):
    return _lib.MobodyTrainDims(S, A, N, Nt, N if N_global is None else N_global, Nt if Nt_global is None else Nt_global)


def hyper(cfg):
    return _lib.MobodyHyper(float(cfg["gamma"]), float(cfg["tau"]), float(cfg["max_action"]), float(cfg["weight"]),
                            float(cfg["bc_coef"]), int(bool(cfg["q_weighted"])), int(bool(cfg["scale_Q"])),
                            prec_id(cfg.get("mfma", default_mfma())))


def _workspace(name, device, *args, ws=None):
    """The scratch tensor of the size the library's entry `name` reports for `args`: `ws` when that is large enough."""
    n = getattr(load(), name)(*args)
    if n < 0:
        raise _lib.MobodyError(name + ": " + load().mobody_last_error().decode())
    return ws if ws is not None and ws.numel() >= n else torch.empty(n, dtype=torch.float32, device=device)


def _model_fields(dyn_blob, dyn_planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg):
    """The fields the four MobodyEns* blocks share (the model a call runs), spread by the block's one constructor call.
    mopo = (blob, blob_T) of the MOPO ablation's MLP or None.  The dict owns the host array `elites` points to."""
    mb, mbt = mopo if mopo is not None else (None, None)
    return dict(uncertainty_mode=unc_id(uncertainty_mode), dyn_blob=ptr(dyn_blob), dyn_planes=ptr(dyn_planes), mopo_blob=ptr(mb),
                mopo_blob_T=ptr(mbt), precision=prec_id(precision), S=S, A=A, task=task_id,
                elites=(C.c_int32 * len(elites))(*[int(e) for e in elites]), n_elites=len(elites), seed=seed,
                call_dev=ptr(call_dev), use_trg=int(bool(use_trg)))


def _run_with_workspace(name, blk, ws, device):
    """Point `blk` at a workspace of the size `name`_workspace reports for it (`ws` when large enough) and call `name`."""
    ws = _workspace(name + "_workspace", device, C.byref(blk), ws=ws)
    blk.workspace = ptr(ws)
    check(getattr(load(), name)(C.byref(blk), cur_stream()), name)
    return ws


def train_workspace(dims, device):
    return _workspace("mobody_train_workspace", device, C.byref(dims))


def mlp_transpose(blob, in_dim, out_dim, members, out=None, precision=0):
    """T blob of a packed MLP; `precision` = the MFMA mode whose W2 plane format it carries."""
    L = _lib.mlp_layout(in_dim, out_dim, members)
    if prec_id(precision) == 4:
        _check_f16_weights([_mlp_w2(blob, L, members)], "mlp_transpose")
    bt = out if out is not None else torch.empty(L.t_total_floats, dtype=torch.float32, device=blob.device)
    assert bt.numel() == L.t_total_floats
    check(load().mobody_mlp_transpose(in_dim, out_dim, members, ptr(blob), ptr(bt), prec_id(precision), cur_stream()),
          "mobody_mlp_transpose")
    return bt


# Block fillers: one per argument block, shared by the wrappers of its gradient-only and fused forms.  The shared fields are set
# by keyword in ONE constructor call (everything else stays 0 / NULL); a wrapper then assigns the few fields of its own form.
# Forwarding those as **kwargs through helpers doubled the host cost of a call, and so did spelling out every NULL.
def _critic_block(dims, hyp, actor_blob, q_blob, q_blob_T, qtarg_blob, batch, loss_out, ws, q_next, policy_forward,
                  actor_blob_T, qtarg_blob_T):
    s, a, s2, r, nd = batch
    return _lib.MobodyCritic(struct_bytes=_BYTES[_lib.MobodyCritic], d=dims, h=hyp, actor_blob=ptr(actor_blob),
                             actor_blob_T=ptr(actor_blob_T), q_blob=ptr(q_blob), q_blob_T=ptr(q_blob_T),
                             qtarg_blob=ptr(qtarg_blob), qtarg_blob_T=ptr(qtarg_blob_T), state=ptr(s), action=ptr(a),
                             next_state=ptr(s2), reward=ptr(r), not_done=ptr(nd), q_next=ptr(q_next),
                             policy_forward=int(bool(policy_forward)), loss_out=ptr(loss_out), workspace=ptr(ws))


def _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws):
    return _lib.MobodyActor(struct_bytes=_BYTES[_lib.MobodyActor], d=dims, h=hyp, actor_blob=ptr(actor_blob),
                            actor_blob_T=ptr(actor_blob_T), q_blob=ptr(q_blob), q_blob_T=ptr(q_blob_T), state=ptr(state),
                            action=ptr(action), stats=ptr(stats), workspace=ptr(ws))


def critic_step(dims, hyp, actor_blob, q_blob, q_blob_T, qtarg_blob, batch, grad_q, loss_out, ws, q_next=None,
                policy_forward=False, actor_blob_T=None, qtarg_blob_T=None):
    blk = _critic_block(dims, hyp, actor_blob, q_blob, q_blob_T, qtarg_blob, batch, loss_out, ws, q_next, policy_forward,
                        actor_blob_T, qtarg_blob_T)
    blk.grad_q = ptr(grad_q)
    check(load().mobody_critic(C.byref(blk), cur_stream()), "mobody_critic")


def actor_forward(dims, hyp, actor_blob, q_blob, state, action, stats, ws, policy_ready=False, actor_blob_T=None, q_blob_T=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.policy_ready = int(bool(policy_ready))
    check(load().mobody_actor_forward(C.byref(blk), cur_stream()), "mobody_actor_forward")


def actor_backward(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, grad_actor, loss_out,
                   ws, v_true=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.v_true, blk.grad_actor, blk.loss_out = ptr(v_true), ptr(grad_actor), ptr(loss_out)
    check(load().mobody_actor_backward(C.byref(blk), cur_stream()), "mobody_actor_backward")


def critic_update(dims, hyp, actor_blob, q_blob, q_blob_T, qtarg_blob, batch, m, v, t, lr, loss_out, ws, q_next=None,
                  t_dev=None, policy_forward=False, actor_blob_T=None, qtarg_blob_T=None, bump=None, phase=0, gather=None):
    """critic_step + Adam + Polyak in the fused single-GPU form (t: host step count, or t_dev: device int64[1]);
    bump: device int64[1] word (not t_dev) the optimizer launch increments by one.  phase 1 / 2: only the forwards / only the
    backward + update (MobodyCritic.phase: the caller joins whatever rewrites `reward` in between).
    gather: the arguments of gather_batch_rng up to `sizes`, plus its `bump`, as a dict -- the step's first forward launch then
    draws and fetches the minibatch itself and WRITES `batch` (MobodyCritic.gather: packed rings, no q_next, phase 0)."""
    blk = _critic_block(dims, hyp, actor_blob, q_blob, q_blob_T, qtarg_blob, batch, loss_out, ws, q_next, policy_forward,
                        actor_blob_T, qtarg_blob_T)
    blk.m, blk.v, blk.t, blk.t_dev, blk.lr, blk.bump, blk.phase = ptr(m), ptr(v), int(t), ptr(t_dev), float(lr), ptr(bump), int(phase)
    if gather is not None:
        gr, keep = _gather_rng_args(**gather)           # `keep`: the host arrays `gr` points into, alive until the call returns
        blk.gather = C.pointer(gr)
    check(load().mobody_critic(C.byref(blk), cur_stream()), "mobody_critic")


def bosa_critic(dims, hyp, q_blob, q_blob_T, batch, q_next, row_weight, row_const, cons_coef, cons_rows, loss_out, ws, grad_q=None,
                m=None, v=None, t=0, t_dev=None, lr=0.0):
    """BOSA's critic update (seed mode 9) on caller-supplied bootstrap values q_next [N]: the loss mean_rows(w (q1 - y)^2) +
    mean_rows(w (q2 - y)^2) + cons_coef * (sum_{c != 0} (q1 + q2) / cons_rows) with the seed's per-row constant c = row_const.
    loss_out[0] = that loss, loss_out[1] = the conservative term.  grad_q: the gradient form; m, v: Adam fused, and no Polyak
    update (the target nets follow the delayed actor step)."""
    blk = _critic_block(dims, hyp, None, q_blob, q_blob_T, None, batch, loss_out, ws, q_next, False, None, None)
    blk.grad_q, blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(grad_q), ptr(m), ptr(v), int(t), ptr(t_dev), float(lr)
    check(load().mobody_bosa_critic(C.byref(blk), ptr(row_weight), ptr(row_const), float(cons_coef), int(cons_rows), cur_stream()),
          "mobody_bosa_critic")


def actor_update(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, m, v, t, lr, loss_out, ws,
                 v_true=None, t_dev=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.v_true, blk.loss_out = ptr(v_true), ptr(loss_out)
    blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(m), ptr(v), int(t), ptr(t_dev), float(lr)
    check(load().mobody_actor_backward(C.byref(blk), cur_stream()), "mobody_actor_backward")


# TD3_BC actor phase: the same block and workspace, its own two entry points (no v_true; every row is a BC row)
def td3bc_actor_forward(dims, hyp, actor_blob, q_blob, state, action, stats, ws, policy_ready=False, actor_blob_T=None, q_blob_T=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.policy_ready = int(bool(policy_ready))
    check(load().mobody_td3bc_actor_forward(C.byref(blk), cur_stream()), "mobody_td3bc_actor_forward")


def td3bc_actor_backward(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, grad_actor, loss_out, ws):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.grad_actor, blk.loss_out = ptr(grad_actor), ptr(loss_out)
    check(load().mobody_td3bc_actor_backward(C.byref(blk), cur_stream()), "mobody_td3bc_actor_backward")


def td3bc_actor_update(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, m, v, t, lr, loss_out, ws,
                       t_dev=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, action, stats, ws)
    blk.loss_out = ptr(loss_out)
    blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(m), ptr(v), int(t), ptr(t_dev), float(lr)
    check(load().mobody_td3bc_actor_backward(C.byref(blk), cur_stream()), "mobody_td3bc_actor_backward")


# BOSA actor phase (bosa.py:612-629): the same block and workspace; Q is member 0 alone and the estimator's term is an addend
def bosa_actor_forward(dims, hyp, actor_blob, q_blob, state, stats, pi_out, ws, actor_blob_T=None, q_blob_T=None):
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, None, stats, ws)
    check(load().mobody_bosa_actor_forward(C.byref(blk), ptr(pi_out), cur_stream()), "mobody_bosa_actor_forward")


def bosa_actor_backward(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, stats, dpi_extra, loss_out, ws, grad_actor=None,
                        m=None, v=None, t=0, t_dev=None, lr=0.0):
    """dpi_extra [N, A]: what the rest of the loss adds to d loss / d pi (BOSA: -(lamda / N) dll_da).  grad_actor: the gradient form;
    m, v: Adam fused.  loss_out[0] = -mean(q_0) / mean|q_0|, loss_out[1] = 0."""
    blk = _actor_block(dims, hyp, actor_blob, actor_blob_T, q_blob, q_blob_T, state, None, stats, ws)
    blk.grad_actor, blk.loss_out = ptr(grad_actor), ptr(loss_out)
    blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(m), ptr(v), int(t), ptr(t_dev), float(lr)
    check(load().mobody_bosa_actor_backward(C.byref(blk), ptr(dpi_extra), cur_stream()), "mobody_bosa_actor_backward")


# IQL (iql.py): one block type for the three calls of the step (MobodyIql); `nets` = (v_func, q_funcs, target_q_funcs, policy)
# as objects with .blob / .blob_T, `opt` the Adam state of the net the call trains (m, v given: fused form; grad: gradient form)
def iql_workspace(dims, device):
    return _workspace("mobody_iql_workspace", device, C.byref(dims))


def cosine_lr(lr0, k, T_max):
    """Learning rate of 1-based gradient step k under CosineAnnealingLR(T_max) (eta_min 0): the closed form in double, rounded to
    fp32 once -- the value mobody_iql_actor's fused form uses (csrc/train.h cosine_lr)."""
    import math
    import numpy as np
    lr0 = float(np.float32(lr0))
    return float(np.float32(lr0 * (1.0 + math.cos(math.pi * (k - 1) / T_max)) * 0.5))


def _iql_block(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws):
    vf, q, qt, pi = nets
    s, a, s2, r, nd = batch
    return _lib.MobodyIql(struct_bytes=_BYTES[_lib.MobodyIql], d=dims, h=hyp, lam=float(lam), temp=float(temp), T_max=int(T_max),
                          v_blob=ptr(vf.blob), v_blob_T=ptr(vf.blob_T), q_blob=ptr(q.blob), q_blob_T=ptr(q.blob_T),
                          qtarg_blob=ptr(qt.blob), qtarg_blob_T=ptr(qt.blob_T), pi_blob=ptr(pi.blob), pi_blob_T=ptr(pi.blob_T),
                          state=ptr(s), action=ptr(a), next_state=ptr(s2), reward=ptr(r), not_done=ptr(nd), adv=ptr(adv),
                          loss_out=ptr(loss_out), workspace=ptr(ws))


def _iql_call(name, blk, grad, m, v, t, t_dev, lr, bump=None, log_out=None, extra=()):
    """extra: the entry's own arguments between the block and the stream"""
    blk.grad, blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(grad), ptr(m), ptr(v), int(t), ptr(t_dev), float(lr)
    blk.bump, blk.log_out = ptr(bump), ptr(log_out)
    check(getattr(load(), name)(C.byref(blk), *extra, cur_stream()), name)


def iql_value(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws, grad=None, m=None, v=None, t=0, t_dev=None, lr=0.0,
              log_out=None):
    """V update (iql.py:174-185): writes adv[N] (before the update), loss_out[0] = L_V; log_out[2] = mean adv, mean V."""
    _iql_call("mobody_iql_value", _iql_block(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws), grad, m, v, t, t_dev, lr,
              log_out=log_out)


def iql_critic(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws, grad=None, m=None, v=None, t=0, t_dev=None, lr=0.0,
               bump=None):
    """Twin-Q update against y = r + nd gamma V(s') (iql.py:187-196), Adam + Polyak in the fused form."""
    _iql_call("mobody_iql_critic", _iql_block(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws), grad, m, v, t, t_dev, lr,
              bump=bump)


def iql_actor(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws, grad=None, m=None, v=None, t=0, t_dev=None, lr=0.0):
    """Policy update (iql.py:198-202) from adv; fused form: Adam at cosine_lr(lr, t or t_dev[0], T_max)."""
    _iql_call("mobody_iql_actor", _iql_block(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws), grad, m, v, t, t_dev, lr)


# DARA (dara.py): the classifier update and the relabel in front of IQL's three calls, one block type (MobodyDara).  `heads` =
# (sa_classifier, sas_classifier) as objects with .blob / .blob_T; `batch` = (state, action, next_state, reward, ...) of [src | tar]
def dara_workspace(dims, device):
    """Floats of the DARA step's scratch: iql_workspace's (the same tensor serves the IQL calls) + the classifier's."""
    return _workspace("mobody_dara_workspace", device, C.byref(dims))


def _pair_opt(blk, second, grads, opts, t, t_dev, lr, loss_out):
    """The gradient blobs or the Adam state of a block that trains two nets, `sa` and `second`, under one step count and rate."""
    for k, net in enumerate(("sa", second)):
        if grads is not None:
            setattr(blk, "grad_" + net, ptr(grads[k]))
        if opts is not None:
            setattr(blk, "m_" + net, ptr(opts[k][0]))
            setattr(blk, "v_" + net, ptr(opts[k][1]))
    blk.t, blk.t_dev, blk.lr, blk.loss_out = int(t), ptr(t_dev), float(lr), ptr(loss_out)


def _dara_block(dims, precision, heads, batch, ws, n_src):
    sa, sas = heads
    return _lib.MobodyDara(struct_bytes=_BYTES[_lib.MobodyDara], precision=prec_id(precision), d=dims, n_src=int(n_src),
                           sa_blob=ptr(sa.blob), sa_blob_T=ptr(sa.blob_T), sas_blob=ptr(sas.blob), sas_blob_T=ptr(sas.blob_T),
                           state=ptr(batch[0]), action=ptr(batch[1]), next_state=ptr(batch[2]), workspace=ptr(ws))


def dara_classifier(dims, precision, heads, batch, noise_std, loss_out, ws, n_src=0, noise_sas=None, noise_sa=None, seed=0, call=0,
                    call_dev=None, call_offset=0, grads=None, opts=None, t=0, t_dev=None, lr=0.0):
    """One classifier update (dara.py:202-223) on the d.N rows [src | tar] of `batch`; loss_out[2] = (loss_sa, loss_sas).
    grads = (grad_sa, grad_sas): the gradient form; opts = ((m_sa, v_sa), (m_sas, v_sas)): ONE fused Adam over both heads at step
    t (or t_dev[0]) and rate lr.  Noise: explicit unit normals, or the device generator at (seed, call) -- call_dev[0] +
    call_offset when call_dev is given."""
    blk = _dara_block(dims, precision, heads, batch, ws, n_src)
    blk.noise_std, blk.noise_sas, blk.noise_sa = float(noise_std), ptr(noise_sas), ptr(noise_sa)
    blk.seed, blk.call, blk.call_dev, blk.call_offset = int(seed) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF, ptr(call_dev), int(call_offset)
    _pair_opt(blk, "sas", grads, opts, t, t_dev, lr, loss_out)
    check(load().mobody_dara_classifier(C.byref(blk), cur_stream()), "mobody_dara_classifier")


def dara_relabel(dims, precision, heads, batch, eta, ws, n_src=0, delta_out=None, log_out=None):
    """reward[:n_src] += eta * penalty of a noise-free classifier pass on the source rows (dara.py:281-292); delta_out[n_src] =
    the penalty, log_out[1] = its mean."""
    blk = _dara_block(dims, precision, heads, batch, ws, n_src)
    blk.reward, blk.eta, blk.delta_out, blk.log_out = ptr(batch[3]), float(eta), ptr(delta_out), ptr(log_out)
    check(load().mobody_dara_relabel(C.byref(blk), cur_stream()), "mobody_dara_relabel")


# IGDF (igdf.py): the contrastive update and the per-step filter in front of IQL's three calls, one block type (MobodyIgdf), and the
# row-weighted critic.  `encs` = (encoder_sa, encoder_ss) as objects with .blob / .blob_T and out_dim Z
def igdf_workspace(dims, n, Z, device):
    """Floats of the IGDF step's scratch: iql_workspace's (the same tensor serves the IQL calls) + the encoders' on n / 2n-1 rows."""
    return _workspace("mobody_igdf_workspace", device, C.byref(dims), int(n), int(Z))


def igdf_contrast(phi, psi_tar, psi_src, Z):
    """phi [n, ldz], psi_tar [n, ldz], psi_src [n-1, ldz] -> (loss[1], dz3_sa[n, Np3], dz3_ss[2n-1, Np3]) of the in-batch
    contrastive loss (igdf.py:427-440); columns >= Z of the inputs are not read."""
    n, ldz = phi.shape
    Np3 = (int(Z) + 15) // 16 * 16
    dev = phi.device
    dz_sa = torch.empty(n, Np3, dtype=torch.float32, device=dev)
    dz_ss = torch.empty(2 * n - 1, Np3, dtype=torch.float32, device=dev)
    lossp = torch.empty((n + 31) // 32, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    check(load().mobody_igdf_contrast(ptr(phi), ptr(psi_tar), ptr(psi_src), n, int(Z), ldz, ptr(dz_sa), ptr(dz_ss), ptr(lossp), ptr(loss),
                                      cur_stream()), "mobody_igdf_contrast")
    return loss, dz_sa, dz_ss


def igdf_select(score, k, importance_weight, kept=None, w=None):
    """(kept int32[k], w[k]): the positions of the k largest scores in ascending order and exp(importance_weight * score) there."""
    n = score.numel()
    kept = torch.empty(int(k), dtype=torch.int32, device=score.device) if kept is None else kept
    w = torch.empty(int(k), dtype=torch.float32, device=score.device) if w is None else w
    check(load().mobody_igdf_select(ptr(score), n, int(k), float(importance_weight), ptr(kept), ptr(w), cur_stream()), "mobody_igdf_select")
    return kept, w


def _igdf_block(dims, precision, encs, n, Z, batch, ws):
    sa, ss = encs
    return _lib.MobodyIgdf(struct_bytes=_BYTES[_lib.MobodyIgdf], precision=prec_id(precision), d=dims, n=int(n), Z=int(Z),
                           sa_blob=ptr(sa.blob), sa_blob_T=ptr(sa.blob_T), ss_blob=ptr(ss.blob), ss_blob_T=ptr(ss.blob_T),
                           state=ptr(batch[0]), action=ptr(batch[1]), next_state=ptr(batch[2]), workspace=ptr(ws))


def igdf_info(dims, precision, encs, n, Z, batch, loss_out, ws, grads=None, opts=None, t=0, t_dev=None, lr=0.0, bump=None):
    """One contrastive update (igdf.py:418-447) on batch = (state[n, S], action[n, A], next_state[2n-1, S] = [tar s' | src s']);
    loss_out[1].  grads = (grad_sa, grad_ss): the gradient form; opts = ((m_sa, v_sa), (m_ss, v_ss)): ONE fused Adam over both
    encoders at step t (or t_dev[0]) and rate lr; bump: a device word the last optimizer launch increments."""
    blk = _igdf_block(dims, precision, encs, n, Z, batch, ws)
    _pair_opt(blk, "ss", grads, opts, t, t_dev, lr, loss_out)
    blk.bump = ptr(bump)
    check(load().mobody_igdf_info(C.byref(blk), cur_stream()), "mobody_igdf_info")


def igdf_filter(dims, precision, encs, n, k, Z, importance_weight, staged, out, row_weight, ws, score_out=None, kept_out=None):
    """The data filter (igdf.py:494-524): scores the first n rows of `staged` = (state, action, next_state, reward, not_done) of
    [src(n) | tar], keeps the k best in ascending score order and writes `out` = [kept src | tar] (dims.N = k + n_tar rows) and
    row_weight[dims.N] = exp(importance_weight * score) on the kept rows, 1 on the target rows."""
    blk = _igdf_block(dims, precision, encs, n, Z, staged, ws)
    blk.k, blk.importance_weight, blk.reward, blk.not_done = int(k), float(importance_weight), ptr(staged[3]), ptr(staged[4])
    blk.out_state, blk.out_action, blk.out_next_state, blk.out_reward, blk.out_not_done = [ptr(t) for t in out]
    blk.row_weight, blk.score_out, blk.kept_out = ptr(row_weight), ptr(score_out), ptr(kept_out)
    check(load().mobody_igdf_filter(C.byref(blk), cur_stream()), "mobody_igdf_filter")


def igdf_critic(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws, grad=None, m=None, v=None, t=0, t_dev=None, lr=0.0,
                bump=None, row_weight=None):
    """iql_critic with the loss mean(w (q1 - y)^2) + mean(w (q2 - y)^2) (igdf.py:468-479); row_weight None: iql_critic."""
    _iql_call("mobody_igdf_critic", _iql_block(dims, hyp, lam, temp, T_max, nets, batch, adv, loss_out, ws), grad, m, v, t, t_dev, lr,
              bump=bump, extra=(ptr(row_weight),))


def value_loss_grad(qt, v, n_global):
    """qt [2,N] target twin-Q(s,a), v [N] -> (dz3[N,16], loss[1]) of the expectile V loss."""
    N = v.numel()
    dz3 = torch.empty(N, 16, dtype=torch.float32, device=v.device)
    loss = torch.empty(1, dtype=torch.float32, device=v.device)
    lossp = torch.empty((N + 255) // 256, dtype=torch.float32, device=v.device)
    check(load().mobody_value_loss_grad(ptr(qt), ptr(v), N, int(n_global), ptr(dz3), ptr(loss), ptr(lossp), cur_stream()),
          "mobody_value_loss_grad")
    return dz3, loss


def _adam(in_dim, out_dim, members, blob, blob_T, grad, m, v, target, t, t_dev, lr, tau, grad_scale, target_T, precision):
    blk = _lib.MobodyAdam(struct_bytes=_BYTES[_lib.MobodyAdam], in_dim=in_dim, out_dim=out_dim, members=members, blob=ptr(blob),
                          blob_T=ptr(blob_T), grad=ptr(grad), m=ptr(m), v=ptr(v), target=ptr(target), target_T=ptr(target_T),
                          t=t, t_dev=ptr(t_dev), lr=float(lr), tau=float(tau), grad_scale=float(grad_scale),
                          precision=prec_id(precision))
    check(load().mobody_adam_polyak(C.byref(blk), cur_stream()), "mobody_adam_polyak")


def adam_polyak(in_dim, out_dim, members, blob, blob_T, grad, m, v, target, t, lr, tau=-1.0, grad_scale=1.0, target_T=None,
                precision=0):
    _adam(in_dim, out_dim, members, blob, blob_T, grad, m, v, target, int(t), None, lr, tau, grad_scale, target_T, precision)


def adam_polyak_dev(in_dim, out_dim, members, blob, blob_T, grad, m, v, target, t_dev, lr, tau=-1.0, grad_scale=1.0,
                    target_T=None, precision=0):
    """adam_polyak with the step count read from the device word t_dev (graph replay)."""
    assert t_dev is not None, "adam_polyak_dev: t_dev is None"
    _adam(in_dim, out_dim, members, blob, blob_T, grad, m, v, target, 0, t_dev, lr, tau, grad_scale, target_T, precision)


# ------------------------------------------------------------------------------------------------
# replay data movement
# ------------------------------------------------------------------------------------------------
class RingView:
    """A row-interleaved replay ring: `store` is one [rows][pitch] fp32 tensor, a row = state | action | next_state | reward |
    not_done | padding (include/mobody_hip.h, mobody_ring_pitch).  Iterating yields the five field views (strided)."""

    def __init__(self, store, S, A):
        assert store.is_contiguous() and store.dtype == torch.float32 and store.shape[1] >= 2 * S + A + 2
        self.store, self.S, self.A = store, int(S), int(A)
        self.device = store.device

    def fields(self):
        S, A, st = self.S, self.A, self.store
        return st[:, :S], st[:, S:S + A], st[:, S + A:2 * S + A], st[:, 2 * S + A:2 * S + A + 1], st[:, 2 * S + A + 1:2 * S + A + 2]

    def __iter__(self):
        return iter(self.fields())

    def __getitem__(self, k):
        return self.fields()[k]


def ring_pitch(S, A):
    return int(load().mobody_ring_pitch(int(S), int(A)))


def buffer_view(b):
    """MobodyBufferView of a RingView or of a 5-tuple of separate contiguous tensors (state, action, next_state, reward, not_done)."""
    if isinstance(b, RingView):
        base, S, A = b.store.data_ptr(), b.S, b.A
        return _lib.MobodyBufferView(base, base + 4 * S, base + 4 * (S + A), base + 4 * (2 * S + A), base + 4 * (2 * S + A + 1), b.store.shape[1])
    return _lib.MobodyBufferView(*[ptr(t) for t in b], 0)


def _view_device(b):
    return b.device if isinstance(b, RingView) else b[0].device


def gather_batch(buffers, indices, S, A, out=None):
    """buffers: list of RingView or (state, action, next_state, reward, not_done) device tensors; indices: int32 device
    tensors. Returns the concatenated minibatch (state[N,S], action[N,A], next_state[N,S], reward[N,1], not_done[N,1])."""
    n = len(buffers)
    dev = _view_device(buffers[0])
    views = (_lib.MobodyBufferView * n)(*[buffer_view(b) for b in buffers])
    idx = [i.to(device=dev, dtype=torch.int32).contiguous() for i in indices]
    iptr = (C.c_void_p * n)(*[ptr(i) if i.numel() else None for i in idx])
    cnt = (C.c_int64 * n)(*[i.numel() for i in idx])
    N = sum(i.numel() for i in idx)
    if out is None:
        out = (torch.empty(N, S, device=dev), torch.empty(N, A, device=dev), torch.empty(N, S, device=dev),
               torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev))
    check(load().mobody_gather_batch(views, iptr, cnt, n, S, A, *[ptr(t) for t in out], cur_stream()),
          "mobody_gather_batch")
    return out


_scan_ws = {}


def ring_append(buf, cap, ptr_size, S, A, obs, act, next_obs, reward, terminal, keep=None):
    """buf = RingView or (state, action, next_state, reward, not_done) ring tensors; ptr_size int64[2] device tensor."""
    M = obs.shape[0]
    if M == 0:
        return
    dev = obs.device
    scan = _scan_ws.get(dev)
    if scan is None or scan.numel() < M + 1040:      # zeroed once: the append keeps its ticket words at zero itself
        scan = _scan_ws[dev] = torch.zeros(max(M + 1040, 2 * (scan.numel() if scan is not None else 0)), dtype=torch.int32, device=dev)
    check(load().mobody_ring_append(C.byref(buffer_view(buf)), cap, ptr(ptr_size), S, A, ptr(obs), ptr(act), ptr(next_obs),
                                    ptr(reward), ptr(terminal), ptr(keep), M, ptr(scan), cur_stream()),
          "mobody_ring_append")


# ------------------------------------------------------------------------------------------------
# small device-side helpers used by the host mirror
# ------------------------------------------------------------------------------------------------
def termination(task_id, next_obs):
    B, S = next_obs.shape
    done = torch.empty(B, 1, dtype=torch.uint8, device=next_obs.device)
    check(load().mobody_termination(task_id, ptr(next_obs), B, S, ptr(done), cur_stream()), "mobody_termination")
    return done


def rollout_mask(alive_in, terminal, penalty, env_filter, use_filter, keep, alive_out):
    B = terminal.shape[0]
    check(load().mobody_rollout_mask(ptr(alive_in), ptr(terminal), ptr(penalty), float(env_filter), int(bool(use_filter)),
                                     B, ptr(keep), ptr(alive_out), cur_stream()), "mobody_rollout_mask")


def sample_indices(seed, stream_id, counter, call_offset, n, size_dev, out=None):
    if out is None:
        out = torch.empty(n, dtype=torch.int32, device=size_dev.device)
    check(load().mobody_sample_indices(seed, stream_id, ptr(counter), call_offset, n, ptr(size_dev), ptr(out),
                                       cur_stream()), "mobody_sample_indices")
    return out


def counter_add(counter, inc=1):
    """counter: device int64[n]; every word += inc."""
    check(load().mobody_counter_add(ptr(counter), counter.numel(), inc, cur_stream()), "mobody_counter_add")


def par_penalty(next_state_true, next_state_model, reward, coef):
    n, S = next_state_true.shape
    check(load().mobody_par_penalty(ptr(next_state_true), ptr(next_state_model), ptr(reward), float(coef), n, S,
                                    cur_stream()), "mobody_par_penalty")


def _gather_rng_args(buffers, counts, seeds, call_offsets, counter, sizes, bump=()):
    """MobodyGatherRng of gather_batch_rng's arguments, and the host arrays it points into (keep them until the call returns)."""
    n = len(buffers)
    views = (_lib.MobodyBufferView * n)(*[buffer_view(b) for b in buffers])
    cnt = (C.c_int64 * n)(*[int(c) for c in counts])
    sd = (C.c_uint32 * n)(*[int(s) & 0xFFFFFFFF for s in seeds])
    off = (C.c_int64 * n)(*[int(o) for o in call_offsets])
    sz = (C.c_void_p * n)(*[ptr(s) for s in sizes])
    bp = (C.c_void_p * max(1, len(bump)))(*[ptr(t) for t in bump])
    return _lib.MobodyGatherRng(views, cnt, n, sd, off, ptr(counter), sz, bp, len(bump)), (views, cnt, sd, off, sz, bp)


def gather_batch_rng(buffers, counts, seeds, call_offsets, counter, sizes, S, A, out, bump=()):
    """Gather with device-drawn indices: buffers = list of RingView / 5-tuples, sizes = list of device int64[1] views,
    counter = device int64[1] or None.  `out` = (state, action, next_state, reward, not_done) destination tensors.
    bump: up to four device int64[1] words (not `counter`) the launch increments by one."""
    g, (views, cnt, sd, off, sz, bp) = _gather_rng_args(buffers, counts, seeds, call_offsets, counter, sizes, bump)
    check(load().mobody_gather_batch_rng(views, cnt, g.nbuf, S, A, sd, off, g.counter, sz, *[ptr(t) for t in out], bp, g.nbump,
                                         cur_stream()), "mobody_gather_batch_rng")
    return out


# ------------------------------------------------------------------------------------------------
# generic MLP gradient + DARA classifier pieces
# ------------------------------------------------------------------------------------------------
def mlp3_backward(blob_T, in_dim, out_dim, members, dz3, x, h1, h2, grad, ws=None):
    rows = x.shape[0]
    need = load().mobody_mlp3_backward_workspace(in_dim, out_dim, members, rows)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=x.device)
    check(load().mobody_mlp3_backward(ptr(blob_T), in_dim, out_dim, members, ptr(dz3), ptr(x), ptr(h1), ptr(h2), rows,
                                      ptr(grad), ptr(ws), cur_stream()), "mobody_mlp3_backward")
    return ws


def dara_inputs(s, a, s2, std, noise_sas=None, noise_sa=None, seed=0, call=0):
    N, S = s.shape
    A = a.shape[1]
    x_sas = torch.empty(N, 2 * S + A, dtype=torch.float32, device=s.device)
    x_sa = torch.empty(N, S + A, dtype=torch.float32, device=s.device)
    check(load().mobody_dara_inputs(ptr(s), ptr(a), ptr(s2), N, S, A, float(std), ptr(noise_sas), ptr(noise_sa), seed,
                                    call, ptr(x_sas), ptr(x_sa), cur_stream()), "mobody_dara_inputs")
    return x_sas, x_sa


def dara_loss_grad(z_sas, z_sa, n_src, labels=None):
    """z_*: logits [N,2].  Returns (dz_sas[N,16], dz_sa[N,16], loss[2] = (loss_sa, loss_sas))."""
    N = z_sas.shape[0]
    dev = z_sas.device
    dz_sas = torch.empty(N, 16, dtype=torch.float32, device=dev)
    dz_sa = torch.empty(N, 16, dtype=torch.float32, device=dev)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    lossp = torch.empty(2 * ((N + 255) // 256), dtype=torch.float32, device=dev)
    if labels is not None:
        labels = torch.as_tensor(labels).to(device=dev, dtype=torch.int32).contiguous()
    check(load().mobody_dara_loss_grad(ptr(z_sas), ptr(z_sa), ptr(labels), N, int(n_src), ptr(dz_sas), ptr(dz_sa),
                                       ptr(loss), ptr(lossp), cur_stream()), "mobody_dara_loss_grad")
    return dz_sas, dz_sa, loss


def dara_penalty(z_sas, z_sa, coef, reward=None, want_delta=False):
    n = z_sas.shape[0]
    delta = torch.empty(n, 1, dtype=torch.float32, device=z_sas.device) if want_delta or reward is None else None
    check(load().mobody_dara_penalty(ptr(z_sas), ptr(z_sa), n, float(coef), ptr(reward), ptr(delta), cur_stream()),
          "mobody_dara_penalty")
    return delta


# ------------------------------------------------------------------------------------------------
# dynamics pre-training
# ------------------------------------------------------------------------------------------------
def pretrain_transpose(blob, S, A, out=None, precision=0):
    """T blob of the pre-training parameter blob; `precision` (0 / "f32" or 4 / "f16x2") = the mode it will be trained in."""
    L = _lib.pretrain_layout(S, A)
    if prec_id(precision) == 4:
        _check_f16_weights([_mlp_w2(blob[L.off_enc:], L.enc, 7), _mlp_w2(blob[L.off_tr:], L.tr, 7),
                            _mlp_w2(blob[L.off_rw:], L.rw, 7)], "pretrain_transpose")
    bt = out if out is not None else torch.zeros(L.t_total_floats, dtype=torch.float32, device=blob.device)
    check(load().mobody_pretrain_transpose(S, A, ptr(blob), ptr(bt), prec_id(precision), cur_stream()), "mobody_pretrain_transpose")
    return bt


def pretrain_workspace(S, A, b, device):
    return _workspace("mobody_pretrain_workspace", device, S, A, b)


def pretrain_gather(state, action, next_state, reward, idx, start, b, out=None, start_dev=None):
    """idx: device int32 [7, n_idx].  Returns (xenc[7,2b,S], act[7,b,A], rew[7,b])."""
    S, A = state.shape[1], action.shape[1]
    dev = state.device
    assert idx.dtype == torch.int32 and idx.dim() == 2 and idx.shape[0] == 7 and idx.is_contiguous()
    xenc, act, rew = out or (torch.empty(7, 2 * b, S, dtype=torch.float32, device=dev),
                             torch.empty(7, b, A, dtype=torch.float32, device=dev),
                             torch.empty(7, b, dtype=torch.float32, device=dev))
    check(load().mobody_pretrain_gather(ptr(state), ptr(action), ptr(next_state), ptr(reward), ptr(idx), idx.shape[1], start,
                                        ptr(start_dev), b, S, A, ptr(xenc), ptr(act), ptr(rew), cur_stream()),
          "mobody_pretrain_gather")
    return xenc, act, rew


def _pretrain_block(cls, S, A, b, b_global, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, loss_out, ws, seed, call,
                    precision):
    """MobodyPretrain / MobodyPretrainMopo: what the two models and the gradient and fused forms share."""
    return cls(struct_bytes=_BYTES[cls], S=S, A=A, b=b, b_global=b_global, use_trg=int(bool(use_trg)),
               encoder_loss_coef=float(encoder_loss_coef), blob=ptr(blob), blob_T=ptr(blob_T), xenc=ptr(xenc), act=ptr(act),
               rew=ptr(rew), loss_out=ptr(loss_out), workspace=ptr(ws), seed=seed, call=call, precision=prec_id(precision))


def pretrain_grads(S, A, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, grad, loss_out, ws, noise6=None,
                   noise7=None, seed=0, call=0, b_global=None, precision=0, transition_coef=1.0, reward_coef=1.0):
    blk = _pretrain_block(_lib.MobodyPretrain, S, A, b, b if b_global is None else b_global, use_trg, encoder_loss_coef, blob,
                          blob_T, xenc, act, rew, loss_out, ws, seed, call, precision)
    blk.noise6, blk.noise7, blk.grad = ptr(noise6), ptr(noise7), ptr(grad)
    blk.transition_coef, blk.reward_coef = float(transition_coef), float(reward_coef)
    check(load().mobody_pretrain(C.byref(blk), cur_stream()), "mobody_pretrain")


def pretrain_update(S, A, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, m, v, t_main, t_za, lr, loss_out, ws,
                    noise6=None, noise7=None, seed=0, call=0, call_dev=None, t_dev=None, precision=0, loss_acc=None):
    blk = _pretrain_block(_lib.MobodyPretrain, S, A, b, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, loss_out, ws,
                          seed, call, precision)
    blk.noise6, blk.noise7, blk.transition_coef, blk.reward_coef = ptr(noise6), ptr(noise7), 1.0, 1.0
    blk.m, blk.v, blk.t_main, blk.t_za, blk.t_dev, blk.lr = ptr(m), ptr(v), t_main, t_za, ptr(t_dev), float(lr)
    blk.call_dev, blk.loss_acc = ptr(call_dev), ptr(loss_acc)
    check(load().mobody_pretrain(C.byref(blk), cur_stream()), "mobody_pretrain")


def pretrain_adam(S, A, use_trg, blob, blob_T, grad, m, v, t_main, t_za, lr, grad_scale=1.0, precision=0, net_mask=7, t_rw=None):
    """net_mask: bit 0 state encoder, 1 decoder, 2 reward head (a net without a gradient this step is skipped); t_rw: the reward
    head's own step count (default: t_main)."""
    check(load().mobody_pretrain_adam(S, A, int(bool(use_trg)), ptr(blob), ptr(blob_T), ptr(grad), ptr(m), ptr(v), t_main,
                                      t_za, float(lr), float(grad_scale), prec_id(precision), int(net_mask),
                                      t_main if t_rw is None else t_rw, cur_stream()), "mobody_pretrain_adam")


def pretrain_za_adam(S, A, use_trg, blob, grad, m, v, t_za, lr, grad_scale=1.0):
    """Adam step of one action encoder only (the second one of a learn_src_trg step)."""
    check(load().mobody_pretrain_za_adam(S, A, int(bool(use_trg)), ptr(blob), ptr(grad), ptr(m), ptr(v), t_za, float(lr),
                                         float(grad_scale), cur_stream()), "mobody_pretrain_za_adam")


# ---- MOPO ablation pre-training (MobodyPretrainMopoLayout) ----
def pretrain_mopo_transpose(blob, S, A, out=None, precision=0):
    L = _lib.pretrain_mopo_layout(S, A)
    if prec_id(precision) == 4:
        _check_f16_weights([_mlp_w2(blob[L.off_dyn:], L.dyn, 7), _mlp_w2(blob[L.off_rw:], L.rw, 7)], "pretrain_mopo_transpose")
    bt = out if out is not None else torch.zeros(L.t_total_floats, dtype=torch.float32, device=blob.device)
    check(load().mobody_pretrain_mopo_transpose(S, A, ptr(blob), ptr(bt), prec_id(precision), cur_stream()),
          "mobody_pretrain_mopo_transpose")
    return bt


def pretrain_mopo_workspace(S, A, b, device):
    return _workspace("mobody_pretrain_mopo_workspace", device, S, A, b)


def pretrain_mopo_grads(S, A, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, grad, loss_out, ws, noise=None,
                        seed=0, call=0, b_global=None, precision=0):
    """noise: [7, b, S] fake-next-state draw (None: device Philox at (seed, call))."""
    blk = _pretrain_block(_lib.MobodyPretrainMopo, S, A, b, b if b_global is None else b_global, use_trg, encoder_loss_coef, blob,
                          blob_T, xenc, act, rew, loss_out, ws, seed, call, precision)
    blk.noise, blk.grad = ptr(noise), ptr(grad)
    check(load().mobody_pretrain_mopo(C.byref(blk), cur_stream()), "mobody_pretrain_mopo")


def pretrain_mopo_update(S, A, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, m, v, t, lr, loss_out, ws,
                         noise=None, seed=0, call=0, call_dev=None, t_dev=None, precision=0, loss_acc=None):
    blk = _pretrain_block(_lib.MobodyPretrainMopo, S, A, b, b, use_trg, encoder_loss_coef, blob, blob_T, xenc, act, rew, loss_out,
                          ws, seed, call, precision)
    blk.noise, blk.m, blk.v, blk.t, blk.t_dev, blk.lr = ptr(noise), ptr(m), ptr(v), t, ptr(t_dev), float(lr)
    blk.call_dev, blk.loss_acc = ptr(call_dev), ptr(loss_acc)
    check(load().mobody_pretrain_mopo(C.byref(blk), cur_stream()), "mobody_pretrain_mopo")


def pretrain_mopo_adam(S, A, blob, blob_T, grad, m, v, t, lr, grad_scale=1.0, precision=0):
    check(load().mobody_pretrain_mopo_adam(S, A, ptr(blob), ptr(blob_T), ptr(grad), ptr(m), ptr(v), t, float(lr),
                                           float(grad_scale), prec_id(precision), cur_stream()), "mobody_pretrain_mopo_adam")


def dyn_validate_mopo(blob, mopo_blob, S, A, obs, act, next_obs, rew, ws=None):
    """validate() of a mopo model: mean_e = s + MLP_e([s, a]) from `mopo_blob` (mobody_mlp_layout(S + A, S, 7)), the reward
    head from the inference blob.  out[0:7] transition MSE, out[7:14] reward MSE (device tensor)."""
    B = obs.shape[0]
    ws = _workspace("mobody_dyn_validate_workspace", obs.device, S, A, B, ws=ws)
    out = torch.empty(14, dtype=torch.float32, device=obs.device)
    check(load().mobody_dyn_validate_mopo(ptr(blob), ptr(mopo_blob), S, A, ptr(_f32(obs)), ptr(_f32(act)), ptr(_f32(next_obs)),
                                          ptr(_f32(rew).reshape(-1).contiguous()), B, ptr(out), ptr(ws), cur_stream()),
          "mobody_dyn_validate_mopo")
    return out


def dyn_validate(blob, S, A, obs, act, next_obs, rew, use_trg, ws=None):
    """validate(): out[0:7] per-member transition MSE, out[7:14] per-member reward MSE (device tensor)."""
    B = obs.shape[0]
    ws = _workspace("mobody_dyn_validate_workspace", obs.device, S, A, B, ws=ws)
    out = torch.empty(14, dtype=torch.float32, device=obs.device)
    check(load().mobody_dyn_validate(ptr(blob), S, A, ptr(_f32(obs)), ptr(_f32(act)), ptr(_f32(next_obs)),
                                     ptr(_f32(rew).reshape(-1).contiguous()), B, int(bool(use_trg)), ptr(out), ptr(ws),
                                     cur_stream()), "mobody_dyn_validate")
    return out


def rollout(dyn_blob, actor_blob, S, A, task_id, max_action, init_obs, H, elites, seed, call0, penalty_coef, use_penalty,
            use_trg, env_filter, filter_bad_rollout, buf, cap, ptr_size, ws=None, dyn_planes=None, actor_blob_T=None,
            precision=0, mopo=None, uncertainty_mode=0, call_dev=None):
    """H-step on-device rollout of `init_obs` appended to the ring `buf` (mobody_ens_rollout).  mopo = (blob, blob_T) of the
    MOPO ablation's MLP; uncertainty_mode: name or MOBODY_UNC_* id.  Returns the workspace."""
    init_obs = _f32(init_obs)
    B = init_obs.shape[0]
    view = buffer_view(buf)
    model = _model_fields(dyn_blob, dyn_planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg)
    a = _lib.MobodyEnsRollout(struct_bytes=_BYTES[_lib.MobodyEnsRollout], actor_blob=ptr(actor_blob), actor_blob_T=ptr(actor_blob_T),
                              init_obs=ptr(init_obs), B=B, H=int(H), call0=call0, max_action=float(max_action),
                              penalty_coef=float(penalty_coef), env_filter=float(env_filter), use_penalty=int(bool(use_penalty)),
                              filter_bad_rollout=int(bool(filter_bad_rollout)), ring=C.pointer(view), cap=cap,
                              ptr_size=ptr(ptr_size), **model)
    return _run_with_workspace("mobody_ens_rollout", a, ws, init_obs.device)


def eval_state(B, S, device):
    """The caller-owned row state of mobody_ens_evaluate: obs_state[B,S], alive uint8[B], ret / pen_sum / disc float[B],
    length int32[B].  Uninitialised: the first call (resume=False) sets it."""
    f = dict(dtype=torch.float32, device=device)
    return dict(obs_state=torch.empty(B, S, **f), alive=torch.empty(B, dtype=torch.uint8, device=device),
                ret=torch.empty(B, **f), pen_sum=torch.empty(B, **f), disc=torch.empty(B, **f),
                length=torch.empty(B, dtype=torch.int32, device=device))


def ens_evaluate(dyn_blob, actor_blob, S, A, task_id, max_action, init_obs, H, elites, seed, call0, state, use_trg=True,
                 discount=1.0, resume=False, ws=None, dyn_planes=None, actor_blob_T=None, precision=0, mopo=None,
                 uncertainty_mode=0, call_dev=None):
    """H steps of policy evaluation in the model on the row state `state` (eval_state; mobody_ens_evaluate): per row the
    discounted sum of the ensemble's raw mean rewards up to and including the terminating step, the penalty sum, the
    length and the alive flag.  init_obs may be None when resume.  Returns the workspace."""
    B = state["obs_state"].shape[0]
    if init_obs is not None:
        init_obs = _f32(init_obs)
        assert init_obs.shape == (B, S)
    model = _model_fields(dyn_blob, dyn_planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg)
    a = _lib.MobodyEnsEval(struct_bytes=_BYTES[_lib.MobodyEnsEval], actor_blob=ptr(actor_blob), actor_blob_T=ptr(actor_blob_T),
                           init_obs=ptr(init_obs), B=B, H=int(H), call0=call0, max_action=float(max_action),
                           discount=float(discount), resume=int(bool(resume)), obs_state=ptr(state["obs_state"]),
                           alive=ptr(state["alive"]), ret=ptr(state["ret"]), pen_sum=ptr(state["pen_sum"]),
                           disc=ptr(state["disc"]), length=ptr(state["length"]), **model)
    return _run_with_workspace("mobody_ens_evaluate", a, ws, state["obs_state"].device)


def eval_policy_state(B, S, device):
    """The caller-owned row state of mobody_ens_evaluate_policy: eval_state plus member int32[B] (read and written in member
    mode only).  Uninitialised: the first call (resume=False) sets it."""
    st = eval_state(B, S, device)
    st["member"] = torch.empty(B, dtype=torch.int32, device=device)
    return st


def ens_evaluate_policy(dyn_blob, policy_blob, S, A, task_id, max_action, init_obs, H, elites, seed, call0, state, head=0,
                        members=False, use_trg=True, discount=1.0, resume=False, ws=None, dyn_planes=None, policy_blob_T=None,
                        precision=0, mopo=None, uncertainty_mode=0, call_dev=None):
    """ens_evaluate for both policy head forms (mobody_ens_evaluate_policy).  head 0: `policy_blob` is the deterministic actor
    (S, A, 1); head 1: the Gaussian policy (S, 2A, 1), the action is max_action * tanh(mu).  members: every row keeps the elite
    state["member"][b] = elites[b % len(elites)] for its whole episode (state from eval_policy_state).  Returns the workspace."""
    B = state["obs_state"].shape[0]
    if init_obs is not None:
        init_obs = _f32(init_obs)
        assert init_obs.shape == (B, S)
    model = _model_fields(dyn_blob, dyn_planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg)
    a = _lib.MobodyEnsEvalPolicy(struct_bytes=_BYTES[_lib.MobodyEnsEvalPolicy], policy_blob=ptr(policy_blob),
                                 policy_blob_T=ptr(policy_blob_T), init_obs=ptr(init_obs), B=B, H=int(H), call0=call0,
                                 max_action=float(max_action), discount=float(discount), resume=int(bool(resume)),
                                 obs_state=ptr(state["obs_state"]), alive=ptr(state["alive"]), ret=ptr(state["ret"]),
                                 pen_sum=ptr(state["pen_sum"]), disc=ptr(state["disc"]), length=ptr(state["length"]),
                                 head=int(head), member_mode=int(bool(members)), member=ptr(state["member"]) if members else None,
                                 **model)
    return _run_with_workspace("mobody_ens_evaluate_policy", a, ws, state["obs_state"].device)


def eval_summary(state, G=1, out=None):
    """The figures of a finished row state by member group b % G (mobody_eval_summary).  Returns `out`, float32 [4 (G + 1) + 1] on
    the device: (mean return, mean length, mean penalty sum, alive share) per group, the same four over all rows, and the NaN
    flag (int32 bits in the last word).  No synchronisation: the caller reads `out` once."""
    dev = state["ret"].device
    if out is None:
        out = torch.empty(4 * (int(G) + 1) + 1, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 4 * (int(G) + 1) + 1
    flag = out[4 * (int(G) + 1):4 * (int(G) + 1) + 1]
    check(load().mobody_eval_summary(ptr(state["ret"]), ptr(state["pen_sum"]), ptr(state["length"]), ptr(state["alive"]),
                                     state["ret"].shape[0], int(G), ptr(out), ptr(flag), cur_stream()), "mobody_eval_summary")
    return out


def replay_state(B, H, S, A, device):
    """The caller-owned row state and tables of mobody_ens_replay: obs_state[B,S], act_state[B,A], obs_err / rew_err /
    penalty float[H,B], term_model uint8[H,B].  Uninitialised: the call sets every word."""
    f = dict(dtype=torch.float32, device=device)
    return dict(obs_state=torch.empty(B, S, **f), act_state=torch.empty(B, A, **f), obs_err=torch.empty(H, B, **f),
                rew_err=torch.empty(H, B, **f), penalty=torch.empty(H, B, **f),
                term_model=torch.empty(H, B, dtype=torch.uint8, device=device))


def ens_replay(dyn_blob, S, A, task_id, data, data_rows, row0, H, elites, seed, call0, state, reset_every=0, use_trg=True,
               ws=None, dyn_planes=None, precision=0, mopo=None, uncertainty_mode=0, call_dev=None):
    """Open-loop error of the model over B recorded windows of `data` (a RingView or a 5-tuple of separate tensors, rows in
    dataset order) starting at the device int64 rows `row0` (mobody_ens_replay): the model is fed the recorded actions and
    its state, reward and termination flag are compared with the recorded ones for H steps, into the tables of `state`
    (replay_state).  reset_every = K > 0 puts the recorded next state back after every K-th step.  Returns the workspace."""
    assert row0.dtype == torch.int64 and row0.dim() == 1
    B = row0.shape[0]
    assert state["obs_state"].shape == (B, S) and state["obs_err"].shape == (int(H), B)
    view = buffer_view(data)
    model = _model_fields(dyn_blob, dyn_planes, mopo, precision, S, A, task_id, elites, seed, uncertainty_mode, call_dev, use_trg)
    a = _lib.MobodyEnsReplay(struct_bytes=_BYTES[_lib.MobodyEnsReplay], data=C.pointer(view), data_rows=int(data_rows), row0=ptr(row0),
                             B=B, H=int(H), reset_every=int(reset_every), call0=call0, obs_state=ptr(state["obs_state"]),
                             act_state=ptr(state["act_state"]), obs_err=ptr(state["obs_err"]), rew_err=ptr(state["rew_err"]),
                             penalty=ptr(state["penalty"]), term_model=ptr(state["term_model"]), **model)
    return _run_with_workspace("mobody_ens_replay", a, ws, row0.device)


# ---- wide MLPs (csrc/wide.hip): BOSA's VAE nets, exact fp32 whatever MOBODY_MFMA says ------------------------------------
def wide_mlp3_forward(blob, L, sources, out_mode="raw", max_action=1.0, save=False, precision=0, source_rows=None):
    """The wide net `blob` (layout L = _lib.wide_layout(...)) on x = the `sources` (up to three) side by side.  A 2-D source
    [rows, w] is read by every member, a 3-D one [members, rows, w] holds one copy per member.  source_rows: one entry per
    source, None / 0 for a full source or its period p (src_rows): the source is then passed as [p, w] / [members, p, w] and row
    r of x reads its row r % p; at least one source is full and gives `rows`.  Returns out [members, rows, out_dim], or with
    save=True (out, x, h1, h2): the tensors mobody_wide_mlp3_backward reads, x [1 or members, rows, Kp1] and h1, h2
    [members, rows, Hp]."""
    srcs = [_f32(s) for s in sources]
    assert 1 <= len(srcs) <= 3
    periods = [int(p or 0) for p in (source_rows if source_rows is not None else [0] * len(srcs))]
    assert len(periods) == len(srcs) and not all(periods), periods
    rows, dev, E = [s.shape[-2] for s, p in zip(srcs, periods) if not p][0], blob.device, L.members
    shared = all(s.dim() == 2 for s in srcs)
    for s, p in zip(srcs, periods):                  # a period beyond `rows` is the entry point's to refuse
        assert s.shape[-2] == (p or rows) and (s.dim() == 2 or (s.dim() == 3 and s.shape[0] == E)), tuple(s.shape)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out = new(E, rows, L.out_dim)
    x, h1, h2 = new(1 if shared else E, rows, L.Kp1), new(E, rows, L.Hp), new(E, rows, L.Hp)
    a = _lib.block(_lib.MobodyWideFwd, precision=prec_id(precision), layout=L, blob=ptr(blob), x_shared=int(shared), rows=rows,
                   out_mode=_lib.WIDE_OUT_MODES[out_mode], max_action=float(max_action), out=ptr(out), save_x=ptr(x),
                   save_h1=ptr(h1), save_h2=ptr(h2))
    for i, s in enumerate(srcs):
        setattr(a, "src%d" % i, ptr(s))
        setattr(a, "src_width%d" % i, s.shape[-1])
        setattr(a, "src_member_stride%d" % i, 0 if s.dim() == 2 else s.shape[-2] * s.shape[-1])
        setattr(a, "src_rows%d" % i, periods[i])
    check(load().mobody_wide_mlp3_forward(C.byref(a), cur_stream()), "mobody_wide_mlp3_forward")
    return (out, x, h1, h2) if save else out


def wide_mlp3_backward(blob, L, dz3, x, h1, h2, grad=None, dx_cols=None, ws=None, precision=0):
    """Parameter gradient (blob layout, padding written as zero) of a wide net from dz3 [members, rows, out_dim] and the
    forward's saves; dx_cols = (c0, c1): also d loss / d x[:, c0:c1] as [members, rows, c1 - c0].  Returns (grad, dx or None)."""
    rows, dev, E = dz3.shape[1], blob.device, L.members
    grad = torch.empty(L.total_floats, dtype=torch.float32, device=dev) if grad is None else grad
    need = load().mobody_wide_mlp3_backward_workspace(C.byref(L), rows)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    dx, c0, c1 = None, 0, 0
    if dx_cols is not None:
        c0, c1 = dx_cols
        assert 0 <= c0 < c1 <= L.in_dim, dx_cols
        dx = torch.empty(E, rows, c1 - c0, dtype=torch.float32, device=dev)
    a = _lib.block(_lib.MobodyWideBwd, precision=prec_id(precision), layout=L, blob=ptr(blob), dz3=ptr(dz3), x=ptr(x), h1=ptr(h1),
                   h2=ptr(h2), x_shared=int(x.shape[0] == 1), rows=rows, grad=ptr(grad), dx=ptr(dx), dx_col0=c0, dx_col1=c1, workspace=ptr(ws))
    check(load().mobody_wide_mlp3_backward(C.byref(a), cur_stream()), "mobody_wide_mlp3_backward")
    return grad, dx


def wide_adam(blob, grad, m, v, lr, t=0, t_dev=None):
    """One torch-default Adam step on a flat wide blob (or several laid end to end); t_dev: device int64 step count."""
    a = _lib.block(_lib.MobodyWideAdam, blob=ptr(blob), grad=ptr(grad), m=ptr(m), v=ptr(v), n=blob.numel(), t=int(t), t_dev=ptr(t_dev),
                   lr=float(lr))
    check(load().mobody_wide_adam(C.byref(a), cur_stream()), "mobody_wide_adam")


# ---- BOSA's VAE stage (csrc/bosa.hip) -------------------------------------------------------------------------------------
def bosa_block(kind, S, A, hidden, members, B, beta, max_action=1.0, num_samples=0, **fields):
    """A MobodyBosaVae block of the VAE `kind` ('policy' | 'dynamics'); tensors by field name."""
    return _lib.block(_lib.MobodyBosaVae, kind=_lib.BOSA_KINDS[kind], S=int(S), A=int(A), hidden=int(hidden), members=int(members),
                      B=int(B), beta=float(beta), max_action=float(max_action), num_samples=int(num_samples),
                      **{k: (ptr(v) if isinstance(v, torch.Tensor) or v is None else v) for k, v in fields.items()})


def bosa_workspace(blk, device):
    n = load().mobody_bosa_workspace(C.byref(blk))
    if n < 0:
        raise _lib.MobodyError("mobody_bosa_workspace: bad block: " + load().mobody_last_error().decode(errors="replace"))
    return torch.empty(n, dtype=torch.float32, device=device)


def bosa_reparam(enc, eps, beta, dz=None):
    """enc [n, 2 Lz], eps [n, Lz] -> (z [n, Lz], kl [1], denc [n, 2 Lz] or None): clamp / exp / reparameterise, the KL term and
    -- dz = dLoss/dz given -- the gradient of Loss + beta KL with respect to enc (bosa.py:116-117, :68, :521)."""
    n, Lz = eps.shape
    dev = enc.device
    z = torch.empty(n, Lz, dtype=torch.float32, device=dev)
    kl = torch.empty(1, dtype=torch.float32, device=dev)
    denc = torch.empty(n, 2 * Lz, dtype=torch.float32, device=dev) if dz is not None else None
    lossp = torch.empty((n * Lz + 255) // 256, dtype=torch.float32, device=dev)
    check(load().mobody_bosa_reparam(ptr(enc), ptr(eps), ptr(dz), n, Lz, float(beta), ptr(z), ptr(denc), ptr(lossp), ptr(kl),
                                     cur_stream()), "mobody_bosa_reparam")
    return z, kl, denc


def bosa_vae(blk):
    check(load().mobody_bosa_vae(C.byref(blk), cur_stream()), "mobody_bosa_vae")


def bosa_loglik(blk):
    check(load().mobody_bosa_loglik(C.byref(blk), cur_stream()), "mobody_bosa_loglik")


def wide_mlp3_input_grad(blob, L, dz3, h1, h2, dx_cols, ws=None, precision=0, x_shared=True):
    """d loss / d x[:, c0:c1] of a wide net whose parameters are held fixed, as [members, rows, c1 - c0]: the three input-gradient
    products of wide_mlp3_backward without its weight gradients, so the same bits.  x_shared: the block's field, as the forward that
    saved h1 / h2 had it (x itself is not read)."""
    rows, dev, E = dz3.shape[1], blob.device, L.members
    need = load().mobody_wide_mlp3_backward_workspace(C.byref(L), rows)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
    c0, c1 = dx_cols
    assert 0 <= c0 < c1 <= L.in_dim, dx_cols
    dx = torch.empty(E, rows, c1 - c0, dtype=torch.float32, device=dev)
    a = _lib.block(_lib.MobodyWideBwd, precision=prec_id(precision), layout=L, blob=ptr(blob), dz3=ptr(dz3), h1=ptr(h1), h2=ptr(h2),
                   x_shared=int(bool(x_shared)), rows=rows, dx=ptr(dx), dx_col0=c0, dx_col1=c1, workspace=ptr(ws))
    check(load().mobody_wide_mlp3_input_grad(C.byref(a), cur_stream()), "mobody_wide_mlp3_input_grad")
    return dx


def bosa_loglik_grad_workspace(blk, device):
    n = load().mobody_bosa_loglik_grad_workspace(C.byref(blk))
    if n < 0:
        raise _lib.MobodyError("mobody_bosa_loglik_grad_workspace: bad block: " + load().mobody_last_error().decode(errors="replace"))
    return torch.empty(n, dtype=torch.float32, device=device)


def bosa_loglik_grad(blk, dll_da):
    """The policy VAE's estimator (blk.ll, blk.w_out as bosa_loglik writes them) and dll_da [B, A] = d ll / d blk.action."""
    check(load().mobody_bosa_loglik_grad(C.byref(blk), ptr(dll_da), cur_stream()), "mobody_bosa_loglik_grad")


# ---- BOSA's critic / actor stage without a torch op (csrc/bosa_stage2.hip) ------------------------------------------
def bosa_target_block(actor, q, next_state, q_next, expl_noise, noise_clip, noise=None, seed=0, call=0, call_dev=None, ws=None):
    """A MobodyBosaTarget block: `actor`, `q` the TARGET nets (objects with blob / blob_T / precision / max_action, the twin-Q's
    in_dim = S + A)."""
    N, S = next_state.shape
    return _lib.block(_lib.MobodyBosaTarget, precision=prec_id(actor.precision), S=S, A=actor.out_dim, N=N, actor_blob=ptr(actor.blob),
                      actor_blob_T=ptr(actor.blob_T), q_blob=ptr(q.blob), q_blob_T=ptr(q.blob_T), next_state=ptr(next_state), noise=ptr(noise),
                      seed=seed, call=call, call_dev=ptr(call_dev), expl_noise=float(expl_noise), noise_clip=float(noise_clip),
                      max_action=float(actor.max_action), q_next=ptr(q_next), workspace=ptr(ws))


def bosa_target_workspace(blk, device):
    n = load().mobody_bosa_target_workspace(C.byref(blk))
    if n < 0:
        raise _lib.MobodyError("mobody_bosa_target_workspace: bad block: " + load().mobody_last_error().decode(errors="replace"))
    return torch.empty(n, dtype=torch.float32, device=device)


def bosa_target(blk):
    """q_next [N] = min Q_target(s', clamp(pi_target(s') + clamp(noise * expl_noise, +-clip), +-max_action)) (bosa.py:570-577)."""
    check(load().mobody_bosa_target(C.byref(blk), cur_stream()), "mobody_bosa_target")


def bosa_stage2_rows(N, mask=None, row_weight=None, dll=None, dpi=None, dpi_scale=0.0, A=0):
    """row_weight = mask * 0.5 and / or dpi = dll * dpi_scale, in one launch."""
    blk = _lib.block(_lib.MobodyBosaStage2, N=N, A=A, mask=ptr(mask), row_weight=ptr(row_weight), dll=ptr(dll), dpi=ptr(dpi),
                     dpi_scale=float(dpi_scale))
    check(load().mobody_bosa_stage2_rows(C.byref(blk), cur_stream()), "mobody_bosa_stage2_rows")


def bosa_stage2_words(N, words, mask_mean=None, closs=None, cons_coef=0.0, ll=None, aloss=None, lamda=0.0, bump=None, bump_inc=()):
    """The stage's logged words (closs given: the critic's four; ll given: the actor's three) in one launch, which then adds
    bump_inc[k] to the device int64 words bump[k]."""
    blk = _lib.block(_lib.MobodyBosaStage2, N=N, mask_mean=ptr(mask_mean), closs=ptr(closs), cons_coef=float(cons_coef), ll=ptr(ll),
                     aloss=ptr(aloss), lamda=float(lamda), words=ptr(words), bump=ptr(bump), nbump=len(bump_inc),
                     bump_inc=(C.c_int64 * 4)(*[int(x) for x in bump_inc]))
    check(load().mobody_bosa_stage2_words(C.byref(blk), cur_stream()), "mobody_bosa_stage2_words")


# ---- fitted Q evaluation (csrc/fqe.hip) -----------------------------------------------------------------------------
def _block_workspace(name, blk, device):
    n = getattr(load(), name)(C.byref(blk))
    if n < 0:
        raise _lib.MobodyError(name + ": bad block: " + load().mobody_last_error().decode(errors="replace"))
    return torch.empty(n, dtype=torch.float32, device=device)


def _fqe_fields(policy, head, q, state, policy_T):
    """The fields both FQE blocks share: `policy` the frozen net (head 0: out_dim A; head 1: out_dim 2 A), `q` a twin-Q (in_dim
    S + A) whose precision the call runs at; policy_T: the policy's T blob in THAT precision's format (None: the policy's own)."""
    S = state.shape[1]
    return dict(precision=prec_id(q.precision), head=int(head), S=S, A=q.in_dim - S, policy_blob=ptr(policy.blob),
                policy_blob_T=ptr(policy.blob_T if policy_T is None else policy_T), q_blob=ptr(q.blob), q_blob_T=ptr(q.blob_T),
                max_action=float(policy.max_action))


def fqe_target_block(policy, head, q_target, next_state, q_next, action_out=None, ws=None, policy_T=None):
    """A MobodyFqeTarget block: `q_target` FQE's target twin-Q."""
    return _lib.block(_lib.MobodyFqeTarget, N=next_state.shape[0], next_state=ptr(next_state), action_out=ptr(action_out),
                      q_next=ptr(q_next), workspace=ptr(ws), **_fqe_fields(policy, head, q_target, next_state, policy_T))


def fqe_target_workspace(blk, device):
    return _block_workspace("mobody_fqe_target_workspace", blk, device)


def fqe_target(blk):
    """q_next [N] = mean over the two members of Q_targ(s', pi(s')), pi by the block's head rule."""
    check(load().mobody_fqe_target(C.byref(blk), cur_stream()), "mobody_fqe_target")


def fqe_value_block(policy, head, q, state, out, nan_flag, q_out=None, ws=None, policy_T=None):
    """A MobodyFqeValue block: `q` FQE's online twin-Q, out float32[4], nan_flag int32[1], q_out [2][B] or None."""
    return _lib.block(_lib.MobodyFqeValue, B=state.shape[0], state=ptr(state), q_out=ptr(q_out), out=ptr(out), nan_flag=ptr(nan_flag),
                      workspace=ptr(ws), **_fqe_fields(policy, head, q, state, policy_T))


def fqe_value_workspace(blk, device):
    return _block_workspace("mobody_fqe_value_workspace", blk, device)


def fqe_value(blk):
    """out = (mean q0, mean q1, mean 0.5 (q0 + q1), max |q0 - q1|) of Q(s0, pi(s0)) over the block's start states."""
    check(load().mobody_fqe_value(C.byref(blk), cur_stream()), "mobody_fqe_value")


# ------------------------------------------------------------------------------------------------
# the analytic control task (mobody_amd/task.py; csrc/task.hip)
# ------------------------------------------------------------------------------------------------
TASK_CONSTANTS = ("f", "grav", "dt", "g", "c", "lam", "k", "h", "sigma", "alive_bonus", "ctrl_cost", "max_action")


def task_params(S, A, task_id, mu, gain, bmat, **constants):
    """MobodyTaskParams of device tables mu [S], gain [A], bmat [S][A] and the twelve constants by name (TASK_CONSTANTS)."""
    assert set(constants) == set(TASK_CONSTANTS), set(constants) ^ set(TASK_CONSTANTS)
    for t, n in ((mu, S), (gain, A), (bmat, S * A)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    return _lib.MobodyTaskParams(S=S, A=A, task=task_id, mu=ptr(mu), gain=ptr(gain), bmat=ptr(bmat),
                                 **{k: float(v) for k, v in constants.items()})


def task_step(p, obs, act, noise=None, alive=None, seed=0, call=0, call_dev=None, out=None):
    """One step of the task `p` on B rows (mobody_task_step).  Returns dict(next_obs [B,S], reward [B], terminal uint8 [B]);
    `out` may hand in those tensors (next_obs may be `obs`)."""
    obs, act = _f32(obs), _f32(act)
    dev, B = obs.device, obs.shape[0]
    assert obs.shape == (B, p.S) and act.shape == (B, p.A)
    if noise is not None:
        noise = _f32(noise, dev)
        assert noise.shape == (B, p.S)
    o = out or {}
    nxt = o["next_obs"] if "next_obs" in o else torch.empty(B, p.S, dtype=torch.float32, device=dev)
    rew = o["reward"] if "reward" in o else torch.empty(B, dtype=torch.float32, device=dev)
    term = o["terminal"] if "terminal" in o else torch.empty(B, dtype=torch.uint8, device=dev)
    a = _lib.block(_lib.MobodyTaskStep, p=p, obs=ptr(obs), act=ptr(act), B=B, noise=ptr(noise), alive=ptr(alive), seed=seed,
                   call=call & 0xFFFFFFFF, call_dev=ptr(call_dev), next_obs=ptr(nxt), reward=ptr(rew), terminal=ptr(term))
    check(load().mobody_task_step(C.byref(a), cur_stream()), "mobody_task_step")
    return dict(next_obs=nxt, reward=rew, terminal=term)


def task_evaluate(p, policy_blob, head, init_obs, H, seed, call0, state, discount=1.0, resume=False, ws=None, policy_blob_T=None,
                  precision=0, call_dev=None, ctrl=1, ctrl_push=0.0, ctrl_eps=0.0):
    """H steps of the policy in the task `p` on the row state `state` (eval_state; mobody_task_evaluate).  head 0 / 1: the two
    policy forms; head 2: the built-in controller (ctrl, ctrl_push, ctrl_eps; policy_blob may be None).  Returns the workspace."""
    B = state["obs_state"].shape[0]
    if init_obs is not None:
        init_obs = _f32(init_obs)
        assert init_obs.shape == (B, p.S)
    a = _lib.block(_lib.MobodyTaskEval, precision=prec_id(precision), p=p, policy_blob=ptr(policy_blob), policy_blob_T=ptr(policy_blob_T),
                   init_obs=ptr(init_obs), B=B, H=int(H), head=int(head), ctrl=int(ctrl), resume=int(bool(resume)),
                   ctrl_push=float(ctrl_push), ctrl_eps=float(ctrl_eps), seed=seed, call0=call0 & 0xFFFFFFFF, call_dev=ptr(call_dev),
                   discount=float(discount), obs_state=ptr(state["obs_state"]), alive=ptr(state["alive"]), ret=ptr(state["ret"]),
                   pen_sum=ptr(state["pen_sum"]), disc=ptr(state["disc"]), length=ptr(state["length"]))
    return _run_with_workspace("mobody_task_evaluate", a, ws, state["obs_state"].device)


def task_collect(p, lanes, L, time_limit, ctrl, ctrl_push, ctrl_eps, split, init_std, seed, call0=0, ws=None):
    """`lanes` lanes of L steps each under the built-in controllers (mobody_task_collect): ctrl / ctrl_push / ctrl_eps are pairs,
    lane b < split runs the first.  Returns device tensors observations [lanes L, S], actions, next_observations, rewards
    [lanes L], terminals uint8 [lanes L]; row b L + t is step t of lane b."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n, f = int(lanes) * int(L), dict(dtype=torch.float32, device=dev)
    out = dict(observations=torch.empty(n, p.S, **f), actions=torch.empty(n, p.A, **f), next_observations=torch.empty(n, p.S, **f),
               rewards=torch.empty(n, **f), terminals=torch.empty(n, dtype=torch.uint8, device=dev))
    a = _lib.block(_lib.MobodyTaskCollect, p=p, lanes=int(lanes), split=int(split), L=int(L), time_limit=int(time_limit),
                   ctrl=(C.c_int32 * 2)(*[int(c) for c in ctrl]), ctrl_push=(C.c_float * 2)(*[float(x) for x in ctrl_push]),
                   ctrl_eps=(C.c_float * 2)(*[float(x) for x in ctrl_eps]), init_std=float(init_std), seed=seed, call0=call0 & 0xFFFFFFFF,
                   **{k: ptr(v) for k, v in out.items()})
    _run_with_workspace("mobody_task_collect", a, ws, dev)
    return out


def online_state(lanes, S, device):
    """The lanes' state and counters of mobody_task_interact, all zero: lane_obs [lanes, S], lane_t / lane_ep / done_count / len_sum
    int32 [lanes], lane_ret / ret_sum [lanes] and the interaction count word (int64 [1])."""
    f, i = dict(dtype=torch.float32, device=device), dict(dtype=torch.int32, device=device)
    return dict(lane_obs=torch.zeros(lanes, S, **f), lane_t=torch.zeros(lanes, **i), lane_ep=torch.zeros(lanes, **i),
                lane_ret=torch.zeros(lanes, **f), done_count=torch.zeros(lanes, **i), ret_sum=torch.zeros(lanes, **f),
                len_sum=torch.zeros(lanes, **i), count=torch.zeros(1, dtype=torch.int64, device=device))


def task_interact(p, policy_blob, head, ring, cap, ptr_size, state, time_limit, expl, init_std, seed, call0=0, ws=None,
                  policy_blob_T=None, precision=0):
    """One interaction of the policy with the task `p` on the lanes of `state` (online_state), recorded into `ring` (a RingView or
    the 5-tuple of ring tensors) of `cap` rows at the device words ptr_size (mobody_task_interact: 3 launches, no host read).
    Returns the workspace."""
    lanes = state["lane_obs"].shape[0]
    view = buffer_view(ring)
    a = _lib.block(_lib.MobodyTaskInteract, precision=prec_id(precision), p=p, policy_blob=ptr(policy_blob), policy_blob_T=ptr(policy_blob_T),
                   lanes=lanes, cap=int(cap), head=int(head), time_limit=int(time_limit), expl=float(expl), init_std=float(init_std),
                   seed=seed, call0=call0 & 0xFFFFFFFF, ring=C.pointer(view), ptr_size=ptr(ptr_size),
                   **{k: ptr(v) for k, v in state.items()})
    return _run_with_workspace("mobody_task_interact", a, ws, state["lane_obs"].device)
