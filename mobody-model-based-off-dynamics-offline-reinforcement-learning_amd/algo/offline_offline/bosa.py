"""BOSA baseline, VAE stage -- host-side mirror of the reference's `algo/offline_offline/bosa.py` (class BOSA), written from the
algorithm.

BOSA trains in two stages (bosa.py:552-639).  While `total_it < vae_iteration` a train() call only fits two VAEs on the mixed
batch [tar(bs) | src(bs)]: a behaviour VAE over actions (`vae_policy`, VAE_Policy :23-133) and an ensemble dynamics VAE over next
states (`vae_dyna`, VAE_Dynamics_Ensemble :203-327).  Afterwards a TD3-style critic / actor is trained, the critic masked by the
dynamics VAE's importance-sampled log-likelihood and the actor regularised by the policy VAE's.  Without further keys this class
builds the first stage -- the VAE steps, their checkpoints and both likelihood estimators -- and a train() call that would enter the
second stage raises NotImplementedError before it changes any state.  With config['critic_actor'] truthy the second
stage is built too: the twin-Q critic with the masked conservative seed (`mobody_bosa_critic`), the delayed actor step through
critic_1 alone with the derivative of the policy VAE's estimator (`mobody_bosa_actor_forward / _backward`,
`mobody_bosa_loglik_grad`), the three target nets, the reference's ten checkpoint files plus the targets', and `critic_actor_train`
beside `vae_models_train`.  Stage-2 calls run eagerly whatever config['graph'] says (it only replays the VAE stage); with
config['critic_actor_graph'] = 1 they run through the library's row-wise entries alone -- no torch op between the
launches -- and replay as two HIP graphs, one for critic calls and one for actor calls, their counts in device words.

Same plugin surface as the reference: `BOSA(config, device)`, `.train(src_rb, tar_rb, batch_size, writer, wandbrun)` (the
reference's takes four arguments and its driver passes five), `.vae_policy .vae_dyna .vae_policy_optimizer .vae_dyna_optimizer`,
`.vae_policy_train(batch) .vae_dyna_train(batch) .vae_models_train(batch)`, `.select_action(state, test)`, `.save/.load(prefix)`.

Both VAEs are 750 wide in the reference's configs, so they run on the wide-MLP kernels (csrc/wide.hip, csrc/bosa.hip),
in exact fp32 whatever MOBODY_MFMA / config['mfma'] says: the split-precision planes exist for 256-wide layers only.  With
rng='device' and no logging step a whole train() call -- the gather of both buffers, the policy-VAE step, the dynamics-VAE step --
replays as one HIP graph; the noise call ids and both Adam step counts then live in device words.

Where the reference is odd: `vae_models_train` increments `total_it` a second time, so the VAE stage lasts
`vae_iteration // 2` train() calls (`vae_steps`); `elbo_policy_loss`, `elbo_dyna_loss`, `iwae_*_loss` and `lamda_dyna` are never
used by train() and are not built; EnsembleFC's unit-variance initial weights saturate the `log_std` clamp of an untrained 750-wide
dynamics VAE (kept); `log(epsilon_dyna_exp)` masks every row until the dynamics VAE is well trained (kept).
"""
import math
import os
import warnings

import numpy as np
import torch

from ... import _lib, dp, ops, packing
from .mobody import REFRESH_EVERY, _Adam, _PackedNet, evaluate_in_model, evaluate_in_task, refuse_missing_keys

_KEYS = ("vae_policy_lr", "vae_policy_hidden_dim", "vae_policy_beta", "vae_dyna_lr", "vae_dyna_ensemble", "vae_dyna_hidden_dim",
         "vae_dyna_beta", "vae_iteration", "lamda_policy", "lamda_dyna", "epsilon_policy_exp", "epsilon_dyna_exp", "conservation_coef",
         "num_samples", "noise_clip", "expl_noise", "update_interval")
LOG_KEYS = ("VAE_Policy/reconstruction_loss", "VAE_Policy/KL_loss", "VAE_Policy/vae_loss", "VAE_Dynamics/reconstruction_loss",
            "VAE_Dynamics/KL_loss", "VAE_Dynamics/vae_loss")
SEED_POLICY, SEED_DYNA = 108, 109          # seed ids of the two VAEs' noise streams (101-107 are index streams)
SEED_TARGET = 110                          # seed id of the second stage's target-noise stream (rng='device')
STAGE2_KEYS = ("gamma", "tau", "actor_lr", "critic_lr")      # what config['critic_actor'] additionally requires
STAGE2_LOG_KEYS = ("critic_mask_ratio", "critic_loss", "critic_td_loss", "critic_cons_loss", "actor_loss", "neg_log_beta_mean",
                   "neg_log_beta_max", "lamda_policy")       # bosa.py:591-627, the order of the device words
STAGE2_FILES = ("_critic_1", "_critic_1_optimizer", "_critic_2", "__critic_2_optimizer", "_actor", "_actor_optimizer")   # bosa.py:646-651
TARGET_FILES = ("_actor_target", "_critic_1_target", "_critic_2_target")


def vae_steps(vae_iteration):
    """train() calls the VAE stage lasts: a call enters it while the once-incremented total_it is below vae_iteration and then
    increments total_it again (bosa.py:509, :553, :560), so total_it is 2, 4, 6, ... after the calls."""
    return max(int(vae_iteration), 0) // 2


def _check_config(config):
    missing = [k for k in _KEYS if k not in config]
    if missing:
        raise NotImplementedError(f"BOSA is built from a BOSA config only: config lacks {missing} (the reference's "
                                  "config/*/bosa/*.yaml values are read without defaults; none are substituted here)")
    for k in ("vae_policy_hidden_dim", "vae_dyna_hidden_dim"):
        if not 8 <= int(config[k]) <= 1024:
            raise ValueError(f"config['{k}'] = {config[k]} outside 8..1024")
    if not 1 <= int(config["vae_dyna_ensemble"]) <= 8:
        raise ValueError(f"config['vae_dyna_ensemble'] = {config['vae_dyna_ensemble']} outside 1..8")
    if not 1 <= int(config["num_samples"]) <= 64:
        raise ValueError(f"config['num_samples'] = {config['num_samples']} outside 1..64")
    for k in ("vae_policy_beta", "vae_dyna_beta", "epsilon_policy_exp", "epsilon_dyna_exp"):
        if not float(config[k]) > 0.0:
            raise ValueError(f"config['{k}'] = {config[k]} must be positive")
    if int(config["vae_iteration"]) < 0:
        raise ValueError(f"config['vae_iteration'] = {config['vae_iteration']} < 0")
    g = config.get("critic_actor_graph", 0)                 # read with config['critic_actor'] only, as the stage's other keys
    if config.get("critic_actor") and (isinstance(g, bool) or g not in (0, 1)):
        raise ValueError(f"config['critic_actor_graph'] = {g!r}: expected 0 (stage-2 calls run eagerly) or 1 (they replay as HIP graphs)")


class _WideVae(object):
    """nn.Module-like handle on one VAE: two wide nets in ONE blob (encoder | decoder), the gradient in the same layout."""

    def __init__(self, kind, S, A, hidden, members, beta, max_action, device):
        self.kind, self.S, self.A, self.hidden, self.beta = kind, int(S), int(A), int(hidden), float(beta)
        self.ensemble_size = 1 if kind == "policy" else int(members)
        self.latent_dim = 2 * self.A if kind == "policy" else 2 * self.S
        self.max_action, self.device = float(max_action), device
        Lz, E = self.latent_dim, self.ensemble_size
        if kind == "policy":
            self.enc_layout, self.dec_layout = _lib.wide_layout(S + A, hidden, 2 * Lz, 1), _lib.wide_layout(S + Lz, hidden, A, 1)
        else:
            self.enc_layout, self.dec_layout = _lib.wide_layout(2 * S + A, hidden, 2 * Lz, E), _lib.wide_layout(S + A + Lz, hidden, S, E)
        self.n_enc = self.enc_layout.total_floats
        self.blob = torch.zeros(self.n_enc + self.dec_layout.total_floats, dtype=torch.float32, device=device)
        self.grad = torch.zeros_like(self.blob)
        self._pack = packing.pack_bosa_vae_policy if kind == "policy" else packing.pack_bosa_vae_dynamics
        self.blob.copy_(torch.cat(self._pack(self._initial(), device)))
        self.version = 1

    def _initial(self):
        S, A, H, Lz, E = self.S, self.A, self.hidden, self.latent_dim, self.ensemble_size
        sd = {}
        if self.kind == "policy":                                       # nn.Linear's default (bosa.py:38-55)
            for k, (i, o) in (("encoder_shared.0", (S + A, H)), ("encoder_shared.2", (H, H)), ("mean", (H, Lz)), ("log_std", (H, Lz)),
                              ("decoder.0", (S + Lz, H)), ("decoder.2", (H, H)), ("decoder.4", (H, A))):
                bound = 1.0 / np.sqrt(i)
                sd[k + ".weight"], sd[k + ".bias"] = torch.empty(o, i).uniform_(-bound, bound), torch.empty(o).uniform_(-bound, bound)
        else:                                                           # EnsembleFC: fmod(randn, 2), zero bias (bosa.py:188-196)
            for k, (i, o) in (("encoder_shared.0", (2 * S + A, H)), ("encoder_shared.2", (H, H)), ("mean", (H, Lz)), ("log_std", (H, Lz)),
                              ("decoder.0", (S + A + Lz, H)), ("decoder.2", (H, H)), ("decoder.4", (H, S))):
                sd[k + ".W"], sd[k + ".b"] = torch.fmod(torch.randn(E, i, o), 2), torch.zeros(E, 1, o)
        return sd

    def state_dict(self):
        enc, dec = self.blob[:self.n_enc], self.blob[self.n_enc:]
        if self.kind == "policy":
            return packing.unpack_bosa_vae_policy(enc, dec, self.S, self.A, self.hidden)
        return packing.unpack_bosa_vae_dynamics(enc, dec, self.S, self.A, self.hidden, self.ensemble_size)

    def pack(self, sd):
        """A dict with this VAE's keys and shapes -> one tensor in blob layout (encoder | decoder)."""
        want = {k: tuple(v.shape) for k, v in self.state_dict().items()}
        got = {k: tuple(torch.as_tensor(v).shape) for k, v in sd.items()}
        if got != want:
            raise ValueError(f"{self.kind} VAE: state_dict keys / shapes {got} do not match {want}")
        return torch.cat(self._pack(sd, self.device))

    def load_state_dict(self, sd):
        self.blob.copy_(self.pack(sd))                                   # in place: captured graphs and Adam hold the pointer
        self.version += 1

    def parameters(self):
        return list(self.state_dict().values())

    def block(self, B, num_samples=0, **fields):
        return ops.bosa_block(self.kind, self.S, self.A, self.hidden, self.ensemble_size, B, self.beta, self.max_action, num_samples,
                              blob=self.blob, **fields)


class _WideAdam(object):
    """torch.optim.Adam(vae.parameters(), lr) (bosa.py:406, :414): one optimizer over the VAE's 14 parameters, one step count;
    state_dict in torch's format, parameters in the module's order."""

    def __init__(self, vae, lr):
        self.vae, self.lr, self.t = vae, float(lr), 0
        self.m, self.v = torch.zeros_like(vae.blob), torch.zeros_like(vae.blob)

    def _unpack(self, blob):
        v = self.vae
        enc, dec = blob[:v.n_enc], blob[v.n_enc:]
        if v.kind == "policy":
            return list(packing.unpack_bosa_vae_policy(enc, dec, v.S, v.A, v.hidden).values())
        return list(packing.unpack_bosa_vae_dynamics(enc, dec, v.S, v.A, v.hidden, v.ensemble_size).values())

    def state_dict(self):
        ms, vs = self._unpack(self.m), self._unpack(self.v)
        state = {i: dict(step=torch.tensor(float(self.t)), exp_avg=ms[i], exp_avg_sq=vs[i]) for i in range(len(ms))} if self.t else {}
        group = dict(lr=self.lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, params=list(range(len(ms))))
        return dict(state=state, param_groups=[group])

    def load_state_dict(self, sd):
        st = sd["state"]
        self.lr = float(sd["param_groups"][0]["lr"])
        if not st:
            self.t = 0
            self.m.zero_(); self.v.zero_()
            return
        keys = list(self.vae.state_dict())
        if sorted(st) != list(range(len(keys))):
            raise ValueError(f"{self.vae.kind} VAE optimizer: expected the state of {len(keys)} parameters, got {sorted(st)}")
        for name, dst in (("exp_avg", self.m), ("exp_avg_sq", self.v)):
            dst.copy_(self.vae.pack({k: st[i][name] for i, k in enumerate(keys)}))
        self.t = int(float(st[0]["step"]))


class _Member(object):
    """critic_1 / critic_2 (Critic, bosa.py:351-366) as views of one member of the packed twin-Q net: state_dict in the reference
    module's layout, `net.{0,2,4}.{weight,bias}`."""

    def __init__(self, net, member):
        self.net, self.member = net, member

    def state_dict(self):
        pre = self.net.prefixes[self.member]
        return {k[len(pre):].replace("network.", "net."): v for k, v in self.net.state_dict().items() if k.startswith(pre)}

    def parameters(self):
        return list(self.state_dict().values())


def _merge_members(net, sds):
    """One state dict per member in the reference's layout -> what net.load_state_dict reads."""
    return {pre + k.replace("net.", "network."): v for pre, sd in zip(net.prefixes, sds) for k, v in sd.items()}


class BOSA(object):
    third_loss_name = "vae_dyna_loss"

    def __init__(self, config, device):
        # 1. the keys the reference reads without defaults: a config without them is not a BOSA run (the refusal has the type the
        #    registry gave for 'bosa' before this class existed).  2. ranges.  3. data parallel.  4. the device.
        _check_config(config)
        d = torch.distributed
        if d.is_available() and d.is_initialized() and d.get_world_size() > 1:
            raise NotImplementedError("data-parallel BOSA is not built: run 'bosa' on one GPU (only 'mobody' has the exchange "
                                      "protocol of mobody_amd.dp wired through the CLI)")
        self.config = config
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BOSA (MI355X build) needs a GPU device; there is no CPU fallback")
        if config.get("critic_actor"):                            # 5. the second stage's own keys, before anything is built
            refuse_missing_keys("BOSA", [k for k in STAGE2_KEYS if k not in config], "config/*/bosa/*.yaml values")
        S, A = int(config["state_dim"]), int(config["action_dim"])
        self.S, self.A, self.max_action = S, A, float(config["max_action"])
        self.discount, self.tau = config.get("gamma"), config.get("tau")
        self.update_interval = config["update_interval"]
        self.vae_iteration = int(config["vae_iteration"])
        self.vae_policy_beta, self.vae_dyna_beta = float(config["vae_policy_beta"]), float(config["vae_dyna_beta"])
        self.lamda_policy, self.lamda_dyna = config["lamda_policy"], config["lamda_dyna"]
        self.epsilon_policy_exp, self.epsilon_dyna_exp = float(config["epsilon_policy_exp"]), float(config["epsilon_dyna_exp"])
        self.conservation_coef, self.num_samples = config["conservation_coef"], int(config["num_samples"])
        self.noise_clip, self.expl_noise = config["noise_clip"], config["expl_noise"]
        self.rng, self.seed = config.get("rng", "numpy"), int(config.get("seed", 0))
        self.use_graph = int(config.get("graph", 0))
        self.vae_policy = _WideVae("policy", S, A, config["vae_policy_hidden_dim"], 1, self.vae_policy_beta, self.max_action, self.device)
        self.vae_policy_optimizer = _WideAdam(self.vae_policy, config["vae_policy_lr"])
        self.vae_dyna = _WideVae("dynamics", S, A, config["vae_dyna_hidden_dim"], config["vae_dyna_ensemble"], self.vae_dyna_beta, 1.0,
                                 self.device)
        self.vae_dyna_optimizer = _WideAdam(self.vae_dyna, config["vae_dyna_lr"])
        # the TD3 actor of the second stage (Actor, bosa.py:330-349): untrained here, select_action works
        self.actor = _PackedNet(S, A, 1, ("",), self.device, out_mode=1, max_action=self.max_action, precision=ops.prec_id(ops.default_mfma()))
        self.dynamics = None
        self.total_it = 0
        self._noise_calls = 0                                     # VAE noise draws done (rng='device': the streams' call id)
        self._loss = torch.zeros(6, dtype=torch.float32, device=self.device)         # LOG_KEYS order
        self._ctr = torch.zeros(3, dtype=torch.int64, device=self.device)            # [replays since capture, policy t, dyna t]
        self._batch, self._batch_key, self._ws = None, None, {}
        self._graph, self._graph_key, self._graph_base = None, None, None
        self.noise_fn = None          # optional hook (tests): (kind, shape) -> fp32 array of that shape, the VAE's latent noise
        self._synced = True
        self.critic_actor = bool(config.get("critic_actor"))
        self._in_stage2 = False                                   # the last train() call was a stage-2 call
        if self.critic_actor:
            self._init_stage2(config)

    def _init_stage2(self, config):
        """Actor (bosa.py:420), critic_1 / critic_2 (:423-426) as the two members of one packed twin-Q net with ONE Adam over both
        (the reference steps its two optimizers together, always: the same updates), and the three targets (:429-431)."""
        S, A, dev = self.S, self.A, self.device
        self.precision = self.actor.precision
        if self.precision in (1, 2):
            raise ValueError(f"BOSA's critic / actor stage runs at mfma 'f32', 'bf16x3' or 'f16x2', not {ops.default_mfma()!r}")
        self.tau = float(config["tau"])
        self.f16_guard = ops.check_f16_guard(config.get("f16_guard", "raise"))
        if self.f16_guard != "off":
            with torch.cuda.device(dev):
                self._health = ops.health_block(dev)
        self.critic = _PackedNet(S + A, 1, 2, ("network1.", "network2."), dev, precision=self.precision)
        self.critic_1, self.critic_2 = _Member(self.critic, 0), _Member(self.critic, 1)
        self.critic_optimizer = _Adam(self.critic, config["critic_lr"])
        self.actor_optimizer = _Adam(self.actor, config["actor_lr"])
        self.actor_target, self.critic_target = self.actor.clone().eval(), self.critic.clone().eval()
        self.critic_1_target, self.critic_2_target = _Member(self.critic_target, 0), _Member(self.critic_target, 1)
        self._hyp = _lib.MobodyHyper(float(config["gamma"]), self.tau, self.max_action, 1.0, 0.0, 0, 1, self.precision)
        self._s2 = torch.zeros(8, dtype=torch.float32, device=dev)          # STAGE2_LOG_KEYS order
        self._s2[7] = float(self.lamda_policy)
        self._closs, self._aloss = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
        self._stats = torch.zeros(2, dtype=torch.float32, device=dev)
        self._s2_key, self._s2_buf = None, None
        # config['critic_actor_graph']: the stage's calls through the library's row-wise entries alone, replayed as two
        # HIP graphs.  The device words: [next noise call id, critic step, actor step, next draw id of the target buffer].
        self.critic_actor_graph = int(config.get("critic_actor_graph", 0))
        self._s2_ctr = torch.zeros(4, dtype=torch.int64, device=dev)
        self._s2_ctr_host = None                                  # what the words hold, as far as the host knows
        self._s2_graphs, self._s2_graph_key, self._s2_warm, self._s2_capture_failed = {}, None, {}, False
        self.stage2_replays, self.stage2_captures = 0, {"critic": 0, "actor": 0}

    # ------------------------------------------------------------------ acting
    def select_action(self, state, test=False):
        """bosa.py:431-434."""
        x = state if isinstance(state, torch.Tensor) else torch.as_tensor(np.asarray(state), dtype=torch.float32)
        return self.actor(x.reshape(1, -1).to(self.device)).squeeze().cpu().numpy()

    def eval_policy(self):
        """(net, head) for fitted Q evaluation: the TD3 actor, head 0."""
        return self.actor, 0

    evaluate_in_model = evaluate_in_model          # the six classes' one method (mobody.py)
    evaluate_in_task = evaluate_in_task

    def _seed_for(self, k):
        return (self.seed + k + dp.rank_salt()) & 0xFFFFFFFF

    def _health_check(self):
        """The wide nets run in exact fp32 and report no f16 range faults; a non-finite parameter is reported here (a device
        sync: called on logging steps, in save() and at the end of the CLI's run, never per step)."""
        for name, v in (("vae_policy", self.vae_policy), ("vae_dyna", self.vae_dyna)):
            if not bool(torch.isfinite(v.blob).all()):
                raise FloatingPointError(f"{name}: non-finite parameters after {self.total_it} counts of total_it")
        if self.critic_actor:
            self._health_check_stage2()

    def _health_check_stage2(self):
        """The device health words, as TD3BC reads them: an f16x2 weight-range fault or a non-finite optimizer result of the actor
        or critic has frozen every optimizer launch since.  'raise' reports it; 'fallback' moves an F16_RANGE fault to bf16x3 --
        T blobs and planes of all four packed nets again from the intact fp32 weights -- and goes on (the host step counts are
        not rewound: the frozen steps stay counted)."""
        words = ops.health_bound(self.device)
        if words is None:
            return
        mask, step = ops.health_read(words)
        if mask == 0:
            return
        nets = (("actor", self.actor), ("critic", self.critic), ("actor_target", self.actor_target), ("critic_target", self.critic_target))
        found = []
        for name, n in nets:
            m = float(ops._mlp_w2(n.blob, n.layout, n.members).abs().max())
            if (n.precision == 4 and not (m < ops.F16_W_LIMIT)) or not bool(torch.isfinite(n.blob).all()):
                found.append(f"{name} (max |W2| = {m:g})")
        msg = (f"device health word {'|'.join(ops.health_bits(mask))}" + (f" at Adam step {step}" if step else "") + ": " +
               (", ".join(found) or "no net of this object (another object on this device)") + "; the optimizer steps since were "
               f"frozen.  f16x2 planes hold |w| < {ops.F16_W_LIMIT}: use MOBODY_MFMA=bf16x3 (or f16_guard='fallback')")
        if self.f16_guard == "fallback" and mask == _lib.HEALTH_F16_RANGE and found:
            warnings.warn("falling back to mfma 'bf16x3': " + msg)
            self.precision = self._hyp.precision = ops.prec_id("bf16x3")
            for _, n in nets:
                n.precision = self.precision
                ops.mlp_transpose(n.blob, n.in_dim, n.out_dim, n.members, out=n.blob_T, precision=self.precision)
                n.version += 1
            ops.health_clear()
            return
        raise FloatingPointError(msg)

    # ------------------------------------------------------------------ the VAE steps (bosa.py:507-550)
    def _workspace(self, vae, B, num_samples=0):
        key = (vae.kind, B, num_samples)
        if key not in self._ws:
            self._ws[key] = ops.bosa_workspace(vae.block(B, num_samples), self.device)
        return self._ws[key]

    def _vae_step(self, vae, opt, b, loss, dev=False):
        """One training step of `vae` on the staged batch b.  dev: the captured form -- noise call id and step count in device words."""
        B = b[0].shape[0]
        sid = SEED_POLICY if vae.kind == "policy" else SEED_DYNA
        eps = None
        if self.noise_fn is not None:
            eps = torch.as_tensor(self.noise_fn(vae.kind, (vae.ensemble_size, B, vae.latent_dim)), dtype=torch.float32).to(self.device).contiguous()
        elif self.rng != "device":                     # the reference's torch.randn_like(std), from torch's generator
            eps = torch.randn(vae.ensemble_size, B, vae.latent_dim, device=self.device)
        if not dev:
            opt.t += 1
        call, t_dev, call_dev = self._noise_calls, None, None
        if dev:
            base = self._graph_base
            call, t_dev, call_dev = base["noise"] + 1, self._ctr[1:2] if vae.kind == "policy" else self._ctr[2:3], self._ctr[0:1]
        blk = vae.block(B, state=b[0], action=b[1], next_state=b[2], eps=eps, seed=self._seed_for(sid), call=call, call_dev=call_dev,
                        grad=vae.grad, m=opt.m, v=opt.v, t=opt.t, t_dev=t_dev, lr=opt.lr, loss_out=loss, workspace=self._workspace(vae, B))
        self._keep = (eps,)
        ops.bosa_vae(blk)

    @staticmethod
    def _as_batch(batch, device):
        return tuple(torch.as_tensor(t, dtype=torch.float32).to(device).contiguous() for t in batch[:3])

    def _log_dict(self, lo, hi):
        return dict(zip(LOG_KEYS[lo:hi], [float(x) for x in self._loss[lo:hi].tolist()]))

    def vae_policy_train(self, batch):
        """bosa.py:516-532 on (state, action, ...); returns the reference's log dict (a device read)."""
        self._noise_calls += 1
        self._vae_step(self.vae_policy, self.vae_policy_optimizer, self._as_batch(batch, self.device), self._loss[0:3])
        return self._log_dict(0, 3)

    def vae_dyna_train(self, batch):
        """bosa.py:534-550."""
        self._noise_calls += 1
        self._vae_step(self.vae_dyna, self.vae_dyna_optimizer, self._as_batch(batch, self.device), self._loss[3:6])
        return self._log_dict(3, 6)

    def vae_models_train(self, batch):
        """bosa.py:507-514: counts total_it once more, then both VAE steps."""
        self.total_it += 1
        self._graph = None
        log = self.vae_policy_train(batch)
        log.update(self.vae_dyna_train(batch))
        return log

    # ------------------------------------------------------------------ the estimators (bosa.py:72-105, :257-298, :584-591)
    def _loglik(self, vae, state, action, next_state, num_samples, log_eps=0.0, mask=False):
        n = self.num_samples if num_samples is None else int(num_samples)
        if not 1 <= n <= 64:
            raise ValueError(f"num_samples = {n} outside 1..64")
        b = self._as_batch((state, action, next_state if next_state is not None else state), self.device)
        B, E = b[0].shape[0], vae.ensemble_size
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
        out = dict(ll=new(E, B))
        if mask:
            out.update(min_ll=new(B), mask=new(B), mask_mean=new(1))
        eps, policy = None, vae.kind == "policy"
        shape = (B, n, vae.latent_dim) if policy else (n, E, B, vae.latent_dim)
        if self.noise_fn is not None:
            eps = torch.as_tensor(self.noise_fn(vae.kind + "_ll", shape), dtype=torch.float32).to(self.device).contiguous()
        elif self.rng != "device":
            eps = torch.randn(*shape, device=self.device)
        self._noise_calls += 1
        self._graph = None                                          # a captured step's call ids continue from the host's counts
        ops.bosa_loglik(vae.block(B, n, state=b[0], action=b[1], next_state=b[2], eps=eps, seed=self._seed_for(SEED_POLICY if policy else SEED_DYNA),
                                  call=self._noise_calls, log_eps=float(log_eps), workspace=self._workspace(vae, B, n), **out))
        return out

    def policy_log_likelihood(self, state, action, num_samples=None):
        """VAE_Policy.importance_sampling_estimator(state, action, vae_policy_beta, num_samples) -> [B]."""
        return self._loglik(self.vae_policy, state, action, None, num_samples)["ll"][0]

    def dyna_log_likelihood(self, state, action, next_state, num_samples=None):
        """VAE_Dynamics_Ensemble.importance_sampling_estimator(...) -> [E, B]."""
        return self._loglik(self.vae_dyna, state, action, next_state, num_samples)["ll"]

    def dyna_mask(self, state, action, next_state):
        """The critic's mask (bosa.py:584-591): (min over members of the log-likelihood > log(epsilon_dyna_exp)) as 0 / 1 floats,
        and its mean (`critic_mask_ratio`, a device scalar)."""
        out = self._loglik(self.vae_dyna, state, action, next_state, None, log_eps=math.log(self.epsilon_dyna_exp), mask=True)
        return out["mask"], out["mask_mean"][0]

    # ------------------------------------------------------------------ training (bosa.py:552-639)
    def _gather(self, src, tar, bs):
        """Rows [tar(bs) | src(bs)] (bosa.py:557-558); the index draws in the reference's order, src first."""
        if self.rng == "device":
            for rb in (src, tar):
                if rb.size <= 0:
                    raise ValueError("low >= high")
                rb._draws += 1
            salt = dp.rank_salt()
            ops.gather_batch_rng([tar._fields(), src._fields()], [bs, bs], [(rb.seed + salt) & 0xFFFFFFFF for rb in (tar, src)],
                                 [tar._draws, src._draws], None, [tar.ptr_size[1:2], src.ptr_size[1:2]], self.S, self.A, self._batch)
        else:
            i_src = src.draw_indices(bs)
            i_tar = tar.draw_indices(bs)
            ops.gather_batch([tar._fields(), src._fields()], [i_tar, i_src], self.S, self.A, out=self._batch)

    def _graph_step(self, src, tar, bs):
        """Replay (capturing first) one VAE-stage call: both gathers, the policy-VAE step, the dynamics-VAE step."""
        po, do = self.vae_policy_optimizer, self.vae_dyna_optimizer
        key = (bs, id(src), id(tar), src.state.data_ptr(), tar.state.data_ptr(), tuple(t.data_ptr() for t in self._batch),
               self.vae_policy.blob.data_ptr(), self.vae_dyna.blob.data_ptr(), po.m.data_ptr(), do.m.data_ptr())
        base = self._graph_base
        if self._graph is not None and (tar._draws, src._draws) != (base["tar"] + base["replays"], base["src"] + base["replays"]):
            self._graph = None                                      # somebody else drew from a buffer: re-seed the call ids
        if self._graph is None or self._graph_key != key:
            torch.cuda.synchronize()
            self._ctr.copy_(torch.tensor([0, po.t, do.t], dtype=torch.int64))
            self._graph_base = dict(noise=self._noise_calls, tar=tar._draws, src=src._draws, replays=0)
            base, c, salt = self._graph_base, self._ctr, dp.rank_salt()
            self._workspace(self.vae_policy, 2 * bs), self._workspace(self.vae_dyna, 2 * bs)     # sized outside the capture

            def step():
                # call ids: base + 1 + replays done (c[0]); the gather advances both Adam step counts (it does not read them),
                # the last launch advances c[0]
                ops.gather_batch_rng([tar._fields(), src._fields()], [bs, bs], [(rb.seed + salt) & 0xFFFFFFFF for rb in (tar, src)],
                                     [base["tar"] + 1, base["src"] + 1], c[0:1], [tar.ptr_size[1:2], src.ptr_size[1:2]], self.S, self.A,
                                     self._batch, bump=(c[1:2], c[2:3]))
                self._vae_step(self.vae_policy, po, self._batch, self._loss[0:3], dev=True)
                self._vae_step(self.vae_dyna, do, self._batch, self._loss[3:6], dev=True)
                ops.counter_add(c[0:1], 1)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    step()
            except Exception as exc:
                import warnings
                torch.cuda.synchronize()
                warnings.warn(f"HIP-graph capture of the VAE-stage step failed ({exc!r}); continuing eagerly")
                self.use_graph, self._graph = 0, None
                return False
            self._graph, self._graph_key = g, key
        self._graph.replay()
        self._graph_base["replays"] += 1
        tar._draws += 1
        src._draws += 1
        self._noise_calls += 1
        po.t += 1
        do.t += 1
        return True

    def train(self, src_replay_buffer, tar_replay_buffer, batch_size=128, writer=None, wandbrun=None):
        """One call of the reference's train() (bosa.py:552-639).  total_it += 1; fewer than batch_size rows in either buffer: return;
        draw src(bs) then tar(bs); total_it < vae_iteration: both VAE steps, and total_it += 1 once more.  Otherwise the call belongs to
        the critic / actor stage: with config['critic_actor'] the gather plus critic_actor_train (eager whatever config['graph']
        says; replayed under config['critic_actor_graph']), without it NotImplementedError before anything changes."""
        bs = int(batch_size)
        short = src_replay_buffer.size < bs or tar_replay_buffer.size < bs
        if self.critic_actor and not short and not self.total_it + 1 < self.vae_iteration:
            return self._train_stage2(src_replay_buffer, tar_replay_buffer, bs, writer)
        if not short and not self.total_it + 1 < self.vae_iteration:
            raise NotImplementedError(f"BOSA's critic / actor stage is not built: this call would leave the VAE stage (total_it "
                                      f"{self.total_it}, vae_iteration {self.vae_iteration}: {vae_steps(self.vae_iteration)} train() "
                                      "calls); nothing was changed")
        self.total_it += 1
        if short:
            return
        self._in_stage2 = False
        self.total_it += 1                                          # vae_models_train's own count (bosa.py:509)
        log5k = writer is not None and self.total_it % 5000 == 0
        N = 2 * bs
        want = self.use_graph == 1 or (self.use_graph == 2 and N < 4096)
        if (want and self.rng == "device" and self.noise_fn is None and not log5k and self._batch_key == (N,)
                and self._graph_step(src_replay_buffer, tar_replay_buffer, bs)):
            return
        self._graph = None                                          # an eager step moves the host-side counts
        if self._batch_key != (N,):
            dev = self.device
            self._batch = tuple(torch.empty(N, w, device=dev) for w in (self.S, self.A, self.S, 1, 1))
            self._batch_key = (N,)
        self._gather(src_replay_buffer, tar_replay_buffer, bs)
        self._noise_calls += 1                                      # one call id for both VAEs' streams
        self._vae_step(self.vae_policy, self.vae_policy_optimizer, self._batch, self._loss[0:3])
        self._vae_step(self.vae_dyna, self.vae_dyna_optimizer, self._batch, self._loss[3:6])
        if log5k:                                                   # bosa.py:636-639
            self._health_check()
            for k, v in self._log_dict(0, 6).items():
                writer.add_scalar(f"train/{k}", v, self.total_it)

    # ------------------------------------------------------------------ the critic / actor stage (bosa.py:565-634)
    def _stage2_buffers(self, N):
        if self._s2_key != N:
            dev, f = self.device, lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
            bs = N - N // 2
            c = torch.zeros(N, dtype=torch.float32, device=dev)
            c[N // 2:] = float(self.conservation_coef) / bs        # the seed's constant on the source rows (:597-598)
            dims = ops.train_dims(self.S, self.A, N, N)
            blk = self.vae_policy.block(N, self.num_samples)
            self._s2_buf = dict(dims=dims, ws=ops.train_workspace(dims, dev), c=c, w=f(N), pi=f(N, self.A), dll=f(N, self.A), dpi=f(N, self.A),
                                ll=f(1, N), gws=ops.bosa_loglik_grad_workspace(blk, dev), bs=bs)
            if self.critic_actor_graph:                            # what the eager path lets torch allocate per call
                tb = _lib.block(_lib.MobodyBosaTarget, S=self.S, A=self.A, N=N)
                self._s2_buf.update(q_next=f(N), tws=ops.bosa_target_workspace(tb, dev), ll_d=f(self.vae_dyna.ensemble_size, N), min_ll=f(N),
                                    mask=f(N), mask_mean=f(1))
                self._workspace(self.vae_dyna, N, self.num_samples)
            self._s2_key = N
        return self._s2_buf

    def _noise(self, kind, shape, seed_id, stream):
        """Normal draws of the second stage: the test hook, torch's generator (the reference's), or -- rng='device' -- a device stream."""
        if self.noise_fn is not None:
            return torch.as_tensor(self.noise_fn(kind, shape), dtype=torch.float32).to(self.device).contiguous()
        if self.rng != "device":
            return torch.randn(*shape, device=self.device)
        self._noise_calls += 1
        n = int(np.prod(shape))
        return ops.rng_normal(self._seed_for(seed_id), _lib.BOSA_STREAMS[stream], self._noise_calls, n, self.device).reshape(shape)

    def critic_actor_train(self, batch_mix):
        """bosa.py:553, :565-634 on the mixed rows (state, action, next_state, reward, not_done), [tar(bs) | src(bs)]: counts total_it,
        the masked conservative critic step, and -- when total_it % update_interval == 0 -- the actor step and the three Polyak
        updates.  The eight logged scalars stay in device words (stage2_log() reads them).  Under rng other than 'device' the normal
        draws come in the reference's order: target noise, dynamics estimator, policy estimator."""
        self.total_it += 1
        self._in_stage2, self._graph = True, None
        b = tuple(torch.as_tensor(t, dtype=torch.float32).to(self.device).contiguous() for t in batch_mix[:5])
        s, a, s2 = b[0], b[1], b[2]
        b = (s, a, s2, b[3].reshape(-1, 1), b[4].reshape(-1, 1))
        N, S, A = s.shape[0], self.S, self.A
        z = self._stage2_buffers(N)
        q, qt, qo, ao = self.critic, self.critic_target, self.critic_optimizer, self.actor_optimizer
        actor_step = self.total_it % self.update_interval == 0
        if self.critic_actor_graph:                                  # the same step through the library's row-wise entries alone
            self._stage2_launches(b, z, actor_step, dev=False)
            self._s2_warm["actor" if actor_step else "critic"] = N
            return
        # target noise and the bootstrap value min Q_target(s', a') (:571-577)
        noise = self._noise("target", (N, A), SEED_TARGET, "target_noise")
        a2 = (self.actor_target(s2) + (noise * self.expl_noise).clamp(-self.noise_clip, self.noise_clip)).clamp(-self.max_action, self.max_action)
        q_next = ops.mlp3_forward(qt.blob, S + A, 1, 2, s2, a2, blob_T=qt.blob_T, precision=qt.precision).min(0)[0].reshape(N).contiguous()
        mask, ratio = self.dyna_mask(s, a, s2)                       # :583-591
        self._s2[0:1].copy_(ratio.reshape(1))
        torch.mul(mask, 0.5, out=z["w"])
        self._keep2 = (b, q_next, mask, noise)
        crit = (z["dims"], self._hyp, q.blob, q.blob_T, b, q_next, z["w"], z["c"], float(self.conservation_coef), z["bs"], self._closs, z["ws"])
        if actor_step:               # gradient form, then Adam with the Polyak update: the actor step reads only the online critic
            ops.bosa_critic(*crit, grad_q=qo.grad)
            qo.step(target=qt, tau=self.tau)
        else:
            qo.t += 1
            ops.bosa_critic(*crit, m=qo.m, v=qo.v, t=qo.t, lr=qo.lr)
        self._s2[1:2].copy_(self._closs[0:1])
        self._s2[3:4].copy_(self._closs[1:2])
        torch.sub(self._closs[0:1], self._closs[1:2] * float(self.conservation_coef), out=self._s2[2:3])
        if not actor_step:
            return
        act = self.actor
        ops.bosa_actor_forward(z["dims"], self._hyp, act.blob, q.blob, s, self._stats, z["pi"], z["ws"], actor_blob_T=act.blob_T, q_blob_T=q.blob_T)
        n, vae = self.num_samples, self.vae_policy
        eps = None
        if self.noise_fn is not None or self.rng != "device":
            eps = self._noise("policy_ll", (N, n, vae.latent_dim), SEED_POLICY, "policy_ll")
        else:
            self._noise_calls += 1
        blk = vae.block(N, n, state=s, action=z["pi"], eps=eps, seed=self._seed_for(SEED_POLICY), call=self._noise_calls, ll=z["ll"],
                        workspace=z["gws"])
        ops.bosa_loglik_grad(blk, z["dll"])
        torch.mul(z["dll"], -float(self.lamda_policy) / N, out=z["dpi"])           # d(lamda mean(-ll)) / d pi  (:615-620)
        ops.bosa_actor_backward(z["dims"], self._hyp, act.blob, act.blob_T, q.blob, q.blob_T, s, self._stats, z["dpi"], self._aloss, z["ws"],
                                grad_actor=ao.grad)
        ao.step(target=self.actor_target, tau=self.tau)
        self._keep2 += (eps,)
        nlb = -z["ll"][0]
        torch.mean(nlb, dim=0, keepdim=True, out=self._s2[5:6])
        torch.amax(nlb, dim=0, keepdim=True, out=self._s2[6:7])
        torch.add(self._aloss[0:1], self._s2[5:6] * float(self.lamda_policy), out=self._s2[4:5])

    # ------------------------------------------------------------------ the same stage without a torch op
    def _stage2_launches(self, b, z, actor_step, dev):
        """critic_actor_train's step as launches of the library alone: mobody_bosa_target, the dynamics estimator with its mask,
        mobody_bosa_stage2_rows / _words around the critic and the actor phase.  dev: the captured form -- the noise call ids and
        both step counts are read from self._s2_ctr, which the last launch advances; otherwise the host's counts, which this
        advances as critic_actor_train does.  Bit for bit the nets of the torch composition; the logged mean is summed in the
        kernel's order, not torch.mean's."""
        s, a, s2 = b[0], b[1], b[2]
        N, n, A, c = s.shape[0], self.num_samples, self.A, self._s2_ctr
        q, qt, qo, ao, act, vd, vp = self.critic, self.critic_target, self.critic_optimizer, self.actor_optimizer, self.actor, self.vae_dyna, self.vae_policy
        noise = eps_d = eps_p = None
        if self.noise_fn is not None or self.rng != "device":
            noise = self._noise("target", (N, A), SEED_TARGET, "target_noise")
            eps_d = self._noise("dynamics_ll", (n, vd.ensemble_size, N, vd.latent_dim), SEED_DYNA, "dynamics_ll")
        if dev:
            base, call_dev = 0, c[0:1]
        else:                        # the draws' call ids follow the host's count, as _noise / _loglik advance it
            base, call_dev = self._noise_calls + 1, None
            self._noise_calls += (3 if actor_step else 2) if noise is None else 1
        ops.bosa_target(ops.bosa_target_block(self.actor_target, qt, s2, z["q_next"], self.expl_noise, self.noise_clip, noise=noise,
                                              seed=self._seed_for(SEED_TARGET), call=base, call_dev=call_dev, ws=z["tws"]))
        ops.bosa_loglik(vd.block(N, n, state=s, action=a, next_state=s2, eps=eps_d, seed=self._seed_for(SEED_DYNA), call=base + 1, call_dev=call_dev,
                                 log_eps=float(math.log(self.epsilon_dyna_exp)), workspace=self._workspace(vd, N, n), ll=z["ll_d"],
                                 min_ll=z["min_ll"], mask=z["mask"], mask_mean=z["mask_mean"]))
        ops.bosa_stage2_rows(N, mask=z["mask"], row_weight=z["w"])
        self._keep2 = (b, z["q_next"], z["mask"], noise, eps_d)
        crit = (z["dims"], self._hyp, q.blob, q.blob_T, b, z["q_next"], z["w"], z["c"], float(self.conservation_coef), z["bs"], self._closs, z["ws"])
        if actor_step:
            ops.bosa_critic(*crit, grad_q=qo.grad)
            qo.step_dev(c[1:2], target=qt, tau=self.tau) if dev else qo.step(target=qt, tau=self.tau)
        elif dev:
            ops.bosa_critic(*crit, m=qo.m, v=qo.v, t_dev=c[1:2], lr=qo.lr)
        else:
            qo.t += 1
            ops.bosa_critic(*crit, m=qo.m, v=qo.v, t=qo.t, lr=qo.lr)
        words = dict(mask_mean=z["mask_mean"], closs=self._closs, cons_coef=float(self.conservation_coef))
        if dev:                      # the words of the NEXT call: 2 or 3 noise ids, one step per net stepped, one draw
            words.update(bump=c, bump_inc=(3 if actor_step else 2, 1, int(actor_step), 1))
        if not actor_step:
            ops.bosa_stage2_words(N, self._s2, **words)
            return
        ops.bosa_actor_forward(z["dims"], self._hyp, act.blob, q.blob, s, self._stats, z["pi"], z["ws"], actor_blob_T=act.blob_T, q_blob_T=q.blob_T)
        if noise is not None:
            eps_p = self._noise("policy_ll", (N, n, vp.latent_dim), SEED_POLICY, "policy_ll")
        ops.bosa_loglik_grad(vp.block(N, n, state=s, action=z["pi"], eps=eps_p, seed=self._seed_for(SEED_POLICY), call=base + 2, call_dev=call_dev,
                                      ll=z["ll"], workspace=z["gws"]), z["dll"])
        ops.bosa_stage2_rows(N, dll=z["dll"], dpi=z["dpi"], dpi_scale=-float(self.lamda_policy) / N, A=A)
        ops.bosa_actor_backward(z["dims"], self._hyp, act.blob, act.blob_T, q.blob, q.blob_T, s, self._stats, z["dpi"], self._aloss, z["ws"],
                                grad_actor=ao.grad)
        ao.step_dev(c[2:3], target=self.actor_target, tau=self.tau) if dev else ao.step(target=self.actor_target, tau=self.tau)
        self._keep2 += (eps_p,)
        ops.bosa_stage2_words(N, self._s2, ll=z["ll"], aloss=self._aloss, lamda=float(self.lamda_policy), **words)

    def _stage2_replay(self, src, tar, bs, actor_call):
        """Replay (capturing first) one stage-2 call: both gathers and _stage2_launches, as the critic graph or the actor graph.
        The graphs take every count from the device words, which are rewritten -- no recapture -- whenever the host's own counts
        have moved on without them (an eager call, an estimator call, load(), a draw by someone else); a changed batch size,
        pointer, precision or buffer drops both graphs."""
        N, z, qo, ao = 2 * bs, self._s2_buf, self.critic_optimizer, self.actor_optimizer
        for rb in (src, tar):
            if rb.size <= 0:
                raise ValueError("low >= high")
        nets = (self.actor, self.critic, self.actor_target, self.critic_target, self.vae_policy, self.vae_dyna)
        key = (bs, id(src), id(tar), src.state.data_ptr(), tar.state.data_ptr(), tuple(t.data_ptr() for t in self._batch), self.precision,
               tuple(n.blob.data_ptr() for n in nets), qo.m.data_ptr(), ao.m.data_ptr(), z["q_next"].data_ptr(), src._draws - tar._draws)
        if self._s2_graph_key != key:
            self._s2_graphs, self._s2_graph_key = {}, key
        want = [self._noise_calls + 1, qo.t + 1, ao.t + 1, tar._draws + 1]
        if self._s2_ctr_host != want:
            self._s2_ctr.copy_(torch.tensor(want, dtype=torch.int64))
            self._s2_ctr_host = want
        kind = "actor" if actor_call else "critic"
        g = self._s2_graphs.get(kind)
        if g is None:
            c, salt = self._s2_ctr, dp.rank_salt()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    ops.gather_batch_rng([tar._fields(), src._fields()], [bs, bs], [(rb.seed + salt) & 0xFFFFFFFF for rb in (tar, src)],
                                         [0, src._draws - tar._draws], c[3:4], [tar.ptr_size[1:2], src.ptr_size[1:2]], self.S, self.A, self._batch)
                    self._stage2_launches(self._batch, z, actor_call, dev=True)
            except Exception as exc:
                torch.cuda.synchronize()
                warnings.warn(f"HIP-graph capture of the critic / actor stage's {kind} call failed ({exc!r}); continuing eagerly")
                self._s2_graphs, self._s2_graph_key, self._s2_capture_failed = {}, None, True
                return False
            self._s2_graphs[kind] = g
            self.stage2_captures[kind] += 1
        g.replay()
        self.total_it += 1
        self._in_stage2, self._graph = True, None
        tar._draws += 1
        src._draws += 1
        self._noise_calls += 3 if actor_call else 2
        qo.t += 1
        ao.t += int(actor_call)
        self._s2_ctr_host = [self._noise_calls + 1, qo.t + 1, ao.t + 1, tar._draws + 1]
        self.stage2_replays += 1
        return True

    def stage2_log(self):
        """The reference's log_dict of the last stage-2 call (a device sync): the four critic scalars, and after an actor step the
        four actor scalars of the latest one."""
        x = [float(v) for v in self._s2.tolist()]
        return dict(zip(STAGE2_LOG_KEYS[:8 if self.actor_optimizer.t else 4], x))

    def _train_stage2(self, src, tar, bs, writer):
        N = 2 * bs
        log5k = writer is not None and (self.total_it + 1) % 5000 == 0
        health = self.total_it % REFRESH_EVERY == 0 or log5k
        actor_call = (self.total_it + 1) % self.update_interval == 0
        # config['critic_actor_graph']: the call replays unless it logs, is on the health cadence, or the buffers of this size -- and one
        # eager call of its kind on them, which makes every launch once outside a capture -- are not there yet
        if (self.critic_actor_graph == 1 and not self._s2_capture_failed and self.rng == "device" and self.noise_fn is None and not health
                and self._batch_key == (N,) and self._s2_key == N and self._s2_warm.get("actor" if actor_call else "critic") == N
                and self._stage2_replay(src, tar, bs, actor_call)):
            return
        if self._batch_key != (N,):
            self._batch = tuple(torch.empty(N, w, device=self.device) for w in (self.S, self.A, self.S, 1, 1))
            self._batch_key = (N,)
        if health:                                                  # TD3BC's cadence: every REFRESH_EVERY calls and on logging steps
            self._health_check()
        self._gather(src, tar, bs)
        self.critic_actor_train(self._batch)
        if log5k:                                                   # bosa.py:636-639: this call's log_dict
            log = self.stage2_log()
            for k in STAGE2_LOG_KEYS[:8 if actor_call else 4]:
                writer.add_scalar(f"train/{k}", log[k], self.total_it)

    def losses(self):
        """(policy-VAE loss, dynamics-VAE reconstruction loss, dynamics-VAE loss) of the last step (forces a device sync); after a
        stage-2 call (critic_loss, actor_loss, critic_td_loss)."""
        if self._in_stage2:
            x = self._s2.tolist()
            return float(x[1]), float(x[4]), float(x[2])
        x = self._loss.tolist()
        return float(x[2]), float(x[3]), float(x[5])

    def log_line(self):
        """The CLI's periodic line: the six VAE losses under their own names, or the second stage's scalars (a device sync)."""
        if self._in_stage2:
            return " ".join(f"{k} {v:.4f}" for k, v in self.stage2_log().items())
        return " ".join(f"{k} {v:.4f}" for k, v in self._log_dict(0, 6).items())

    def max_train_steps(self):
        """train() calls this build can run from a fresh object: the VAE stage's; with config['critic_actor'] there is no bound."""
        if self.critic_actor:
            return math.inf
        return vae_steps(self.vae_iteration)

    # ------------------------------------------------------------------ checkpoints (bosa.py:641-665)
    def save(self, filename):
        """The reference's four VAE files.  Its six critic / actor files belong to the second stage: written, with the three targets',
        under config['critic_actor'] only (_save_stage2)."""
        self._health_check()
        torch.save(self.vae_policy.state_dict(), filename + "_vae_policy")
        torch.save(self.vae_policy_optimizer.state_dict(), filename + "_vae_policy_optimizer")
        torch.save(self.vae_dyna.state_dict(), filename + "_vae_dynamics")
        torch.save(self.vae_dyna_optimizer.state_dict(), filename + "_vae_dynamics_optimizer")
        if self.critic_actor:
            self._save_stage2(filename)

    def _save_stage2(self, filename):
        """The reference's six critic / actor files under its names (bosa.py:646-651, `__critic_2_optimizer` with its two
        underscores), modules in its layout; the one Adam over both critics is written as its two halves.  And the three target nets,
        which the reference does not save: a resumed run continues bit for bit."""
        qs = self.critic_optimizer.state_dict()
        half = lambda lo: dict(state={k - lo: v for k, v in qs["state"].items() if lo <= k < lo + 6},
                               param_groups=[dict(qs["param_groups"][0], params=list(range(6)))])
        named = lambda sd: {k.replace("network.", "net."): v for k, v in sd.items()}
        for suffix, obj in zip(STAGE2_FILES + TARGET_FILES,
                               (self.critic_1.state_dict(), half(0), self.critic_2.state_dict(), half(6), named(self.actor.state_dict()),
                                self.actor_optimizer.state_dict(), named(self.actor_target.state_dict()), self.critic_1_target.state_dict(),
                                self.critic_2_target.state_dict())):
            torch.save(obj, filename + suffix)

    def _load_stage2(self, ld, filename):
        """Reads what _save_stage2 wrote.  A checkpoint without the three target files (the reference's ten) loads with the targets
        copied from the online nets."""
        unnamed = lambda sd: {k.replace("net.", "network."): v for k, v in sd.items()}
        self.critic.load_state_dict(_merge_members(self.critic, (ld("_critic_1"), ld("_critic_2"))))
        self.actor.load_state_dict(unnamed(ld("_actor")))
        h1, h2 = ld("_critic_1_optimizer"), ld("__critic_2_optimizer")
        state = dict(h1["state"])
        state.update({k + 6: v for k, v in h2["state"].items()})
        if len(h1["state"]) != len(h2["state"]) or (state and float(h1["state"][0]["step"]) != float(h2["state"][0]["step"])):
            raise ValueError("critic optimizers: the two critics' step counts differ; one optimizer steps both")
        self.critic_optimizer.load_state_dict(dict(state=state, param_groups=[dict(h1["param_groups"][0], params=list(range(12)))]))
        self.actor_optimizer.load_state_dict(ld("_actor_optimizer"))
        if all(os.path.exists(filename + f) for f in TARGET_FILES):
            self.actor_target.load_state_dict(unnamed(ld("_actor_target")))
            self.critic_target.load_state_dict(_merge_members(self.critic_target, (ld("_critic_1_target"), ld("_critic_2_target"))))
        else:
            self.actor_target.load_state_dict(self.actor.state_dict())
            self.critic_target.load_state_dict(self.critic.state_dict())

    def load(self, filename):
        """Reads the four VAE files (the reference's load goes on to pass a file NAME to the actor optimizer's load_state_dict
        and cannot run; the critic / actor files are the second stage's: read with config['critic_actor'], see _load_stage2)."""
        ld = lambda s: torch.load(filename + s, map_location="cpu", weights_only=True)
        self.vae_policy.load_state_dict(ld("_vae_policy"))
        self.vae_policy_optimizer.load_state_dict(ld("_vae_policy_optimizer"))
        self.vae_dyna.load_state_dict(ld("_vae_dynamics"))
        self.vae_dyna_optimizer.load_state_dict(ld("_vae_dynamics_optimizer"))
        if self.critic_actor:
            self._load_stage2(ld, filename)
        self._graph = None
