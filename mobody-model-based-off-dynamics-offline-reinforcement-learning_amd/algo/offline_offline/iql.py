"""IQL baseline -- host-side mirror of the reference's `algo/offline_offline/iql.py` (class IQL), written from the algorithm.

Same plugin surface as the reference: `IQL(config, device, target_entropy=None)`, `.train(src_rb, tar_rb, batch_size, writer,
wandbrun)`, `.select_action(state, test=True)`, `.update_target()`, `.save/.load(prefix)` (the seven files `_critic`,
`_critic_optimizer`, `_value`, `_value_optimizer`, `_actor`, `_actor_optimizer`, `_actor_lr_scheduler`), attributes `.q_funcs
.target_q_funcs .v_func .policy .q_optimizer .v_optimizer .policy_optimizer .policy_lr_schedule .total_it`.

What the step is (iql.py:204-240): the batch is src(bs) | tar(bs) -- no trg_ratio, no model, no fake buffer, no refresh.
  1. V: adv = min(Qt1, Qt2)(s, a) - V(s) with the TARGET twin-Q; L_V = mean(|lam - 1[adv < 0]| adv^2); Adam(critic_lr).
  2. Q: y = r + nd gamma V(s') with the V of AFTER step 1; L_Q = mse(q1, y) + mse(q2, y); Adam(critic_lr); Polyak.
  3. policy: w = min(exp(temp adv), 100) with the adv of step 1 (V BEFORE its update, detached);
     L_pi = mean over N A of w (tanh(mu) - a)^2, mu the first A of the policy's 2 A outputs, NO max_action factor;
     Adam(actor_lr) under CosineAnnealingLR(T_max = config['max_step']): gradient step k runs at lr0 (1 + cos(pi (k-1) / T)) / 2.
The logstd half of the policy's output layer takes an exactly zero gradient, so those parameters keep their initial bits.
Each phase is one entry point (`mobody_iql_value / _critic / _actor`, csrc/train.hip; seed modes 5 and 6 of csrc/mlp_bwd.hip).

IQL is a MOBODY subclass: packed nets, Adam state, the health guard, the `mfma` key and the HIP-graph replay are the base
class's.  The base reads its step layout from `self.config`, so the constructor hands it the IQL step in MOBODY's terms
(`step_config`); the caller's dict is kept as `user_config`.

Where the reference is odd: its `load()` raises NameError (`file_name`) -- `load` here works and reads the seven files
its `save` writes; `update_interval` and `target_entropy` are stored and unused, there as here; its `alpha` property reads a
`log_alpha` that does not exist and is left out.  Not built: data-parallel IQL (refused in the constructor, before any collective).
"""
import math
import os

import numpy as np
import torch

from ... import ops
from .mobody import MOBODY, REFRESH_EVERY, _Adam, _PackedNet, refuse_data_parallel, refuse_missing_keys


def step_config(config):
    """The IQL step in the terms the MOBODY base class reads its config in."""
    step = dict(config)
    step.update(src_ratio=1, trg_ratio=1, fake_batch_scale=0, fake_buffer_size=1, q_weighted=0, advantage=1, scale_Q=0,
                penalize_fake=0, rollout_from_src=0, penalty_type="none", weight=0.0, bc_coef=0.0)
    step.setdefault("gaussian_noise_std", 1.0)
    return step


class _GaussianPolicy(_PackedNet):
    """Policy (iql.py:66-95): a packed S -> 2 A MLP with linear outputs mu | logstd."""

    def __init__(self, S, A, max_action, device, precision):
        _PackedNet.__init__(self, S, 2 * A, 1, ("network.",), device, precision=precision)
        self.action_dim, self.max_action = A, float(max_action)

    def mu_logstd(self, x):
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device)
        return ops.mlp3_forward(self.blob, self.in_dim, self.out_dim, 1, x, blob_T=self.blob_T, precision=self.precision)[0]

    def __call__(self, x, get_logprob=False):
        """iql.py:74-89: (sampled action, log-probability or None, tanh(mu)), both actions times max_action.  The sample is
        drawn with torch on the device."""
        mu, logstd = self.mu_logstd(x).chunk(2, dim=1)
        std = torch.clamp(logstd, -20, 2).exp()
        pre = mu + std * torch.randn_like(mu)
        action = torch.tanh(pre)
        logprob = None
        if get_logprob:
            base = torch.distributions.Normal(mu, std).log_prob(pre)
            jac = 2.0 * (math.log(2.0) - pre - torch.nn.functional.softplus(-2.0 * pre))
            logprob = (base - jac).sum(axis=-1, keepdim=True)
        return action * self.max_action, logprob, torch.tanh(mu) * self.max_action


class _CosineLR(object):
    """CosineAnnealingLR(policy_optimizer, T_max), eta_min 0, in closed form: `last_epoch` IS the optimizer's step count (the
    reference steps both once per train() call), so a replayed step that advances the count advances the schedule."""

    def __init__(self, opt, T_max):
        self.optimizer, self.T_max, self.eta_min, self.base_lrs = opt, int(T_max), 0, [opt.lr]

    @property
    def last_epoch(self):
        return self.optimizer.t

    def lr_of_step(self, k):
        """Learning rate of 1-based gradient step k."""
        return ops.cosine_lr(self.base_lrs[0], k, self.T_max)

    def get_last_lr(self):
        return [self.lr_of_step(self.last_epoch + 1)]

    def step(self):
        """The schedule follows the optimizer's count: nothing to advance."""

    def state_dict(self):
        return dict(T_max=self.T_max, eta_min=self.eta_min, base_lrs=list(self.base_lrs), last_epoch=self.last_epoch,
                    _step_count=self.last_epoch + 1, _get_lr_called_within_step=False, _last_lr=self.get_last_lr())

    def load_state_dict(self, sd):
        self.T_max, self.eta_min, self.base_lrs = int(sd["T_max"]), sd.get("eta_min", 0), [float(x) for x in sd["base_lrs"]]
        if self.eta_min != 0:
            raise ValueError("policy_lr_schedule: eta_min != 0 is not built")
        self.optimizer.lr = self.base_lrs[0]
        if int(sd["last_epoch"]) != self.optimizer.t:
            raise ValueError(f"policy_lr_schedule: last_epoch {sd['last_epoch']} != the policy optimizer's step count "
                             f"{self.optimizer.t} (the reference steps both once per train() call)")


class IQL(MOBODY):
    third_loss_name = "v_loss"            # losses()[2], where MOBODY and TD3_BC report the BC loss

    def __init__(self, config, device, target_entropy=None):
        refuse_data_parallel("IQL", "iql")
        # The reference reads config['lam'], ['temp'] and ['max_step'] without defaults: a MOBODY or TD3_BC config handed to 'iql' is
        # not an IQL run (T_max above all shapes the whole schedule).
        refuse_missing_keys("IQL", [k for k in ("lam", "temp", "max_step") if k not in config],
                            "config/mujoco/iql/*.yaml values are lam 0.7, temp 3.0, max_step 500000")
        self.lam, self.temp, self.T_max = float(config["lam"]), float(config["temp"]), int(config["max_step"])
        if not 0.0 < self.lam < 1.0:
            raise ValueError(f"config['lam'] = {self.lam} outside (0, 1)")
        if self.T_max < 1:
            raise ValueError(f"config['max_step'] = {self.T_max} < 1 (T_max of the policy's cosine schedule)")
        if 2 * int(config["action_dim"]) > 128:
            raise ValueError("action_dim: the policy's 2 A outputs must fit 128 columns")
        self.user_config = config
        MOBODY.__init__(self, step_config(config), device)
        self.target_entropy = target_entropy if target_entropy else -config["action_dim"]     # stored, unused (as the reference)
        S, A = self.S, self.A
        self.v_func = _PackedNet(S, 1, 1, ("network.",), self.device, precision=self.precision)
        self.v_optimizer = _Adam(self.v_func, config["critic_lr"])
        self.policy = _GaussianPolicy(S, A, config["max_action"], self.device, self.precision)
        self.policy_optimizer = _Adam(self.policy, config["actor_lr"])
        self.policy_lr_schedule = _CosineLR(self.policy_optimizer, self.T_max)
        self._adv = None
        self._log = torch.zeros(2, dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ acting / targets
    def select_action(self, state, test=True):
        """iql.py:160-166: one state in, the squeezed action as numpy out (test: tanh(mu) * max_action, else a sample)."""
        x = torch.as_tensor(np.asarray(state), dtype=torch.float32).reshape(1, -1)
        action, _, mean = self.policy(x.to(self.device))
        return (mean if test else action).squeeze().cpu().numpy()

    def eval_policy(self):
        """(net, head) for fitted Q evaluation: the Gaussian policy, head 1 (max_action * tanh(mu), select_action's test action)."""
        return self.policy, 1

    def update_target(self):
        """iql.py:168-172.  (train() does not call it: the critic's optimizer launch applies the Polyak update itself.)"""
        t, q = self.target_q_funcs, self.q_funcs
        t.blob.copy_(self.tau * q.blob + (1.0 - self.tau) * t.blob)
        ops.mlp_transpose(t.blob, t.in_dim, t.out_dim, t.members, out=t.blob_T, precision=t.precision)

    def _extra_named(self):
        return (("v_func", self.v_func, self.v_optimizer),)

    # ------------------------------------------------------------------ training
    def _dims(self, N, Nt, Ng, Ntg):
        if self._ws_key != (N, Nt):
            self._ws = ops.iql_workspace(ops.train_dims(self.S, self.A, N, Nt, N, Nt), self.device)
            self._adv = torch.zeros(N, dtype=torch.float32, device=self.device)
            self._ws_key = (N, Nt)
        return ops.train_dims(self.S, self.A, N, Nt, Ng, Ntg), ops.hyper(self.config)

    def _nets(self):
        return (self.v_func, self.q_funcs, self.target_q_funcs, self.policy)

    def _graph_ok(self, writer):
        """Replay the steady-state step (rng='device', fused updates); the logging steps run eagerly."""
        want = self.use_graph == 1 or (self.use_graph == 2 and self._batch[0].shape[0] < 4096)
        logs = writer is not None and self.total_it % 5000 == 0
        return bool(want and self.rng == "device" and self.fused_update and not logs)

    def _captured_gather(self, src, tar, bs, out, seed_ids=(101, 102), bump=(1, 2, 3)):
        """The draw [src(bs) | tar(bs)] of a captured step: call id c[0] + 1 (the critic's optimizer launch advances c[0]); the
        launch advances the step words `bump` of the optimizers that follow it (it does not read them)."""
        c, bufs = self._ctr, [src, tar]
        ops.gather_batch_rng(buffers=[rb._fields() for rb in bufs], counts=[bs, bs], seeds=[self._seed_for(k) for k in seed_ids],
                             call_offsets=[1, 1], counter=c[0:1], sizes=[rb.ptr_size[1:2] for rb in bufs], S=self.S, A=self.A,
                             out=out, bump=tuple(c[k:k + 1] for k in bump))

    def _graph_segments(self, src, tar, batch_size, world, segmented):
        bs = int(batch_size)

        def fused_step():
            self._captured_gather(src, tar, bs, self._batch)
            self._update(self._batch, 2 * bs, 2 * bs, dev=True)
        return [fused_step]

    # What a baseline with IQL's three phases behind a step of its own overrides: _rows, _buffers and _draw (DARA, IGDF).
    def _rows(self, bs):
        """Rows of the training batch at batch size bs."""
        return 2 * bs

    def _rows5(self, rows):
        return tuple(torch.empty(rows, w, device=self.device) for w in (self.S, self.A, self.S, 1, 1))

    def _buffers(self, bs, N, alloc=False):
        """Whether the cached minibatch tensors fit the step; alloc: make them fit."""
        fit = self._batch is not None and self._batch_key == (N,)
        if alloc and not fit:
            self._batch, self._batch_key = self._rows5(N), (N,)
        return fit

    def _draw(self, src, tar, bs, N, writer, log5k):
        """The eager step up to IQL's phases: fill self._batch.  Index draws in the reference's order: src, tar."""
        self._gather([src, tar], [bs, bs], self._batch)

    def train(self, src_replay_buffer, tar_replay_buffer, batch_size=128, writer=None, wandbrun=None):
        """One gradient step (iql.py:204-240, dara.py:271-324, igdf.py:487-549)."""
        self.total_it += 1
        if not self._synced:
            self.sync_replicas()
        bs = int(batch_size)
        N = self._rows(bs)
        log5k = writer is not None and self.total_it % 5000 == 0
        if (self.total_it - 1) % REFRESH_EVERY == 0 or log5k:
            self._health_check()
        if self._buffers(bs, N) and self._graph_ok(writer) and self._graph_step(src_replay_buffer, tar_replay_buffer, batch_size):
            return
        if self._graph is not None:                       # an eager step moves the host-side counts
            self._graph = None
        self._buffers(bs, N, alloc=True)
        self._draw(src_replay_buffer, tar_replay_buffer, bs, N, writer, log5k)
        self._update(self._batch, N, N, log=log5k)
        if log5k:      # the three scalars of a logging step, each from BEFORE the update of its net (:181-183, :193-194)
            adv_mean, v_mean, q1_mean = [float(x) for x in torch.cat([self._log, self._q1_mean.reshape(1)]).tolist()]
            writer.add_scalar("train/adv", adv_mean, self.total_it)
            writer.add_scalar("train/value", v_mean, self.total_it)
            writer.add_scalar("train/q1", q1_mean, self.total_it)

    def _critic(self, *args, **kw):
        """The twin-Q phase's call (a subclass with a row-weighted loss puts its own here)."""
        ops.iql_critic(*args, **kw)

    def _update(self, b, N, Nt, dev=False, log=False):
        """V -> Q (+ Polyak) -> policy.  dev: the step counts are the device words of the captured step (already advanced)."""
        dims, hyp = self._dims(N, N, N, N)
        head = (dims, hyp, self.lam, self.temp, self.T_max, self._nets(), b, self._adv)
        ov, oq, op = self.v_optimizer, self.q_optimizer, self.policy_optimizer
        c = self._ctr
        if log:
            q12 = ops.mlp3_forward(self.q_funcs.blob, self.S + self.A, 1, 2, b[0], b[1], blob_T=self.q_funcs.blob_T, precision=self.precision)
            self._q1_mean = q12[0].mean()
        if self.fused_update:
            if not dev:
                ov.t += 1; oq.t += 1; op.t += 1
            ops.iql_value(*head, self._loss[3:4], self._ws, m=ov.m, v=ov.v, t=ov.t, t_dev=c[3:4] if dev else None, lr=ov.lr,
                          log_out=self._log if log else None)
            self._critic(*head, self._loss[0:1], self._ws, m=oq.m, v=oq.v, t=oq.t, t_dev=c[1:2] if dev else None, lr=oq.lr,
                         bump=c[0:1] if dev else None)
            ops.iql_actor(*head, self._loss[1:2], self._ws, m=op.m, v=op.v, t=op.t, t_dev=c[2:3] if dev else None, lr=op.lr)
            return
        assert not dev, "the captured step is the fused form"
        ops.iql_value(*head, self._loss[3:4], self._ws, grad=ov.grad, log_out=self._log if log else None)
        ov.step()
        self._critic(*head, self._loss[0:1], self._ws, grad=oq.grad)
        oq.step(target=self.target_q_funcs, tau=self.tau)
        ops.iql_actor(*head, self._loss[1:2], self._ws, grad=op.grad)
        lr0 = op.lr
        op.lr = self.policy_lr_schedule.lr_of_step(op.t + 1)
        try:
            op.step()
        finally:
            op.lr = lr0

    def losses(self):
        """(q_loss, pi_loss, v_loss) of the last step (forces a device sync)."""
        q, pi, _, v = [float(x) for x in self._loss.tolist()]
        return q, pi, v

    # ------------------------------------------------------------------ checkpoints (iql.py:246-262)
    def save(self, filename):
        self._health_check()
        torch.save(self.q_funcs.state_dict(), filename + "_critic")
        torch.save(self.q_optimizer.state_dict(), filename + "_critic_optimizer")
        torch.save(self.v_func.state_dict(), filename + "_value")
        torch.save(self.v_optimizer.state_dict(), filename + "_value_optimizer")
        torch.save(self.policy.state_dict(), filename + "_actor")
        sd = self.policy_optimizer.state_dict()           # as torch saves a scheduled optimizer: the current rate + the base rate
        sd["param_groups"][0].update(lr=self.policy_lr_schedule.get_last_lr()[0], initial_lr=self.policy_optimizer.lr)
        torch.save(sd, filename + "_actor_optimizer")
        torch.save(self.policy_lr_schedule.state_dict(), filename + "_actor_lr_scheduler")

    def _ld(self, filename, suffix):
        return torch.load(filename + suffix, map_location="cpu", weights_only=True)

    def load(self, filename, optional=()):
        """optional: of "_value" (with its optimizer's file) and "_actor_lr_scheduler", the files a checkpoint may lack."""
        self._graph = None                              # re-capture: the device-side Adam step counts change
        self._synced = False
        ld = lambda s: self._ld(filename, s)
        have = lambda s: s not in optional or os.path.exists(filename + s)
        self.q_funcs.load_state_dict(ld("_critic"))
        self.q_optimizer.load_state_dict(ld("_critic_optimizer"))
        if have("_value"):
            self.v_func.load_state_dict(ld("_value"))
            self.v_optimizer.load_state_dict(ld("_value_optimizer"))
        self.policy.load_state_dict(ld("_actor"))
        self.policy_optimizer.load_state_dict(ld("_actor_optimizer"))
        if have("_actor_lr_scheduler"):
            self.policy_lr_schedule.load_state_dict(ld("_actor_lr_scheduler"))   # (restores the optimizer's base rate)
        else:                                             # a reference checkpoint: the optimizer file holds the scheduled rate
            self.policy_optimizer.lr = self.policy_lr_schedule.base_lrs[0]
