"""TD3_BC baseline -- host-side mirror of the reference's `algo/offline_offline/td3_bc.py` (class TD3BC), written from the
algorithm.

Same plugin surface as the reference: `TD3BC(config, device, target_entropy=None)`, `.train(src_rb, tar_rb, batch_size, writer,
wandbrun)`, `.select_action(state, test=True)`, `.update_target()`, `.save/.load(prefix)` (the four files `_critic`,
`_critic_optimizer`, `_actor`, `_actor_optimizer`), attributes `.q_funcs .target_q_funcs .policy .q_optimizer
.policy_optimizer .classifier .total_it`.

What the step is (td3_bc.py:178-224): the batch is src(bs) | tar(int(trg_ratio * bs)) -- no model, no fake buffer, no refresh;
the critic update is MOBODY's (min target-Q TD regression, Adam, Polyak) and runs through `mobody_critic` unchanged; the actor
loss is `weight / mean|Q| * mean(-Q) + bc_coef * BC` with BC on EVERY row against the batch's own actions, and
`config['advantage'] == 1` weights each row's BC term by min(exp(q / mean|q|), 100) of the same Q(s, pi(s)) the policy term uses,
NOT detached: its gradient reaches the actor through the frozen critic (`mobody_td3bc_actor_forward / _backward`, seed mode 4 of
csrc/mlp_bwd.hip).  `penalty_type == 'dara'` trains the domain classifier every step and adds 0.1 * penalty to the step's source
rewards; every other value (the CLI's default 'par' included) does nothing.

TD3BC is a MOBODY subclass: packed nets, Adam state, checkpoints, the health guard, the `mfma` key, the engine interface of
`dp.dp_update` and the HIP-graph replay are the base class's.  The base reads its step layout from `self.config`, so the
constructor hands it the TD3_BC step in MOBODY's terms (`step_config`): src_ratio 1, no fake rows, no V phase, `q_weighted` =
(advantage == 1), scale_Q 1; the caller's dict is kept as `user_config`.  Only the batch assembly (`train`) and the three actor
methods differ.  Not built: data-parallel TD3_BC (refused in the constructor, before any collective) and graph capture under
'dara' (those steps run eagerly).
"""
import numpy as np
import torch

from ... import ops
from .mobody import MOBODY, REFRESH_EVERY, refuse_data_parallel

DARA_REWARD_COEF = 0.1          # td3_bc.py:200 (a literal there, not config['penalty_coef'])


def step_config(config):
    """The TD3_BC step in the terms the MOBODY base class reads its config in."""
    step = dict(config)
    step.update(src_ratio=1, fake_batch_scale=0, fake_buffer_size=1, q_weighted=int(config["advantage"] == 1), advantage=0,
                scale_Q=1, penalize_fake=0, rollout_from_src=0,
                penalty_type="dara" if config["penalty_type"] == "dara" else "none")
    step.setdefault("gaussian_noise_std", 1.0)          # Classifier's constructor default (td3_bc.py:52, :104)
    return step


class TD3BC(MOBODY):
    def __init__(self, config, device, target_entropy=None):
        refuse_data_parallel("TD3_BC", "td3_bc")
        self.user_config = config
        MOBODY.__init__(self, step_config(config), device)

    # ------------------------------------------------------------------ acting / targets
    def select_action(self, state, test=True):
        """td3_bc.py:136-139: one state in, the squeezed action as numpy out."""
        x = torch.as_tensor(np.asarray(state), dtype=torch.float32).reshape(1, -1)
        return self.policy(x.to(self.device)).squeeze().cpu().numpy()

    def update_target(self):
        """td3_bc.py:141-145.  (train() does not call it: the critic's optimizer launch applies the Polyak update itself.)"""
        t, q = self.target_q_funcs, self.q_funcs
        t.blob.copy_(self.tau * q.blob + (1.0 - self.tau) * t.blob)
        ops.mlp_transpose(t.blob, t.in_dim, t.out_dim, t.members, out=t.blob_T, precision=t.precision)

    # ------------------------------------------------------------------ training
    def _counts(self, batch_size):
        return int(batch_size), int(self.config["trg_ratio"] * batch_size)

    def _graph_ok(self, writer):
        """Replay the steady-state step (rng='device'): no refresh steps; 'dara' and the logging steps run eagerly."""
        want = self.use_graph == 1 or (self.use_graph == 2 and self._batch[0].shape[0] < 4096)
        logs = writer is not None and self.total_it % 5000 == 0
        return want and self.rng == "device" and self.penalty_type != "dara" and not logs

    def train(self, src_replay_buffer, tar_replay_buffer, batch_size=128, writer=None, wandbrun=None):
        """One gradient step, td3_bc.py:178-224.  Index draws in the reference's order: src, tar, then under 'dara' the
        classifier's src(bs), tar(bs)."""
        self.total_it += 1
        if not self._synced:
            self.sync_replicas()
        S, A = self.S, self.A
        ns, nt = self._counts(batch_size)
        N = ns + nt
        log5k = writer is not None and self.total_it % 5000 == 0
        if (self.total_it - 1) % REFRESH_EVERY == 0 or log5k:
            self._health_check()
        if (self._batch is not None and self._batch_key == (N,) and self._graph_ok(writer)
                and self._graph_step(src_replay_buffer, tar_replay_buffer, batch_size)):
            return
        if self._graph is not None:                       # an eager step moves the host-side counts
            self._graph = None
        if self._batch_key != (N,):
            dev = self.device
            self._batch = (torch.empty(N, S, device=dev), torch.empty(N, A, device=dev), torch.empty(N, S, device=dev),
                           torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev))
            self._batch_key = (N,)
        b = self._batch
        self._gather([src_replay_buffer, tar_replay_buffer], [ns, nt], b)
        if self.penalty_type == "dara":                                       # :187-200
            loss_sa, loss_sas = self.update_classifier(src_replay_buffer, tar_replay_buffer, batch_size, writer)
            if log5k:                                                         # :132-134
                writer.add_scalar("train/sas classifier loss", loss_sas, global_step=self.total_it)
                writer.add_scalar("train/sa classifier loss", loss_sa, global_step=self.total_it)
                delta = self._dara_delta(b[0][:ns], b[1][:ns], b[2][:ns])
                writer.add_scalar("train/reward penalty", delta.mean(), global_step=self.total_it)
            self._dara_delta(b[0][:ns], b[1][:ns], b[2][:ns], b[3][:ns], DARA_REWARD_COEF)
        if log5k:                                                             # :155-156, the critic before this step's update
            q12 = ops.mlp3_forward(self.q_funcs.blob, S + A, 1, 2, b[0], b[1], blob_T=self.q_funcs.blob_T, precision=self.precision)
            writer.add_scalar("train/q1", q12[0].mean(), self.total_it)
        self._update(b, N, N)

    # ---- engine interface of dp.dp_update: the critic half is the base class's, the actor half is TD3_BC's ----
    def actor_stats(self, b, N, Nt, Ng, Ntg):
        dims, hyp = self._dims(N, N, Ng, Ng)
        ops.td3bc_actor_forward(dims, hyp, self.policy.blob, self.q_funcs.blob, b[0], b[1], self._stats, self._ws,
                                policy_ready=self._policy_rides_along(), actor_blob_T=self.policy.blob_T,
                                q_blob_T=self.q_funcs.blob_T)

    def actor_grad(self, b, N, Nt, Ng, Ntg):
        dims, hyp = self._dims(N, N, Ng, Ng)
        ops.td3bc_actor_backward(dims, hyp, self.policy.blob, self.policy.blob_T, self.q_funcs.blob, self.q_funcs.blob_T,
                                 b[0], b[1], self._stats, self.policy_optimizer.grad, self._loss[1:3], self._ws)

    def actor_update(self, b, N, Nt, t_dev=None):
        dims, hyp = self._dims(N, N, N, N)
        o = self.policy_optimizer
        if t_dev is None:
            o.t += 1
        ops.td3bc_actor_update(dims, hyp, self.policy.blob, self.policy.blob_T, self.q_funcs.blob, self.q_funcs.blob_T, b[0],
                               b[1], self._stats, o.m, o.v, o.t, o.lr, self._loss[1:3], self._ws, t_dev=t_dev)
