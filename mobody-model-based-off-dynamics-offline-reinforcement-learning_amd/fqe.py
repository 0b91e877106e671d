"""Fitted Q evaluation of a frozen policy on the recorded target transitions.  The reference has no counterpart.

A fresh twin-Q net is regressed onto y = r + gamma not_done Q_targ(s', pi(s')) and Q(s0, pi(s0)) is reported over start states.
One step = the ring gather of `batch_size` target rows, `mobody_fqe_target`, `mobody_critic` in its q_next form with Adam and the
Polyak update fused.  With rng='device' the step replays as one HIP graph after one eager step at its size; the gather's call id and
the Adam step count then live in device words.  Rows are drawn by the device generator whatever `rng` says; `rng` only decides
whether the step replays.

Isolation: FQE draws rows with a seed id of its own (SEED_FQE_INDEX; the algorithm classes use 101-110), initialises its nets from a
generator of its own (SEED_FQE_INIT) and advances only its own counts -- the buffers' `_draws`, the algorithm's counters and torch's
generators do not move.  It reports into health words of its own, bound for the length of fit() / value() only.
"""
import contextlib
import math
import warnings

import torch

from . import _lib, ops
from .algo.offline_offline.mobody import _Adam, _PackedNet

SEED_FQE_INDEX, SEED_FQE_INIT = 111, 112       # seed ids: the row draws' stream, the nets' initial values


def initial_state_dict(S, A, seed):
    """The twin-Q's initial values (nn.Linear's default init) from a CPU generator seeded with seed + SEED_FQE_INIT: needs no GPU."""
    g = torch.Generator().manual_seed((int(seed) + SEED_FQE_INIT) & 0xFFFFFFFF)
    sd = {}
    for p in ("network1.", "network2."):
        for li, (i, o) in zip((0, 2, 4), ((S + A, 256), (256, 256), (256, 1))):
            bound = 1.0 / math.sqrt(i)
            sd[f"{p}network.{li}.weight"] = torch.empty(o, i).uniform_(-bound, bound, generator=g)
            sd[f"{p}network.{li}.bias"] = torch.empty(o).uniform_(-bound, bound, generator=g)
    return sd


class FQE(object):
    def __init__(self, policy_net, head, S, A, max_action, gamma, device, precision, lr=3e-4, tau=0.005, batch_size=256, seed=0,
                 rng="device"):
        if int(head) not in (0, 1):
            raise ValueError(f"head {head!r}: 0 (deterministic actor) or 1 (Gaussian policy)")
        want_out = A if int(head) == 0 else 2 * A
        if policy_net.in_dim != S or policy_net.out_dim != want_out or policy_net.members != 1:
            raise ValueError(f"head {head}: the policy must be a one-member {S} -> {want_out} net, got {policy_net.in_dim} -> "
                             f"{policy_net.out_dim} x {policy_net.members}")
        self.policy_net, self.head, self.S, self.A = policy_net, int(head), int(S), int(A)
        self.max_action, self.gamma, self.tau, self.lr = float(max_action), float(gamma), float(tau), float(lr)
        self.device = torch.device(device)
        self.batch_size, self.seed, self.rng = int(batch_size), int(seed), rng
        self.precision = ops.prec_id(precision)
        if self.precision in (1, 2):
            raise ValueError("FQE runs at mfma 'f32', 'bf16x3' or 'f16x2'")
        dev = self.device
        self.q = _PackedNet(S + A, 1, 2, ("network1.", "network2."), dev, init=False, precision=self.precision)
        self._init_nets()
        self.q_target = self.q.clone().eval()
        self.optimizer = _Adam(self.q, self.lr)
        self._health = torch.zeros(_lib.HEALTH_WORDS, dtype=torch.int32, device=dev)
        self._ctr = torch.zeros(4, dtype=torch.int64, device=dev)        # [gather call id, Adam step, spare, spare]
        self._calls, self._ctr_stale = 0, True
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self._out = torch.zeros(5, dtype=torch.float32, device=dev)      # value()'s four words + the NaN flag (int32 bits)
        self._policy_T = None                                            # the policy's T blob at self.precision, when that differs
        self._buf_key, self._buf = None, None
        self._graph, self._graph_key, self._warm = None, None, None
        self.captures, self.replays = 0, 0
        self.fault = None                    # names of the health bits the last fit() raised, or None
        self._fallback = False               # the next prepare() moves FQE to bf16x3
        self._own_mode = False               # FQE fell back on its own: it no longer follows the policy's mode

    # ------------------------------------------------------------------ nets
    def _init_nets(self):
        """nn.Linear's default init of the twin-Q from FQE's own generator (torch's global generators are not touched)."""
        self.q.load_state_dict(initial_state_dict(self.S, self.A, self.seed))

    def reset(self, precision=None):
        """Nets, moments and counts back to their initial values from the FQE seed; precision: also move to that MFMA mode."""
        if precision is not None:
            self.precision = self.q.precision = self.q_target.precision = ops.prec_id(precision)
        self._init_nets()
        t = self.q_target
        t.blob.copy_(self.q.blob)
        ops.mlp_transpose(t.blob, t.in_dim, t.out_dim, t.members, out=t.blob_T, precision=t.precision)
        t.version += 1
        o = self.optimizer
        o.m.zero_(); o.v.zero_(); o.grad.zero_()
        o.t, self._calls, self._ctr_stale = 0, 0, True
        self._health.zero_()
        self.fault = None
        self._graph = None                   # the precision is part of what a capture holds

    def _policy_planes(self):
        """The policy's T blob in FQE's precision: the policy's own, or -- after FQE alone fell back to bf16x3 -- a copy built here
        from the policy's fp32 weights (rebuilt per evaluation: the policy trains in between)."""
        p = self.policy_net
        if p.precision == self.precision or self.precision == 0:
            self._policy_T = None
            return
        if self._policy_T is None:
            self._policy_T = torch.empty_like(p.blob_T)
        ops.mlp_transpose(p.blob, p.in_dim, p.out_dim, p.members, out=self._policy_T, precision=self.precision)

    @contextlib.contextmanager
    def _own_health(self):
        """FQE's launches report into FQE's words; whatever was bound before is bound again afterwards."""
        with torch.cuda.device(self.device):
            prev = ops.health_bound(self.device)
            ops.health_bind(self._health)
            try:
                yield
            finally:
                ops.health_bind(prev)

    # ------------------------------------------------------------------ the step
    def _buffers(self, bs):
        if self._buf_key != (bs, self.head):
            dev, S, A = self.device, self.S, self.A
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            batch = (f(bs, S), f(bs, A), f(bs, S), f(bs, 1), f(bs, 1))
            blk = _lib.block(_lib.MobodyFqeTarget, head=self.head, S=S, A=A, N=bs)
            dims = ops.train_dims(S, A, bs, bs)
            self._buf = dict(batch=batch, q_next=f(bs), tws=ops.fqe_target_workspace(blk, dev), dims=dims,
                             ws=ops.train_workspace(dims, dev))
            self._buf_key, self._warm = (bs, self.head), None
        return self._buf

    def _hyper(self):
        return _lib.MobodyHyper(self.gamma, self.tau, self.max_action, 1.0, 0.0, 0, 1, self.precision)

    def _seed(self):
        return (self.seed + SEED_FQE_INDEX) & 0xFFFFFFFF

    def _step(self, tar, bs, dev_words):
        """One step's launches.  dev_words: the call id and the step count are the device words (a captured step); else the host's."""
        z, c, o = self._buf, self._ctr, self.optimizer
        ops.gather_batch_rng(buffers=[tar._fields()], counts=[bs], seeds=[self._seed()], call_offsets=[1 if dev_words else self._calls + 1],
                             counter=c[0:1] if dev_words else None, sizes=[tar.ptr_size[1:2]], S=self.S, A=self.A, out=z["batch"],
                             bump=(c[1:2],) if dev_words else ())
        ops.fqe_target(ops.fqe_target_block(self.policy_net, self.head, self.q_target, z["batch"][2], z["q_next"], ws=z["tws"],
                                            policy_T=self._policy_T))
        ops.critic_update(z["dims"], self._hyper(), None, self.q.blob, self.q.blob_T, self.q_target.blob, z["batch"], o.m, o.v,
                          0 if dev_words else o.t + 1, o.lr, self._loss, z["ws"], q_next=z["q_next"], t_dev=c[1:2] if dev_words else None,
                          qtarg_blob_T=self.q_target.blob_T, bump=c[0:1] if dev_words else None)

    def _key(self, tar, bs):
        z, o, p = self._buf, self.optimizer, self.policy_net
        return (bs, id(tar), tar.store.data_ptr(), tar.ptr_size.data_ptr(), tuple(t.data_ptr() for t in z["batch"]), z["q_next"].data_ptr(),
                z["tws"].data_ptr(), z["ws"].data_ptr(), p.blob.data_ptr(), (p.blob_T if self._policy_T is None else self._policy_T).data_ptr(),
                tuple((n.blob.data_ptr(), n.blob_T.data_ptr()) for n in (self.q, self.q_target)), o.m.data_ptr(), o.v.data_ptr(),
                self.precision, self.head)

    def _replay(self, tar, bs):
        key = self._key(tar, bs)
        if self._graph is None or self._graph_key != key:
            torch.cuda.synchronize()
            self._ctr_stale = True
            g = torch.cuda.CUDAGraph()
            try:
                self._sync_words()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._step(tar, bs, True)
            except Exception as exc:
                torch.cuda.synchronize()
                warnings.warn(f"HIP-graph capture of the FQE step failed ({exc!r}); continuing eagerly")
                self.rng, self._graph = "eager", None
                return False
            self._graph, self._graph_key = g, key
            self.captures += 1
        self._sync_words()
        self._graph.replay()
        self.replays += 1
        return True

    def _sync_words(self):
        if self._ctr_stale:
            self._ctr.copy_(torch.tensor([self._calls, self.optimizer.t, 0, 0], dtype=torch.int64))
            self._ctr_stale = False

    def fit(self, tar_rb, steps):
        """`steps` FQE steps on rows of `tar_rb`.  Returns True when the health words stayed clear (one host read, at the end)."""
        if tar_rb.size <= 0:
            raise ValueError("FQE.fit: the target buffer is empty")
        bs = self.batch_size
        self._buffers(bs)
        with self._own_health():
            self._policy_planes()
            for _ in range(int(steps)):
                if not (self.rng == "device" and self._warm == bs and self._replay(tar_rb, bs)):
                    self._step(tar_rb, bs, False)
                    self._ctr_stale, self._warm = True, bs
                self._calls += 1
                self.optimizer.t += 1
            mask, step = ops.health_read(self._health)
        if mask:
            self.fault = "|".join(ops.health_bits(mask))
            # the optimizer launches after the faulting one were frozen: the count goes back to the updates that were applied
            if 0 < step <= self.optimizer.t:
                self.optimizer.t, self._ctr_stale = step, True
            self._fallback = mask == _lib.HEALTH_F16_RANGE and self.precision == 4
            warnings.warn(f"FQE health words {self.fault}" + (f" at Adam step {step}" if step else "") + ": this evaluation's scalars are "
                          "skipped" + ("; the next evaluation runs at mfma='bf16x3'" if self._fallback else ""))
            return False
        self.fault = None
        return True

    def prepare(self, warm_start=False):
        """What the CLI does before an evaluation: a pending fallback resets at bf16x3; a policy that changed its own mode (its
        class fell back) takes FQE along; otherwise reset() unless warm_start."""
        p = self.policy_net.precision
        if self._fallback:
            self._fallback, self._own_mode = False, True
            self.reset(precision="bf16x3")
        elif p != self.precision and not self._own_mode:
            self.reset(precision=p)
        elif self.fault is not None or not warm_start:
            self.reset()

    def td_loss(self):
        """The last step's loss mse(q1, y) + mse(q2, y) (a host read)."""
        return float(self._loss.item())

    def value(self, start_obs):
        """dict(q1, q2, value, head_gap, nan) of Q(s0, pi(s0)) over the rows of start_obs, with one host read."""
        s0 = torch.as_tensor(start_obs, dtype=torch.float32).to(self.device).contiguous()
        flag = self._out[4:5].view(torch.int32)
        with self._own_health():
            self._policy_planes()
            blk = ops.fqe_value_block(self.policy_net, self.head, self.q, s0, self._out[:4], flag, policy_T=self._policy_T)
            ws = ops.fqe_value_workspace(blk, self.device)
            blk.workspace = ws.data_ptr()
            ops.fqe_value(blk)
        w = self._out.tolist()
        return dict(q1=w[0], q2=w[1], value=w[2], head_gap=w[3], nan=w[4] != 0.0)
