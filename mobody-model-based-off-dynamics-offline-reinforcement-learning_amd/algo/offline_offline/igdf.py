"""IGDF baseline -- host-side mirror of the reference's `algo/offline_offline/igdf.py` (class IGDF), written from the algorithm.

Same plugin surface as the reference: `IGDF(config, device, target_entropy=None)`, `.train(src_rb, tar_rb, batch_size, writer,
wandbrun)`, `.update_info(src_rb, tar_rb, batch_size, writer)`, `.select_action(state, test=True)`, `.update_target()`,
`.save/.load(prefix)`, attributes `.info .info_optimizer .update_interval` besides IQL's.

What the step is (igdf.py:487-549): IQL's step (iql.py of this package) behind a data filter.
  1. src(bs) then tar(bs) are drawn.  phi = encoder_sa([s | a]), psi = encoder_ss(s') on the source rows;
     score_i = phi_i . psi_i / (|phi_i| |psi_i|), no epsilon.
  2. k = int(bs * float(xi)); the k source rows of largest score are kept, in ascending score order (argsort(...)[-k:]).
  3. Row weights w = exp(importance_weight * score) on the kept rows, 1 on the target rows.
  4. IQL's V, Q (+ Polyak) and policy phases on the N = k + bs rows [kept src | tar]; the critic loss alone is weighted:
     mean(w (q1 - y)^2) + mean(w (q2 - y)^2).
`update_info` (igdf.py:418-447) trains the two encoders, `info_update_step` steps of an in-batch contrastive loss: tar(bs) then
src(bs - 1) are drawn, logits[i][0] = phi(tar_i) . psi(tar s'_i), logits[i][j] = phi(tar_i) . psi(src s'_{j-1}), binary
cross-entropy against a 1 in column 0, mean over bs^2; ONE Adam over both encoders at actor_lr.
Steps 1-3 are one entry point (`mobody_igdf_filter`), the contrastive step another (`mobody_igdf_info`), the weighted critic a
third (`mobody_igdf_critic`), csrc/train.hip and csrc/igdf.hip; with rng='device' and the fused update the whole train() step --
gather, filter, IQL's three phases -- replays as one HIP graph, and the info step as a graph of its own.

Where the reference is odd: its driver never calls `update_info`, so the encoders keep their initial values (the CLI
here calls it once before the loop when the config has a truthy `info_pretrain`); `ensemble_size > 1` makes its train() fail and
`repr_norm` with `repr_norm_temp` raises, so only ensemble_size 1, repr_norm false and ortho_init false are built; k = 0 breaks
its slicing: k < 1 and xi > 1 are ValueErrors here; `save` writes IQL's seven files and no encoder -- `save` here also writes
`_info` and `_info_optimizer`, `load` reads the seven and the two extras when present; its `alpha` property reads a `log_alpha`
that does not exist and is left out.  Not built: data-parallel IGDF (refused in the constructor, before any collective).
"""
import os

import torch

from ... import ops
from .iql import IQL
from .mobody import _Adam, _PackedNet, _PairedAdam, refuse_data_parallel, refuse_missing_keys

_KEYS = ("lam", "temp", "max_step", "xi", "importance_weight", "repr_dim", "ensemble_size", "repr_norm", "ortho_init", "info_update_step")
MAX_ROWS = 4096             # rows the selection and the contrastive kernel take (csrc/igdf.h)


class _ContrastiveInfo(object):
    """ContrastiveInfo (igdf.py:190-253) with ensemble_size 1: two packed MLPs with linear outputs."""

    def __init__(self, S, A, Z, device, precision):
        self.state_dim, self.action_dim, self.repr_dim, self.ensemble_size = S, A, Z, 1
        self.repr_norm, self.ortho_init = False, False
        self.encoder_sa = _PackedNet(S + A, Z, 1, ("encoder_sa.",), device, precision=precision)
        self.encoder_ss = _PackedNet(S, Z, 1, ("encoder_ss.",), device, precision=precision)

    def encode(self, obs, action, ss):
        return self.encoder_sa(torch.cat([torch.as_tensor(obs), torch.as_tensor(action)], dim=-1)), self.encoder_ss(ss)

    def __call__(self, obs, action, ss, return_repr=False):
        """API compatibility with ContrastiveInfo.forward (:248-253); the training path never calls this."""
        sa, s2 = self.encode(obs, action, ss)
        logits = torch.einsum("iz,jz->ij", sa, s2)
        return (logits, sa, s2) if return_repr else logits

    def state_dict(self):
        return {**self.encoder_sa.state_dict(), **self.encoder_ss.state_dict()}

    def load_state_dict(self, sd):
        self.encoder_sa.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder_sa.")})
        self.encoder_ss.load_state_dict({k: v for k, v in sd.items() if k.startswith("encoder_ss.")})

    def parameters(self):
        return self.encoder_sa.parameters() + self.encoder_ss.parameters()


def kept_rows(batch_size, xi):
    """k = int(bs * float(xi)) (igdf.py:507); k < 1 breaks the reference's slicing ([-0:] keeps every row) and is refused."""
    k = int(int(batch_size) * float(xi))
    if k < 1:
        raise ValueError(f"xi = {xi} keeps k = int({batch_size} * xi) = {k} source rows; the filter needs k >= 1")
    return k


class IGDF(IQL):
    def __init__(self, config, device, target_entropy=None):
        # The reference reads these keys without defaults: a MOBODY, TD3_BC or DARA config handed to 'igdf' is not an IGDF run.  This
        # refusal comes before every other check.
        refuse_missing_keys("IGDF", [k for k in _KEYS if k not in config],
                            "config/*/igdf/*.yaml values are lam 0.7, temp 3.0, xi 0.75, importance_weight 1.0, repr_dim 64, "
                            "ensemble_size 1, repr_norm False, ortho_init False, info_update_step 7000")
        if int(config["ensemble_size"]) != 1:
            raise NotImplementedError(f"config['ensemble_size'] = {config['ensemble_size']}: only ensemble_size 1 is built (the "
                                      "reference's train() fails on an ensemble: torch.diag of a 3-D tensor)")
        if config["repr_norm"]:
            raise NotImplementedError("config['repr_norm'] is not built (with repr_norm_temp the reference raises as well)")
        if config["ortho_init"]:
            raise NotImplementedError("config['ortho_init'] is not built: the encoders take nn.Linear's default initialisation")
        xi = float(config["xi"])
        if not 0.0 < xi <= 1.0:
            raise ValueError(f"config['xi'] = {config['xi']} outside (0, 1] (k = int(batch_size * xi) source rows are kept)")
        if not 1 <= int(config["repr_dim"]) <= 128:
            raise ValueError(f"config['repr_dim'] = {config['repr_dim']} outside 1..128")
        if int(config["info_update_step"]) < 0:
            raise ValueError(f"config['info_update_step'] = {config['info_update_step']} < 0")
        refuse_data_parallel("IGDF", "igdf")
        IQL.__init__(self, config, device, target_entropy)
        self._no_info_graph = False
        self.xi, self.importance_weight, self.Z = xi, float(config["importance_weight"]), int(config["repr_dim"])
        self.output_gain = config.get("output_gain")          # read under ortho_init only: stored, unused
        self.info = _ContrastiveInfo(self.S, self.A, self.Z, self.device, self.precision)
        # torch.optim.Adam(info.parameters()) (igdf.py:407), in `ContrastiveInfo.parameters()` order: encoder_sa first
        self.info_optimizer = _PairedAdam("info_optimizer", "encoders", sa=_Adam(self.info.encoder_sa, config["actor_lr"]),
                                          ss=_Adam(self.info.encoder_ss, config["actor_lr"]))
        self._stage, self._stage_key = None, None             # the drawn rows [src(bs) | tar(bs)] the filter reads
        self._w = self._score = self._kept = None             # row weights [N], scores [bs], kept positions [k] of the last step
        self._ictr = torch.zeros(2, dtype=torch.int64, device=self.device)     # [info rng call, info t]
        self._info_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._ibatch, self._isrc, self._info_ws, self._info_key = None, None, None, None
        self._info_graph, self._info_graph_key = None, None

    def _encs(self):
        return (self.info.encoder_sa, self.info.encoder_ss)

    def _extra_named(self):
        o = self.info_optimizer
        return IQL._extra_named(self) + (("info.encoder_sa", self.info.encoder_sa, o.sa), ("info.encoder_ss", self.info.encoder_ss, o.ss))

    def _health_check(self):
        before = self.precision
        IQL._health_check(self)
        if self.precision != before:                          # 'fallback' moved the nets to bf16x3
            self._info_graph = None

    # ------------------------------------------------------------------ training
    def _dims(self, N, Nt, Ng, Ntg):
        bs = self._stage_key
        if self._ws_key != (N, Nt, bs):   # one workspace: IQL's phases carve its front, the encoders' scratch lies behind
            self._ws = ops.igdf_workspace(ops.train_dims(self.S, self.A, N, Nt, N, Nt), bs, self.Z, self.device)
            self._adv = torch.zeros(N, dtype=torch.float32, device=self.device)
            self._ws_key = (N, Nt, bs)
        return ops.train_dims(self.S, self.A, N, Nt, Ng, Ntg), ops.hyper(self.config)

    def _rows(self, bs):
        return kept_rows(bs, self.xi) + bs

    def _buffers(self, bs, N, alloc=False):
        fit = self._batch is not None and self._batch_key == (N,) and self._stage_key == bs
        if alloc and not fit:
            if not 2 <= bs <= MAX_ROWS:
                raise ValueError(f"batch_size {bs} outside [2, {MAX_ROWS}] (the rows the filter's selection takes)")
            self._stage, self._batch = self._rows5(2 * bs), self._rows5(N)
            self._w = torch.zeros(N, dtype=torch.float32, device=self.device)
            self._score = torch.zeros(bs, dtype=torch.float32, device=self.device)
            self._kept = torch.zeros(N - bs, dtype=torch.int32, device=self.device)
            self._stage_key, self._batch_key = bs, (N,)
        return fit

    def _filter(self, bs, k):
        """mobody_igdf_filter: the staged rows -> the training batch and its row weights (igdf.py:494-524)."""
        N = k + bs
        dims, _ = self._dims(N, N, N, N)
        ops.igdf_filter(dims, self.precision, self._encs(), bs, k, self.Z, self.importance_weight, self._stage, self._batch, self._w,
                        self._ws, score_out=self._score, kept_out=self._kept)

    def _critic(self, *args, **kw):
        ops.igdf_critic(*args, row_weight=self._w, **kw)

    def _graph_segments(self, src, tar, batch_size, world, segmented):
        bs = int(batch_size)
        N = self._rows(bs)

        def fused_step():
            self._captured_gather(src, tar, bs, self._stage)
            self._filter(bs, N - bs)
            self._update(self._batch, N, N, dev=True)
        return [fused_step]

    def _draw(self, src, tar, bs, N, writer, log5k):
        """igdf.py:487-524.  Index draws in the reference's order: src, tar."""
        self._gather([src, tar], [bs, bs], self._stage)
        self._filter(bs, N - bs)

    # ------------------------------------------------------------------ the contrastive update (igdf.py:418-447)
    def _info_buffers(self, n):
        if self._info_key != n:
            if not 2 <= n <= MAX_ROWS:
                raise ValueError(f"batch_size {n} outside [2, {MAX_ROWS}] (the rows the contrastive kernel takes)")
            dev, S, A = self.device, self.S, self.A
            s2 = torch.empty(2 * n - 1, S, device=dev)      # [tar s' (n) | src s' (n - 1)]: encoder_ss runs on the stacked rows
            self._ibatch = (torch.empty(n, S, device=dev), torch.empty(n, A, device=dev), s2, torch.empty(n, 1, device=dev),
                            torch.empty(n, 1, device=dev))
            self._isrc = (torch.empty(n - 1, S, device=dev), torch.empty(n - 1, A, device=dev), s2[n:], torch.empty(n - 1, 1, device=dev),
                          torch.empty(n - 1, 1, device=dev))
            self._info_ws = ops.igdf_workspace(ops.train_dims(S, A, n, n), n, self.Z, dev)
            self._info_key, self._info_graph = n, None

    def _info_tar(self):
        b = self._ibatch
        return (b[0], b[1], b[2][:self._info_key], b[3], b[4])

    def _info_step(self, n, dev=False):
        """mobody_igdf_info on the staged rows.  dev: the captured step -- the step count is a device word (already advanced) and
        the last optimizer launch advances the index streams' call word."""
        o, c = self.info_optimizer, self._ictr
        head = (ops.train_dims(self.S, self.A, n, n), self.precision, self._encs(), n, self.Z, self._ibatch, self._info_loss, self._info_ws)
        if self.fused_update:
            if not dev:
                o.t += 1
            ops.igdf_info(*head, opts=((o.sa.m, o.sa.v), (o.ss.m, o.ss.v)), t=o.t, t_dev=c[1:2] if dev else None, lr=o.lr,
                          bump=c[0:1] if dev else None)
            return
        assert not dev, "the captured step is the fused form"
        ops.igdf_info(*head, grads=(o.sa.grad, o.ss.grad))
        o.sa.step()
        o.ss.step()

    def _info_segment(self, src, tar, n):
        """The captured info step: both gathers on index streams of their own (seed ids 106, 107; call id c[0] + 1; the first
        advances the step count c[1]) and the update, whose last optimizer launch advances c[0]."""
        c = self._ictr
        common = dict(call_offsets=[1], counter=c[0:1], S=self.S, A=self.A)

        def info_step():
            ops.gather_batch_rng(buffers=[tar._fields()], counts=[n], seeds=[self._seed_for(106)], sizes=[tar.ptr_size[1:2]],
                                 out=self._info_tar(), bump=(c[1:2],), **common)
            ops.gather_batch_rng(buffers=[src._fields()], counts=[n - 1], seeds=[self._seed_for(107)], sizes=[src.ptr_size[1:2]],
                                 out=self._isrc, **common)
            self._info_step(n, dev=True)
        return info_step

    def _info_graph_step(self, src, tar, n):
        """Replay (capturing first) one info step."""
        key = (n, id(src), id(tar), src.state.data_ptr(), tar.state.data_ptr(), self.precision, self._info_ws.data_ptr())
        if self._info_graph is None or self._info_graph_key != key:
            torch.cuda.synchronize()
            self._ictr[1] = self.info_optimizer.t
            seg = self._info_segment(src, tar, n)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    seg()
            except Exception as exc:
                import warnings
                torch.cuda.synchronize()
                warnings.warn(f"HIP-graph capture of the info step failed ({exc!r}); continuing eagerly")
                self._info_graph, self._no_info_graph = None, True
                return False
            self._info_graph, self._info_graph_key = g, key
        self._info_graph.replay()
        self.info_optimizer.t += 1
        return True

    def update_info(self, src_replay_buffer, tar_replay_buffer, batch_size, writer=None):
        """igdf.py:418-447: `info_update_step` contrastive steps, each on tar(bs) then src(bs - 1), drawn in that order.  The loss
        is read back only on the steps that log ('train/info loss', every 100)."""
        n = int(batch_size)
        if not self._synced:
            self.sync_replicas()
        self._info_buffers(n)
        want = self.use_graph == 1 or (self.use_graph == 2 and n < 4096)
        graph_ok = bool(want and self.rng == "device" and self.fused_update) and not self._no_info_graph
        for info_step in range(1, int(self.config["info_update_step"]) + 1):
            log = writer is not None and info_step % 100 == 0
            if info_step == 1:
                self._health_check()
            if not (graph_ok and info_step > 1 and not log and self._info_graph_step(src_replay_buffer, tar_replay_buffer, n)):
                self._info_graph = None                   # an eager step moves the host-side count
                self._gather([tar_replay_buffer], [n], self._info_tar())
                self._gather([src_replay_buffer], [n - 1], self._isrc)
                self._info_step(n)
            if log:
                writer.add_scalar("train/info loss", float(self._info_loss), info_step)

    def info_loss(self):
        """The loss of the last info step (forces a device sync)."""
        return float(self._info_loss)

    # ------------------------------------------------------------------ checkpoints (igdf.py:555-571)
    def save(self, filename):
        IQL.save(self, filename)                          # the reference's seven files
        torch.save(self.info.state_dict(), filename + "_info")
        torch.save(self.info_optimizer.state_dict(), filename + "_info_optimizer")

    def load(self, filename):
        IQL.load(self, filename)
        self._info_graph = None
        if os.path.exists(filename + "_info"):            # the two files the reference's save leaves out
            self.info.load_state_dict(self._ld(filename, "_info"))
            self.info_optimizer.load_state_dict(self._ld(filename, "_info_optimizer"))
