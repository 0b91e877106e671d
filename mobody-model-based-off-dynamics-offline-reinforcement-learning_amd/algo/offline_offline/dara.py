"""DARA baseline -- host-side mirror of the reference's `algo/offline_offline/dara.py` (class DARA), written from the algorithm.

Same plugin surface as the reference: `DARA(config, device, target_entropy=None)`, `.train(src_rb, tar_rb, batch_size, writer,
wandbrun)`, `.select_action(state, test=True)`, `.update_target()`, `.update_classifier(src_rb, tar_rb, batch_size, writer)`,
`.save/.load(prefix)`, attributes `.classifier .classifier_optimizer .eta` besides IQL's.

What the step is (dara.py:271-324): IQL's step (iql.py of this package) behind two additions.
  1. One domain-classifier update (dara.py:202-223) on a batch of its own, src(bs) | tar(bs) with labels 0 | 1: Gaussian noise of
     `gaussian_noise_std` on the [s | a | s'] rows and, independently, on the [s | a] rows; loss_sas + loss_sa, each
     F.cross_entropy applied to the head's softmax PROBABILITIES; ONE Adam over both heads at actor_lr.  (The reference's randperm
     of the rows is dropped: the loss is a mean over rows and the noise is i.i.d.)
  2. The training batch is drawn, src(bs) then tar(bs), and its source rewards relabeled (dara.py:281-292) from a noise-free
     classifier pass: r += eta * clamp(log p~_sas[1] - log p~_sa[1] - log p~_sas[0] + log p~_sa[0], -10, 10), p~ =
     softmax(head probabilities) + 1e-10, eta = dara_eta if dara_eta != 0 else eta.  (Head probabilities lie in [0, 1], so the
     penalty lies in [-2, 2]: the clamp is kept and never binds.)
Then IQL's V, Q (+ Polyak) and policy phases on [src | tar] with the relabeled rewards.  Each addition is one entry point
(`mobody_dara_classifier`, `mobody_dara_relabel`, csrc/train.hip; seed mode 7 of csrc/mlp_bwd.hip); with rng='device' and the fused
update the whole step -- both gathers, the classifier update, the relabel, IQL's three phases -- replays as one HIP graph, every
counter (the RNG call id, four Adam step counts) a device word.

Where the reference is odd: `save` writes six files and leaves out V, its optimizer and the scheduler -- `save` here
writes them too (as IQL's), `load` reads the six and the three extras when present; its `alpha` property reads a `log_alpha` that
does not exist and is left out.  Not built: data-parallel DARA (refused in the constructor, before any collective).
"""
import torch

from ... import ops
from .iql import IQL
from .mobody import _Adam, _Classifier, _PackedNet, _PairedAdam, refuse_data_parallel, refuse_missing_keys

_KEYS = ("lam", "temp", "max_step", "gaussian_noise_std", "dara_eta")
NOISE_SEED = 31             # seed offset of the classifier-noise streams (as MOBODY.update_classifier)


class _DaraClassifier(_Classifier):
    """Classifier (dara.py:122-144): the two heads as packed nets at the configured MFMA mode."""

    def __init__(self, S, A, device, gaussian_noise_std, lr, precision):
        self.S, self.A, self.device = S, A, device
        self.action_dim, self.gaussian_noise_std = A, float(gaussian_noise_std)
        self.sa_classifier = _PackedNet(S + A, 2, 1, ("sa_classifier.",), device, precision=precision)
        self.sas_classifier = _PackedNet(2 * S + A, 2, 1, ("sas_classifier.",), device, precision=precision)
        self.opt_sa, self.opt_sas = _Adam(self.sa_classifier, lr), _Adam(self.sas_classifier, lr)
        self._calls = 0

    def logits(self, s, a, s2, with_noise, noise_sas=None, noise_sa=None, seed=0, save=False):
        assert not save, "the training path saves inside mobody_dara_classifier"
        self._calls += 1
        std = self.gaussian_noise_std if with_noise else 0.0
        x_sas, x_sa = ops.dara_inputs(s, a, s2, std, noise_sas, noise_sa, seed, self._calls)
        f = lambda net, x: ops.mlp3_forward(net.blob, net.in_dim, 2, 1, x, blob_T=net.blob_T, precision=net.precision)
        return f(self.sas_classifier, x_sas), f(self.sa_classifier, x_sa)

    def __call__(self, state_batch, action_batch, nextstate_batch, with_noise):
        zs, za = self.logits(state_batch, action_batch, nextstate_batch, with_noise)
        return torch.softmax(zs[0], 1), torch.softmax(za[0], 1)


class DARA(IQL):
    def __init__(self, config, device, target_entropy=None):
        # The reference reads these keys without defaults: a MOBODY or an IQL config handed to 'dara' is not a DARA run.  This
        # refusal comes before every other check.
        missing = [k for k in _KEYS if k not in config]
        if not missing and config["dara_eta"] == 0 and "eta" not in config:
            missing = ["eta"]
        refuse_missing_keys("DARA", missing, "config/mujoco/dara/*.yaml values are lam 0.7, temp 3.0, max_step 500000, "
                            "gaussian_noise_std 1.0, eta 0.1, and --dara_eta from the command line")
        refuse_data_parallel("DARA", "dara")
        if not float(config["gaussian_noise_std"]) >= 0.0:
            raise ValueError(f"config['gaussian_noise_std'] = {config['gaussian_noise_std']} < 0")
        if 2 * int(config["state_dim"]) + int(config["action_dim"]) > 256:
            raise ValueError("state_dim, action_dim: the sas classifier's 2 S + A inputs must fit 256 columns")
        IQL.__init__(self, config, device, target_entropy)
        self.eta = float(config["dara_eta"] if config["dara_eta"] != 0 else config["eta"])      # dara.py:164-167
        self.classifier = _DaraClassifier(self.S, self.A, self.device, config["gaussian_noise_std"], config["actor_lr"], self.precision)
        # torch.optim.Adam(classifier.parameters()) (dara.py:192), in `Classifier.parameters()` order: sa_classifier first
        self.classifier_optimizer = _PairedAdam("classifier_optimizer", "heads", sa=self.classifier.opt_sa, sas=self.classifier.opt_sas)
        self._ctr = torch.zeros(5, dtype=torch.int64, device=self.device)      # [rng call, critic t, actor t, V t, classifier t]
        self._cbatch = None                                                    # the classifier's own batch (dara.py:203-204)
        self._cls_loss = torch.zeros(2, dtype=torch.float32, device=self.device)   # (loss_sa, loss_sas) of the last step
        self._pen = torch.zeros(1, dtype=torch.float32, device=self.device)    # mean penalty of a logging step
        self._delta = None

    def _heads(self):
        return (self.classifier.sa_classifier, self.classifier.sas_classifier)

    def _extra_named(self):
        c = self.classifier
        return IQL._extra_named(self) + (("classifier.sa_classifier", c.sa_classifier, c.opt_sa),
                                         ("classifier.sas_classifier", c.sas_classifier, c.opt_sas))

    # ------------------------------------------------------------------ training
    def _dims(self, N, Nt, Ng, Ntg):
        if self._ws_key != (N, Nt):       # one workspace: IQL's phases carve its front, the classifier's scratch lies behind
            self._ws = ops.dara_workspace(ops.train_dims(self.S, self.A, N, Nt, N, Nt), self.device)
            self._adv = torch.zeros(N, dtype=torch.float32, device=self.device)
            self._delta = torch.zeros(N // 2, dtype=torch.float32, device=self.device)
            self._ws_key = (N, Nt)
        return ops.train_dims(self.S, self.A, N, Nt, Ng, Ntg), ops.hyper(self.config)

    def _buffers(self, bs, N, alloc=False):
        fit = IQL._buffers(self, bs, N, alloc)
        if alloc and not fit:
            self._cbatch = self._rows5(N)
        return fit

    def _classifier_step(self, cb, N, dev=False, noise=None):
        """mobody_dara_classifier on the rows `cb`.  dev: the captured step -- the step count and the noise call id are device
        words (already advanced / read with offset 1, as the gathers read theirs)."""
        dims, _ = self._dims(N, N, N, N)
        o, c = self.classifier_optimizer, self._ctr
        kw = dict(seed=self.seed + NOISE_SEED)
        if noise is not None:
            kw.update(noise_sas=noise[0], noise_sa=noise[1])
        if dev:
            kw.update(call_dev=c[0:1], call_offset=1)
        else:
            self.classifier._calls += 1
            kw.update(call=self.classifier._calls)
        head = (dims, self.precision, self._heads(), cb, self.classifier.gaussian_noise_std, self._cls_loss, self._ws)
        if self.fused_update:
            if not dev:
                o.t += 1
            ops.dara_classifier(*head, opts=((o.sa.m, o.sa.v), (o.sas.m, o.sas.v)), t=o.t, t_dev=c[4:5] if dev else None, lr=o.lr, **kw)
            return
        assert not dev, "the captured step is the fused form"
        ops.dara_classifier(*head, grads=(o.sa.grad, o.sas.grad), **kw)
        o.sa.step()
        o.sas.step()

    def update_classifier(self, src_replay_buffer, tar_replay_buffer, batch_size, writer=None, noise=None, rows=None):
        """dara.py:202-228: one classifier step on src(bs) | tar(bs), drawn in that order.  `rows` = (s, a, s2) and `noise` =
        (unit normals [N, 2S+A], [N, S+A]) let a caller supply the batch and the noise; `classifier_noise_fn` (n_rows -> that pair)
        is asked otherwise, and without it the device generator draws."""
        N = 2 * int(batch_size)
        self._buffers(int(batch_size), N, alloc=True)
        cb = self._cbatch
        if rows is None:
            self._gather([src_replay_buffer, tar_replay_buffer], [int(batch_size)] * 2, cb)
        else:
            for dst, x in zip(cb, rows):
                dst.copy_(torch.as_tensor(x, dtype=torch.float32).reshape(dst.shape))
        if noise is None and self.classifier_noise_fn is not None:
            noise = self.classifier_noise_fn(N)
        if noise is not None:
            noise = tuple(torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous() for x in noise)
        self._classifier_step(cb, N, noise=noise)
        if writer is not None and self.total_it % 5000 == 0:
            loss_sa, loss_sas = [float(x) for x in self._cls_loss.tolist()]
            writer.add_scalar("train/sas classifier loss", loss_sas, global_step=self.total_it)
            writer.add_scalar("train/sa classifier loss", loss_sa, global_step=self.total_it)

    def _relabel(self, b, N, log=False):
        dims, _ = self._dims(N, N, N, N)
        ops.dara_relabel(dims, self.precision, self._heads(), b, self.eta, self._ws, delta_out=self._delta if log else None,
                         log_out=self._pen if log else None)

    def _graph_segments(self, src, tar, batch_size, world, segmented):
        b, cb, bs = self._batch, self._cbatch, int(batch_size)
        N = 2 * bs

        def fused_step():
            # both gathers draw with call id c[0] + 1, on index streams of their own; the first advances the classifier's step count,
            # the second the three of IQL's phases
            self._captured_gather(src, tar, bs, cb, seed_ids=(104, 105), bump=(4,))
            self._classifier_step(cb, N, dev=True)
            self._captured_gather(src, tar, bs, b)
            self._relabel(b, N)
            self._update(b, N, N, dev=True)
        return [fused_step]

    def _graph_step(self, src, tar, batch_size):
        if self._graph is None:                           # the capture reads the classifier's count from its device word
            self._ctr[4] = self.classifier_optimizer.t
        if not IQL._graph_step(self, src, tar, batch_size):
            return False
        self.classifier_optimizer.t += 1
        return True

    def _draw(self, src, tar, bs, N, writer, log5k):
        """dara.py:271-292.  Index draws in the reference's order: src, tar (classifier), src, tar (training)."""
        self.update_classifier(src, tar, bs, writer)
        self._gather([src, tar], [bs, bs], self._batch)
        self._relabel(self._batch, N, log=log5k)
        if log5k:
            writer.add_scalar("train/reward penalty", float(self._pen), global_step=self.total_it)

    def classifier_losses(self):
        """(loss_sa, loss_sas) of the last classifier step (forces a device sync)."""
        return tuple(float(x) for x in self._cls_loss.tolist())

    # ------------------------------------------------------------------ checkpoints (dara.py:330-344)
    def save(self, filename):
        IQL.save(self, filename)                          # _critic(_optimizer), _actor(_optimizer) + _value(_optimizer), _actor_lr_scheduler
        torch.save(self.classifier.state_dict(), filename + "_classifier")
        torch.save(self.classifier_optimizer.state_dict(), filename + "_classifier_optimizer")

    def load(self, filename):
        IQL.load(self, filename, optional=("_value", "_actor_lr_scheduler"))     # the three files the reference's save leaves out
        self.classifier.load_state_dict(self._ld(filename, "_classifier"))
        self.classifier_optimizer.load_state_dict(self._ld(filename, "_classifier_optimizer"))
