"""An analytic off-dynamics control task on the device, with true returns.  The reference has no counterpart: its
ground truth is a simulator.  csrc/task.hip steps the task; tests/task_ref.py restates it in fp64.

The task (the specification)
----------------------------
Setup: S >= 3, A >= 1; mu = synthetic.alive_mean(task, S); z = s - mu; u_j = gain_j * clamp(a_j / max_action, -1, 1);
v = z[S-1]; bmat[i][j] = cos(0.7 (i+1)(j+1)) / sqrt(A), formed once on the host in double and rounded to fp32 (the kernel receives
it as a device table: no device cos); d_i = sum_j bmat[i][j] u_j, j ascending.

State update:

    i not in {0, 1, S-1}:  z'_i     = z_i + dt (-f z_i + g d_i + c sin(z_{i-1}))
    forward speed:         z'_{S-1} = v   + dt (-f v + g fwd),   fwd = mean(u_1..u_{A-1}), or u_0 when A == 1
    angle:                 z'_1     = z_1 + dt (lam grav z_1 + g u_0 - k v)
    height:                z'_0     = z_0 + dt (-f z_0 - h grav z_1^2)
    noise:                 z'_i    += sigma * N(0,1)   drawn as rng_normal_at(seed, STREAM_TASK = 4, call, b S + i); sigma == 0 draws nothing
    next = z' + mu
    reward   = z'_{S-1} + alive_bonus - ctrl_cost * mean_j(u_j^2)
    terminal = the existing predicate of `task` on next

Constants (CONSTANTS, INIT_STD, TIME_LIMIT below):

    | constant    | value |
    |-------------|-------|
    | dt          | 0.05  |
    | g           | 2     |
    | c           | 0.5   |
    | lam         | 0.5   |
    | k           | 0.3   |
    | h           | 2     |
    | sigma       | 0.01  |
    | alive_bonus | 1     |
    | ctrl_cost   | 0.1   |
    | start state | mu + 0.05 N(0,1), element b S + i of stream 6 at call id e (the episode's index in its lane) |
    | time limit  | 1000 steps |

Domain parameters: the source has f = grav = 1 and all gains 1.  The target takes its shift from the env suffix and --shift_level:

    | env suffix                      | target parameters                    |
    |---------------------------------|--------------------------------------|
    | -friction L                     | f = L                                |
    | -gravity L                      | grav = L                             |
    | -kinematic easy / medium / hard | gain_0 = 0.75 / 0.5 / 0.25           |
    | -morph easy / medium / hard     | the same gains on actions 1 .. A-1   |
    | any other suffix                | ValueError naming it                 |

Built-in behaviour controllers (data collection, reference points): a_0 = -6 z_1 + 0.15 v, every other action = push; Gaussian
action noise of std eps_a is added (stream 5, element b A + j), then the action is clipped to [-1, 1].

    | controller | push | eps_a |
    |------------|------|-------|
    | medium     | 0.5  | 0.3   |
    | expert     | 1.0  | 0.1   |

`random` draws actions uniformly in [-1, 1); `medium-expert` gives the first half of the lanes to `medium`, the rest to `expert`.

Isolation: evaluation, collection and the online interaction draw from seed ids of their own (SEED_TASK_EVAL, SEED_TASK_COLLECT,
SEED_TASK_ONLINE, next to FQE's 111 and 112) through the device generator; the algorithm's counters, the buffers' `_draws` and torch's generators do not move.
"""
import math
from dataclasses import dataclass

import numpy as np

from . import synthetic

CONSTANTS = dict(dt=0.05, g=2.0, c=0.5, lam=0.5, k=0.3, h=2.0, sigma=0.01, alive_bonus=1.0, ctrl_cost=0.1)
INIT_STD, TIME_LIMIT, LANE_STEPS = 0.05, 1000, 2000
CONTROLLERS = {"medium": (0.5, 0.3), "expert": (1.0, 0.1)}        # name -> (push, eps_a)
SHIFT_GAINS = {"easy": 0.75, "medium": 0.5, "hard": 0.25}
KINDS = ("random", "medium", "expert", "medium-expert")
SEED_TASK_EVAL, SEED_TASK_COLLECT, SEED_TASK_ONLINE = 113, 114, 115    # seed ids (the algorithm classes use 101-110, FQE 111 and 112)
STREAM_NOISE, STREAM_ACTION, STREAM_START, STREAM_POLICY, STREAM_EXPLORE = 4, 5, 6, 11, 12
CTRL_RANDOM, CTRL_FEEDBACK = 0, 1


def bmat(S, A):
    """bmat[i][j] = cos(0.7 (i+1)(j+1)) / sqrt(A) in double, rounded to fp32 once."""
    i, j = np.arange(1, S + 1, dtype=np.float64)[:, None], np.arange(1, A + 1, dtype=np.float64)[None, :]
    return (np.cos(0.7 * i * j) / math.sqrt(A)).astype(np.float32)


@dataclass(frozen=True)
class TaskSpec:
    """One domain of the task: shapes, the termination task's name and the domain parameters."""
    S: int
    A: int
    task: str
    f: float = 1.0
    grav: float = 1.0
    gain: tuple = ()
    max_action: float = 1.0

    @staticmethod
    def from_env(env, shift_level, domain="source"):
        """The source or target domain of `--env` / `--shift_level` (the table above)."""
        if domain not in ("source", "target"):
            raise ValueError(f"domain {domain!r}: 'source' or 'target'")
        S, A, task = synthetic.env_shape(env)
        parts = env.replace("_", "-").split("-")
        suffix = parts[1] if len(parts) > 1 else ""
        f = grav = 1.0
        gain = [1.0] * A
        if suffix in ("friction", "gravity"):
            try:
                level = float(shift_level)
            except (TypeError, ValueError):
                raise ValueError(f"env {env!r}: shift_level {shift_level!r} is not a number") from None
            if domain == "target":
                f, grav = (level, 1.0) if suffix == "friction" else (1.0, level)
        elif suffix in ("kinematic", "morph"):
            if shift_level not in SHIFT_GAINS:
                raise ValueError(f"env {env!r}: shift_level {shift_level!r} is not one of {sorted(SHIFT_GAINS)}")
            if domain == "target":
                for j in ([0] if suffix == "kinematic" else range(1, A)):
                    gain[j] = SHIFT_GAINS[shift_level]
        else:
            raise ValueError(f"env {env!r}: no task shift for the suffix {suffix!r} (friction, gravity, kinematic, morph)")
        return TaskSpec(S, A, task, float(f), float(grav), tuple(gain))


def controller_of(kind, lanes):
    """(ctrl pair, push pair, eps pair, split) of a data type for `lanes` lanes."""
    if kind == "random":
        return (CTRL_RANDOM,) * 2, (0.0, 0.0), (0.0, 0.0), lanes
    if kind == "medium-expert":
        (p0, e0), (p1, e1) = CONTROLLERS["medium"], CONTROLLERS["expert"]
        return (CTRL_FEEDBACK,) * 2, (p0, p1), (e0, e1), lanes // 2
    if kind not in CONTROLLERS:
        raise ValueError(f"data type {kind!r}: one of {KINDS}")
    p, e = CONTROLLERS[kind]
    return (CTRL_FEEDBACK,) * 2, (p, p), (e, e), lanes


class Task(object):
    """A TaskSpec on a device: its tables, the one-step, the data collection and the true return of a policy."""

    def __init__(self, spec, device, seed=0, constants=None):
        import torch
        from . import ops
        from .algo.mb_utils.terminal_funs import get_termination_fn
        self.spec, self.device, self.seed = spec, torch.device(device), int(seed)
        self.constants = dict(CONSTANTS, **(constants or {}))
        S, A = spec.S, spec.A
        if len(spec.gain) != A:
            raise ValueError(f"TaskSpec.gain has {len(spec.gain)} entries for A = {A}")
        self.mu = torch.from_numpy(synthetic.alive_mean(spec.task, S)).to(self.device)
        self.gain = torch.tensor(spec.gain, dtype=torch.float32, device=self.device)
        self.bmat = torch.from_numpy(bmat(S, A)).to(self.device).contiguous()
        self.task_id = get_termination_fn(spec.task).task_id
        self.params = ops.task_params(S, A, self.task_id, self.mu, self.gain, self.bmat, f=spec.f, grav=spec.grav,
                                      max_action=spec.max_action, **self.constants)
        self._eval, self._graph = None, None
        self.eval_captures = 0

    def _seed(self, seed, offset):
        return ((self.seed if seed is None else int(seed)) + offset) & 0xFFFFFFFF

    def start_states(self, n, seed, episode=0):
        """n start states mu + INIT_STD N(0,1): element b S + i of stream 6 at call id `episode`."""
        from . import ops
        eps = ops.rng_normal(seed, STREAM_START, episode, n * self.spec.S, self.device).reshape(n, self.spec.S)
        return self.mu + np.float32(INIT_STD) * eps

    def step(self, obs, act, noise=None, alive=None, seed=None, call=0, call_dev=None, out=None):
        """One step on B rows: dict(next_obs, reward, terminal).  noise [B, S]: explicit unit normals (parity); None: the device
        generator of `seed` at call id call + call_dev[0]."""
        from . import ops
        return ops.task_step(self.params, obs, act, noise=noise, alive=alive, seed=self._seed(seed, 0), call=call, call_dev=call_dev,
                             out=out)

    def collect(self, kind, rows, seed=None, lane_steps=LANE_STEPS, time_limit=TIME_LIMIT):
        """`rows` transitions collected by the built-in controller(s) of data type `kind`, as the dict ReplayBuffer.convert_D4RL
        takes (host arrays): ceil(rows / lane_steps) lanes of `lane_steps` steps, lane after lane, cut to the first `rows` rows."""
        from . import ops
        rows, lane_steps = int(rows), int(lane_steps)
        lanes = max(1, -(-rows // lane_steps))
        ctrl, push, eps, split = controller_of(kind, lanes)
        out = ops.task_collect(self.params, lanes, lane_steps, time_limit, ctrl, push, eps, split, INIT_STD,
                               self._seed(seed, SEED_TASK_COLLECT), call0=1)
        ds = {k: v[:rows].cpu().numpy() for k, v in out.items()}
        ds["terminals"] = ds["terminals"].astype(bool)
        return ds

    def online(self, buffer, lanes=1, time_limit=TIME_LIMIT, expl=0.0, seed=None, rng="device"):
        """An OnlineTask: `lanes` lanes of this task whose transitions the current policy writes into `buffer`."""
        return OnlineTask(self, buffer, lanes, time_limit, expl, seed, rng)

    def evaluate(self, net, head, episodes, horizon=TIME_LIMIT, discount=1.0, chunk=50, rng="device", seed=None, controller=None,
                 init_obs=None):
        """The TRUE return of a policy over `episodes` episodes of at most `horizon` steps (mobody_task_evaluate): head 0 / 1 read
        `net` (a one-member S -> A actor / S -> 2A Gaussian policy, action max_action tanh(mu)); head 2 runs the built-in
        `controller` ('random', 'medium' or 'expert'; `net` is ignored).  A pure function of the policy and the seed: start states,
        process noise and action noise are the device generator's at seed + SEED_TASK_EVAL, call ids 1 .. horizon, so two calls
        with one policy agree bit for bit and two policies meet the same noise.  horizon > chunk > 0 with rng == 'device': the row
        state is initialised, one captured graph of `chunk` steps is replayed horizon // chunk times and the remainder runs eagerly;
        otherwise one eager call.  init_obs [episodes, S]: these start states in the generator's place.  Returns return_mean,
        length_mean, alive_frac (one host read of mobody_eval_summary's words) and the device tensors returns, lengths, alive."""
        import torch
        from . import ops
        head, B, H, chunk = int(head), int(episodes), int(horizon), int(chunk)
        if head not in (0, 1, 2):
            raise ValueError(f"head {head!r}: 0 (deterministic actor), 1 (Gaussian policy) or 2 (built-in controller)")
        if B < 1 or H < 0 or chunk < 0:
            raise ValueError(f"evaluate: episodes {B} must be >= 1, horizon {H} and chunk {chunk} >= 0")
        S, A = self.spec.S, self.spec.A
        ctrl, push, eps = CTRL_FEEDBACK, 0.0, 0.0
        blob = blob_T = None
        precision = 0
        if head == 2:
            (ctrl,), (push,), (eps,) = [x[:1] for x in controller_of(controller, 1)[:3]]
        else:
            want_out = A if head == 0 else 2 * A
            if net.in_dim != S or net.out_dim != want_out or net.members != 1:
                raise ValueError(f"evaluate: head {head}: the policy must be a one-member {S} -> {want_out} net, got {net.in_dim} -> "
                                 f"{net.out_dim} x {net.members}")
            blob, blob_T, precision = net.blob, net.blob_T, net.precision
        sd = self._seed(seed, SEED_TASK_EVAL)
        if self._eval is None or self._eval[0] != B:
            self._eval = (B, ops.eval_state(B, S, self.device), None, torch.zeros(1, dtype=torch.int64, device=self.device),
                          torch.zeros(9, dtype=torch.float32, device=self.device))
            self._graph = None
        _, st, ws, ctr, words = self._eval
        if init_obs is None:
            obs = self.start_states(B, sd)
        else:
            obs = torch.as_tensor(init_obs, dtype=torch.float32).to(self.device).reshape(B, S).contiguous()

        def run(h, call, resume, call_dev=None):
            return ops.task_evaluate(self.params, blob, head, None if resume else obs, h, sd, call, st, discount=discount,
                                     resume=resume, ws=ws, policy_blob_T=blob_T, precision=precision, call_dev=call_dev, ctrl=ctrl,
                                     ctrl_push=push, ctrl_eps=eps)

        call0 = 1
        if chunk == 0 or H <= chunk or rng != "device":
            ws = run(H, call0, False)
        else:
            ws = run(0, call0, False)                         # initialise the row state (sizes the workspace)
            n_full = H // chunk
            ctr.fill_(call0)
            # The key names every pointer and scalar the captured launches bake in.  The row state and the counter word are not
            # in it: they live in self._eval, and self._graph is dropped whenever self._eval is rebuilt (another B) -- keep the two
            # together.  The graph holds `held` alive, so an address in the key is never handed out again while it could replay.
            held = [t for t in (ws, blob, blob_T) if t is not None]
            key = (chunk, head, float(discount), sd, precision, ctrl, push, eps) + tuple(t.data_ptr() for t in held)

            def body():
                run(chunk, 0, True, call_dev=ctr)
                ops.counter_add(ctr, chunk)

            first = 0
            if self._graph is None or self._graph[0] != key:
                self._graph = None
                body()                                        # the first chunk runs eagerly (capturing executes nothing)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body()
                self._graph = (key, g, held)
                self.eval_captures += 1
                first = 1
            for _ in range(n_full - first):
                self._graph[1].replay()
            if H > n_full * chunk:
                run(H - n_full * chunk, call0 + n_full * chunk, True)
        self._eval = (B, st, ws, ctr, words)
        out = dict(returns=st["ret"].clone(), lengths=st["length"].clone(), alive=st["alive"].clone())
        w = ops.eval_summary(st, 1, out=words).cpu()[:8].tolist()      # the one host read
        out.update(return_mean=w[4], length_mean=w[5], alive_frac=w[7])
        return out


class OnlineTask(object):
    """The interaction of the driver's online modes (train_mobody.py:675-770) with a Task: `lanes` parallel lanes whose current
    policy acts, whose transitions go straight into `buffer`'s ring, and whose episode statistics stay on the device until they are
    asked for.  Owns the lanes' state, the counters and the workspace.  interact() is ONE call of mobody_task_interact (3 launches,
    no host read); under rng == 'device' it is a captured graph replayed, with the bits of the eager call.  The buffer's host cache of
    ptr / size advances by the kernel's arithmetic without a device read.  Draws come from seed + SEED_TASK_ONLINE through the device
    generator: torch's and NumPy's generators and the buffers' `_draws` do not move."""

    def __init__(self, task, buffer, lanes=1, time_limit=TIME_LIMIT, expl=0.0, seed=None, rng="device"):
        from . import ops
        lanes, time_limit, expl = int(lanes), int(time_limit), float(expl)
        if buffer.state.shape[0] != buffer.max_size:
            raise ValueError("online: the buffer's storage was replaced by convert_D4RL; an online buffer keeps its max_size ring")
        if not 1 <= lanes <= buffer.max_size:
            raise ValueError(f"online: lanes {lanes} outside [1, max_size {buffer.max_size}]")
        if time_limit < 1 or not expl >= 0.0:
            raise ValueError(f"online: time_limit {time_limit} must be >= 1 and expl {expl} >= 0")
        if (buffer.state_dim, buffer.action_dim) != (task.spec.S, task.spec.A):
            raise ValueError(f"online: the buffer holds {buffer.state_dim} / {buffer.action_dim} wide rows, the task {task.spec.S} / {task.spec.A}")
        self.task, self.buffer, self.lanes, self.time_limit, self.expl, self.rng = task, buffer, lanes, time_limit, expl, rng
        self.seed = task._seed(seed, SEED_TASK_ONLINE)
        self.state = ops.online_state(lanes, task.spec.S, task.device)
        self.state["lane_obs"].copy_(task.start_states(lanes, self.seed))
        self.ws, self._graph = None, None
        self.captures = self.interactions = 0

    def _call(self, net, head):
        from . import ops
        b = self.buffer
        self.ws = ops.task_interact(self.task.params, net.blob, head, b._fields(), b.max_size, b.ptr_size, self.state, self.time_limit,
                                    self.expl, INIT_STD, self.seed, call0=1, ws=self.ws, policy_blob_T=net.blob_T, precision=net.precision)

    def interact(self, net, head):
        """One interaction of `net` (head 0: a one-member S -> A actor; head 1: an S -> 2A Gaussian policy, sampled) on every lane."""
        import torch
        head = int(head)
        S, A = self.task.spec.S, self.task.spec.A
        if head not in (0, 1) or net.in_dim != S or net.out_dim != (A if head == 0 else 2 * A) or net.members != 1:
            raise ValueError(f"interact: head {head}: the policy must be a one-member {S} -> {A if head == 0 else 2 * A} net (head 0 or 1)")
        if self.rng != "device":
            self._call(net, head)
        else:
            # the key names every pointer and scalar the captured launches bake in; the lanes' state, the counters and the workspace
            # live in self and are never replaced, and the graph holds `held` alive
            held = [t for t in (net.blob, net.blob_T, self.buffer.store, self.buffer.ptr_size) if t is not None]
            key = (head, net.precision) + tuple(t.data_ptr() for t in held)
            if self._graph is None or self._graph[0] != key:
                self._graph = None
                self._call(net, head)                     # the first interaction runs eagerly (capturing executes nothing)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._call(net, head)
                self._graph = (key, g, held)
                self.captures += 1
            else:
                self._graph[1].replay()
        b = self.buffer                                   # k_task_commit's arithmetic on the host cache: no device read
        b._ptr = (b._ptr + self.lanes) % b.max_size
        b._size = min(b._size + self.lanes, b.max_size)
        self.interactions += 1

    def episode_stats(self):
        """The one host read: dict(episodes, return_mean, length_mean) over the episodes finished since the last call (the means are
        None when there are none); the per-lane accumulators are added in lane order and cleared."""
        import torch
        st = self.state
        words = torch.stack([st["done_count"].double(), st["ret_sum"].double(), st["len_sum"].double()]).cpu().numpy()
        n = int(words[0].sum())
        for k in ("done_count", "ret_sum", "len_sum"):
            st[k].zero_()
        if n == 0:
            return dict(episodes=0, return_mean=None, length_mean=None)
        ret = 0.0
        for x in words[1]:
            ret += float(x)
        return dict(episodes=n, return_mean=ret / n, length_mean=float(words[2].sum()) / n)
