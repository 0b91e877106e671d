"""CLI driver -- mirror of the reference's `train_mobody.py` for mode 3 (offline-offline): `--policy MOBODY` and the model-free
baselines `--policy TD3_BC` and `--policy IQL` (no ensemble dynamics is built, loaded or trained for them, train_mobody.py:820;
`--max_step` is also T_max of IQL's cosine schedule).  With `--synthetic 2` the model-free baselines also run the reference's
online modes in the analytic task: `--mode 1` (offline source data, one target interaction every
`tar_env_interact_interval` steps, :675-722) and `--mode 2` (online source with exploration noise, offline target, :723-770).

Accepts the reference's flags with the same names, types and defaults (train_mobody.py:210-307),
merges configuration in the same precedence (yaml <- --params JSON <- CLI-derived keys, :407-416,
:470-531) and runs the same sequence: seed -> build policy via call_algo -> build buffers -> build
dynamics -> attach -> `policy.train(...)` loop (:927-928).

Simulators (gym / mujoco-py / d4rl) and datasets are not part of this build: `--synthetic 1` (the
default when gym/d4rl are not importable) fills the replay buffers with synthetic MuJoCo-shaped
transitions and random-initialised networks and skips simulator evaluation; `--synthetic 0` trains on real
offline datasets without the simulators: `--src_data` (an .npz in d4rl.qlearning_dataset's layout) and `--tar_data` (the
ODRL target file: .npz of its raw arrays, or the .hdf5 itself when h5py is importable; default: the reference's
`dataset/<domain>/<env>_<shift>_<quality>.hdf5` path), ingested exactly as train_mobody.py:548-557 does.  The ensemble
dynamics follows the reference's load-or-train branches (`build_dynamics`, train_mobody.py:817-877): load
`--dynamics_path` / the default `pretrained_dynamics/<env>/srcdatatype-...` tree when present and `--train_dynamics 0`,
otherwise `MOBODYEnsembleDynamics.train` on the two buffers, then save in the reference's directory scheme.  A random
"alive" ensemble is kept only under an explicit `--synthetic 1` with nothing to load.  `--synthetic 2` is the analytic
off-dynamics control task (mobody_amd/task.py): both buffers are filled with episodes collected in the task's source
and shifted target domain (`--srctype` / `--tartype`: random, medium, expert, medium-expert), the dynamics takes the ordinary
load-or-train branches, and at every `eval_freq` the policy is rolled through the TRUE task and the reference's own scalars
`test/source return` / `test/target return` are written.

Several GPUs: started once per GPU (`python -m mobody_amd.dp --gpus N -- <arguments>`, or `python -m torch.distributed.run
--nproc-per-node N train_mobody.py <arguments>`) every process becomes one data-parallel rank (`dp.init_from_env`): same
arguments and seed everywhere, replicated buffers and weights, sharded minibatches / refresh / pre-training batches, and ONE
set of outputs (log, prints, checkpoints, saved dynamics) written by rank 0.  There is no flag for it: the rank count comes
from the launcher's environment, and without WORLD_SIZE nothing below differs from the single-process run.
"""
import argparse
import json
import os
import random
import time

import numpy as np
import torch
import yaml

# (flag, default, type or None for strings / store_true marker)
_FLAGS = [
    ("--dir", "./logs", None), ("--policy", "SAC", None), ("--env", "halfcheetah-friction", None),
    ("--srctype", "medium", None), ("--tartype", "medium", None), ("--shift_level", 0.1, None),
    ("--mode", 3, int), ("--seed", 0, int), ("--save-model", False, "store_true"),
    ("--tar_env_interact_interval", 10, int), ("--max_step", int(1e6), int), ("--params", None, None),
    ("--purely_model_based", 0, int), ("--num_envs", 32, int), ("--eval_freq", 1000, int), ("--dara_eta", 0, float),
    ("--only_use_trg_transition", 5e4, int), ("--transition_update_freq", 2500, int),
    ("--transition_update_start", 5e4, int), ("--trg_rollout_batch_size", 5e4, int), ("--trg_rollout_length", 1, int),
    ("--src_rollout_batch_size", 5e4, int), ("--src_rollout_length", 1, int), ("--model_based_training_steps", 100, int),
    ("--fake_batch_scale", 0.5, float), ("--dynamics_lr", 1e-3, float), ("--encoder_loss_coef", 1, float),
    ("--domain_loss_coef", 0.0, float), ("--cycle_loss_coef", 0.3, float), ("--bc_coef", 1.0, float),
    ("--q_weighted", 1, int), ("--advantage", 0, int), ("--scale_q", 1, int), ("--mobile", 0, int),
    ("--relu_reward", 0, int), ("--penalize_fake", 0, int), ("--gaussian_dynamics", 0, int),
    ("--sep_reward_dynamics", 0, int), ("--vae", 0, int), ("--sas_reward", 0, int), ("--inverse", 0, int),
    ("--inverse_sep_reward_loss", 0, int), ("--latent_reward", 0, int), ("--filter_bad_rollout", 1, int),
    ("--train_together", 0, int), ("--encode_sa", 0, int), ("--vae_a", 0, int), ("--train_with_src_threshold", 1, float),
    ("--env_filter", 10, float), ("--use_src_sa_to_get_target_next_state", 1, int), ("--env_penalty_coef", 0.1, float),
    ("--lcb_penalty_coef", 0, float), ("--rollout_length", 1, int), ("--rollout_from_src", 0, int),
    ("--rollout_from_src_length", 2, int), ("--trg_ratio", 1, float), ("--src_ratio", 1, float),
    ("--dynamics_path", None, str), ("--train_dynamics", 0, int), ("--out_dir_remark", "", str),
    ("--penalty_type", "par", str), ("--penalty_coef", 0.1, float), ("--representation_noise", 0, float),
    ("--group", None, str), ("--wandb", 1, int), ("--cat", 0, int), ("--no_vae", 0, int), ("--trg_only", 0, int),
    ("--mopo", 0, int),
]


def build_parser():
    p = argparse.ArgumentParser()
    for flag, default, typ in _FLAGS:
        if typ == "store_true":
            p.add_argument(flag, action="store_true")
        elif typ is None:
            p.add_argument(flag, default=default)
        else:
            p.add_argument(flag, default=default, type=typ)
    # additions of this build (not in the reference)
    p.add_argument("--synthetic", default=None, type=int, help="1: synthetic buffers/networks (no gym/d4rl needed); 2: the analytic control task (data + true returns)")
    p.add_argument("--rng", default="numpy", choices=["numpy", "device"], help="index/elite RNG: reference NumPy stream or device Philox")
    p.add_argument("--src_rows", default=int(1e6), type=int)
    p.add_argument("--tar_rows", default=5000, type=int)
    p.add_argument("--log_every", default=1000, type=int)
    p.add_argument("--dynamics_max_epochs", default=None, type=int, help="cap on pre-training epochs (reference: until early stopping)")
    p.add_argument("--scalars", default=1, type=int, help="1: write the writer.add_scalar stream to <outdir>/tb/scalars.csv")
    p.add_argument("--src_data", default=None, help="--synthetic 0: source transitions (.npz in d4rl.qlearning_dataset layout)")
    p.add_argument("--tar_data", default=None, help="--synthetic 0: target ODRL dataset (.npz of its raw arrays, or the .hdf5 itself "
                                                     "when h5py is importable); default: the reference's dataset/<domain>/... path")
    return p


class ScalarLog:
    """The `writer` the reference hands to policy.train / dynamics.train (a tensorboard SummaryWriter,
    train_mobody.py:455-458): same add_scalar(tag, value, global_step) surface, rows appended to a CSV file (tensorboard is
    not part of this image).  Values may be device tensors; they are read when the row is written."""

    def __init__(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        self.path = path
        self.f = open(path, "w")
        self.f.write("tag,step,value\n")

    def add_scalar(self, tag, scalar_value, global_step=None, *_, **__):
        v = float(scalar_value.item() if hasattr(scalar_value, "item") else scalar_value)
        self.f.write(f"{tag},{-1 if global_step is None else int(global_step)},{v!r}\n")

    def flush(self):
        self.f.flush()

    def close(self):
        self.f.close()


class NullLog:
    """The writer of every rank but 0: same surface, drops what it is given.  It must not be `None` -- MOBODY.train runs its
    logging steps eagerly and only when it has a writer, and all ranks have to take the same eager-or-replay decision on
    every step (the two paths issue their collectives differently)."""

    def add_scalar(self, *_, **__):
        pass

    flush = close = add_scalar


def load_datasets(args):
    """The two offline datasets of the real-data mode without simulators: the source transitions the reference takes from
    d4rl.qlearning_dataset (train_mobody.py:548-552) come from an .npz file with the same keys, the target transitions from
    the ODRL file through dataset/call_dataset.py's transformation (:553-557)."""
    from mobody_amd.dataset import call_dataset
    if args.src_data is None:
        raise NotImplementedError("--synthetic 0 without simulators needs --src_data FILE.npz (observations, actions, "
                                  "next_observations, rewards, terminals: d4rl.qlearning_dataset's keys); d4rl itself is not in this image")
    with np.load(args.src_data) as z:
        src = {k: z[k] for k in ("observations", "actions", "next_observations", "rewards", "terminals")}
    if args.tar_data is not None and args.tar_data.endswith(".npz"):
        with np.load(args.tar_data) as z:
            tar = call_dataset.transitions_from_arrays({k: z[k] for k in z.files})
    elif args.tar_data is not None:
        tar = call_dataset.transitions_from_hdf5(args.tar_data)
    else:
        tar = call_dataset.call_tar_dataset(args.env, args.shift_level, args.tartype)
    return src, tar


def domain_of(env):
    """train_mobody.py:314-321."""
    if "halfcheetah" in env or "hopper" in env or "walker2d" in env or env.split("-")[0] == "ant":
        return "mujoco"
    if "pen" in env or "relocate" in env or "door" in env or "hammer" in env:
        return "adroit"
    if "antmaze" in env:
        return "antmaze"
    raise NotImplementedError


# hyper-parameters of the reference's config/mujoco/<policy>/*.yaml, used when no config tree is present: its four files per
# policy are identical (mobody's except for eval_freq); tests/golden/g23_td3bc_configs.json holds td3_bc's
_BUILTIN_YAML = {
    "mobody": dict(alpha=0.2, batch_size=128, actor_lr=0.0003, critic_lr=0.0003, gamma=0.99, state_dim=17, action_dim=3,
                   hidden_sizes=256, max_action=1, gaussian_noise_std=1.0, eta=0.1, temperature_opt=False, tau=0.005,
                   update_interval=2, expl_noise=0.2, eval_episode=10, eval_freq=2500, start_steps=5000, max_step=500000,
                   device="cuda", save_freq=5000, lam=0.7, temp=3.0, weight=2.5),
    "td3_bc": dict(batch_size=128, actor_lr=0.0003, critic_lr=0.0003, gamma=0.99, state_dim=17, action_dim=3, hidden_sizes=256,
                   max_action=1, tau=0.005, update_interval=2, expl_noise=0.2, eval_episode=10, eval_freq=10000,
                   start_steps=5000, max_step=500000, device="cuda", weight=2.5, save_freq=5000),
}


# `iql`'s, kept beside the table: load_yaml stays the reference's file lookup for it (no config tree, no file), build_config falls
# back to these values; tests/golden/g24_iql_configs.json holds the reference's four files
_BUILTIN_IQL = dict(ac_gradient_clip=100, alpha=0.2, batch_size=128, actor_lr=0.0003, critic_lr=0.0003, gamma=0.99,
                max_epochs_since_update_decay_interval=150000.0, state_dim=17, action_dim=3, hidden_sizes=256, max_action=1,
                temperature_opt=False, tau=0.005, update_interval=2, expl_noise=0.2, eval_episode=10, eval_freq=10000,
                start_steps=5000, max_step=500000, tar_env_interact_freq=10, device="cuda", lam=0.7, temp=3.0, save_freq=5000)


def uses_model(policy):
    """The ensemble dynamics is built, loaded or trained only for model-based policies (train_mobody.py:820)."""
    return "mb" in policy.lower() or "mobody" in policy.lower()


def load_yaml(domain, policy, env_base):
    """config/<domain>/<policy>/<env>.yaml next to the script (train_mobody.py:410-411); a built-in copy of the mujoco
    hyper-parameters of `mobody` and `td3_bc` is used when no config tree is present.  With $MOBODY_CONFIG_ROOT set,
    $MOBODY_CONFIG_ROOT/<domain>/<policy>/<env>.yaml is looked up first (a reference checkout's config/ directory: the only
    source of `dara`'s, `igdf`'s and `bosa`'s hyper-parameters); unset, nothing changes."""
    root = os.environ.get("MOBODY_CONFIG_ROOT")
    if root:
        path = os.path.join(root, domain, policy, env_base + ".yaml")
        if os.path.exists(path):
            with open(path, "r", encoding="utf-8") as f:
                return yaml.safe_load(f)
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.path.join(here, "config", domain, policy, env_base + ".yaml")
    if os.path.exists(path):
        with open(path, "r", encoding="utf-8") as f:
            return yaml.safe_load(f)
    if policy not in _BUILTIN_YAML or domain != "mujoco":
        raise FileNotFoundError(path)             # same failure as the reference for configs it does not ship
    return dict(_BUILTIN_YAML[policy])


def build_config(args, state_dim, action_dim, max_action):
    """yaml <- --params <- CLI keys (train_mobody.py:407-416, 470-531); env dims override the yaml's."""
    domain = domain_of(args.env)
    try:
        config = load_yaml(domain, args.policy.lower(), args.env.split("-")[0])
    except FileNotFoundError:
        if args.policy.lower() != "iql" or domain != "mujoco":
            raise
        config = dict(_BUILTIN_IQL)                   # the reference's config/mujoco/iql/*.yaml (its four files are identical)
    if args.params is not None:
        config.update(json.loads(args.params))
    shift = args.shift_level
    if domain == "mujoco" and shift not in ("easy", "medium", "hard"):
        shift = float(shift)
    a = args
    config.update({
        "env_name": a.env, "state_dim": state_dim, "action_dim": action_dim, "max_action": max_action,
        "tar_env_interact_interval": int(a.tar_env_interact_interval), "max_step": int(a.max_step), "shift_level": shift,
        "dara_eta": a.dara_eta, "only_use_trg_transition": a.only_use_trg_transition,
        "transition_update_freq": a.transition_update_freq, "transition_update_start": a.transition_update_start,
        "trg_rollout_batch_size": int(a.trg_rollout_batch_size), "trg_rollout_length": int(a.trg_rollout_length),
        "src_rollout_batch_size": int(a.src_rollout_batch_size), "src_rollout_length": int(a.src_rollout_length),
        "model_based_training_steps": a.model_based_training_steps, "fake_batch_scale": a.fake_batch_scale,
        "env_penalty_coef": a.env_penalty_coef, "lcb_penalty_coef": a.lcb_penalty_coef,
        "encoder_loss_coef": a.encoder_loss_coef, "domain_loss_coef": a.domain_loss_coef,
        "cycle_loss_coef": a.cycle_loss_coef,
        "use_src_sa_to_get_target_next_state": a.use_src_sa_to_get_target_next_state,
        "penalty_type": a.penalty_type, "penalty_coef": a.penalty_coef, "rollout_length": a.rollout_length,
        "penalize_fake": a.penalize_fake, "representation_noise": a.representation_noise, "eval_freq": a.eval_freq,
        "bc_coef": a.bc_coef, "rollout_from_src": a.rollout_from_src, "rollout_from_src_length": a.rollout_from_src_length,
        "env_filter": a.env_filter, "trg_ratio": a.trg_ratio, "src_ratio": a.src_ratio, "q_weighted": a.q_weighted,
        "advantage": a.advantage, "scale_Q": a.scale_q, "inverse_sep_reward_loss": a.inverse_sep_reward_loss,
        "latent_reward": a.latent_reward, "filter_bad_rollout": a.filter_bad_rollout, "train_together": a.train_together,
        "train_with_src_threshold": a.train_with_src_threshold, "no_vae": a.no_vae, "trg_only": a.trg_only,
        "mopo": a.mopo,
    })
    config["rng"], config["seed"] = a.rng, a.seed
    return config


def episode_starts(observations, next_observations, terminals):
    """Row indices at which an episode of a transition dataset starts (pure NumPy): row 0, every row after a terminal
    one, and every row whose observation is not the row before's next observation (a time-limit cut or a joined file)."""
    obs, nxt = np.asarray(observations), np.asarray(next_observations)
    n = obs.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    term = np.asarray(terminals).reshape(-1).astype(bool)
    start = np.ones(n, dtype=bool)
    start[1:] = term[:-1] | np.any(nxt[:-1] != obs[1:], axis=1)
    return np.flatnonzero(start)


def model_eval_rows(starts, episodes, seed):
    """`episodes` rows out of `starts` for the evaluation in the model, from a seeded generator of its own (never the global
    one): distinct starts while there are enough, drawn with replacement when there are fewer starts than episodes."""
    starts = np.asarray(starts, dtype=np.int64)
    if starts.size == 0:
        raise ValueError("model_eval_rows: the dataset has no row to start an episode from")
    rng = np.random.default_rng([int(seed), 0x4D45])
    if starts.size >= episodes:
        return np.sort(rng.choice(starts, size=episodes, replace=False))
    return rng.choice(starts, size=episodes, replace=True)


OPEN_LOOP_STEPS = (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000)      # window steps whose error is logged (plus the horizon)


def open_loop_windows(starts, n_rows, horizon, count, seed):
    """`count` window starts for the open-loop model error (pure NumPy): a start i is valid iff the `horizon` rows
    i .. i + horizon - 1 exist and belong to one episode, i.e. i + horizon <= n_rows and no episode start lies in
    (i, i + horizon).  Distinct valid starts, sorted, from a seeded generator of its own (never the global one, and not
    model_eval_rows's); all of them when there are fewer than `count`; ValueError naming the longest run of contiguous
    rows when there is none."""
    starts = np.asarray(starts, dtype=np.int64)
    n_rows, horizon = int(n_rows), int(horizon)
    if horizon < 1:
        raise ValueError(f"open_loop_windows: horizon {horizon} must be at least 1")
    is_start = np.zeros(n_rows + 1, dtype=np.int64)
    is_start[starts[starts < n_rows]] = 1
    inside = np.cumsum(is_start)                                 # inside[j] = episode starts in [0, j]
    i = np.arange(max(n_rows - horizon + 1, 0), dtype=np.int64)
    valid = i[inside[i + horizon - 1] - inside[i] == 0]          # none in (i, i + horizon)
    if valid.size == 0:
        edges = np.unique(np.concatenate([[0], starts[starts < n_rows], [n_rows]]))
        longest = int(np.max(np.diff(edges))) if n_rows > 0 else 0
        raise ValueError(f"open_loop_windows: no window of {horizon} contiguous rows in the {n_rows} rows of the dataset "
                         f"(the longest run of contiguous rows is {longest})")
    if valid.size <= count:
        return valid
    rng = np.random.default_rng([int(seed), 0x4F4C])
    return np.sort(rng.choice(valid, size=int(count), replace=False))


def dynamics_save_path(args, root):
    """`<root>/<env>/srcdatatype-<src>-tardatatype-<tar>-<shift>` (train_mobody.py:822-823, 843-844)."""
    return os.path.join(root, args.env, f"srcdatatype-{args.srctype}-tardatatype-{args.tartype}-{args.shift_level}")


def build_dynamics(args, dynamics, model, src_rb, tar_rb, writer, task, explicit_synthetic, rank=0, world=1):
    """The reference's load-or-train logic for the ensemble dynamics (train_mobody.py:817-877), branch for branch:

    * `--dynamics_path P --train_dynamics 0`: load `P/<env>/srcdatatype-...` when that directory exists, otherwise train on
      the two buffers and save there (:819-840);
    * otherwise the default tree `pretrained_dynamics/<env>/srcdatatype-...` is tried: loaded when it exists and
      `--train_dynamics 0` (a failing load falls through to training, :848-864), else the model is trained
      (`dynamics.train(src_all, trg_all, writer=writer, buffer=[src, tar])`) and saved -- under `--dynamics_path` when
      one is given, under the default tree when not (:865-877).

    The one addition of this build: with an EXPLICIT `--synthetic 1`, no `--dynamics_path` and nothing in the default tree,
    `--train_dynamics 0` keeps a random-initialised ensemble whose transition head is shifted into the task's alive box (benchmarks and smoke runs on
    synthetic buffers; there is nothing to learn from them).  Returns 'loaded' / 'trained' / 'random'.

    Data parallel (`world` > 1): every rank takes the SAME branch.  What the branch depends on the filesystem for (does the
    directory exist, does the load succeed) is evaluated by rank 0 alone and broadcast; a branch the flags alone decide
    (`--train_dynamics 1`) needs no exchange, so `dynamics.train` -- sharded over the ranks, and the first thing it does is refuse
    what data parallel does not support -- is reached before any collective.  Rank 0 writes; the others wait at a barrier
    until the files are there."""
    from mobody_amd import synthetic

    def agree(decide):
        """rank 0's decide() -> True / False on every rank."""
        if world == 1:
            return decide()
        flag = torch.tensor([int(decide()) if rank == 0 else 0], dtype=torch.int64, device=model.device)
        torch.distributed.broadcast(flag, 0)
        return bool(flag.item())

    def try_load(save_path):
        try:
            dynamics.load(save_path)
            return True
        except Exception:                                                      # the reference's bare `except:` (:851)
            return False

    def loaded(save_path, rank0_has_it=False):
        if rank != 0 or not rank0_has_it:
            dynamics.load(save_path)
        if rank == 0:
            print("----------pretrained dynamics loaded----------")
        return "loaded"

    def train_and_save(save_path):
        if explicit_synthetic:
            synthetic.alive_dynamics(model, task)          # synthetic buffers only: start inside the alive box
        dynamics.optim = type("Opt", (), {"param_groups": [{"lr": args.dynamics_lr}]})()
        dynamics.train(src_rb.sample_all(), tar_rb.sample_all(), writer=writer, buffer=[src_rb, tar_rb],
                       max_epochs=args.dynamics_max_epochs)
        if args.dynamics_path is not None:                                     # :831-836, 855-860, 867-872
            save_path = dynamics_save_path(args, args.dynamics_path)
        if rank == 0:
            os.makedirs(save_path, exist_ok=True)
            dynamics.save(save_path)
            print(f"----------dynamics trained and saved to {save_path}----------")
        if world > 1:
            torch.distributed.barrier()
        return "trained"

    if args.dynamics_path is not None and args.train_dynamics == 0:            # :819-840
        save_path = dynamics_save_path(args, args.dynamics_path)
        if agree(lambda: os.path.exists(save_path)):
            return loaded(save_path)
        return train_and_save(save_path)
    save_path = dynamics_save_path(args, "pretrained_dynamics")                # :842-846
    if args.train_dynamics == 0 and agree(lambda: os.path.exists(save_path)):
        if agree(lambda: try_load(save_path)):                                 # a failing load falls through to training
            return loaded(save_path, rank0_has_it=True)
        return train_and_save(save_path)
    if explicit_synthetic and args.train_dynamics == 0:
        synthetic.alive_dynamics(model, task)
        if rank == 0:
            print("--synthetic 1: nothing to load, random-initialised ensemble dynamics (pass --train_dynamics 1 to pre-train it)")
        return "random"
    return train_and_save(save_path)


ONLINE_POLICIES = ("td3_bc", "iql", "dara", "igdf", "bosa")
ONLINE_EXPL_NOISE = 0.2                               # mode 2: + np.random.normal(0, max_action * 0.2) (train_mobody.py:733-735)


def check_mode(args, environ=None):
    """Refuse, with a SystemExit that names the reason and before any GPU work, what the online modes (1: offline-online,
    2: online-offline) are not built for.  Mode 3 passes untouched."""
    if args.mode == 3:
        return
    if args.mode == 0:
        raise SystemExit("--mode 0 (online-online): its SAC is not in the reference tree (call_tune_algo.py:8); nothing to mirror")
    if args.mode not in (1, 2):
        raise SystemExit(f"--mode {args.mode}: 1 (offline-online), 2 (online-offline) or 3 (offline-offline)")
    if args.synthetic != 2:
        raise SystemExit(f"--mode {args.mode} needs an environment to interact with: the analytic task, --synthetic 2 (simulators are not part of this build)")
    if uses_model(args.policy):
        raise SystemExit(f"--mode {args.mode} --policy {args.policy}: the reference builds the dynamics only in its mode-3 branch "
                         "(train_mobody.py:771-877), and an online buffer holds no data to pre-train it on")
    if args.policy.lower() not in ONLINE_POLICIES:
        raise SystemExit(f"--mode {args.mode} --policy {args.policy}: the online modes are built for TD3_BC, IQL, DARA, IGDF and BOSA")
    env = os.environ if environ is None else environ
    if int(env.get("WORLD_SIZE", "1") or 1) > 1:
        raise SystemExit(f"--mode {args.mode}: the online modes run on one GPU (a process group of more than one rank is not supported)")
    from mobody_amd import synthetic
    state_dim, action_dim, _ = synthetic.env_shape(args.env)
    config = build_config(args, state_dim, action_dim, 1.0)
    if args.policy.lower() == "bosa" and not config.get("critic_actor"):
        raise SystemExit(f"--mode {args.mode} --policy BOSA: the actor that interacts exists only with config['critic_actor'] set")
    if args.mode == 1:
        bad = sorted(k for k, v in config.items() if k.startswith(("model_eval_", "model_error_", "fqe_")) and v)
        if bad:
            raise SystemExit(f"--mode 1: {', '.join(bad)}: these evaluators start from episode starts of target data chosen once at "
                             "start-up, and the target buffer starts empty")
    if int(config.get("online_lanes", 1)) < 1:
        raise SystemExit(f"--mode {args.mode}: online_lanes {config.get('online_lanes')} must be at least 1")


def main(argv=None):
    args = build_parser().parse_args(argv)
    if "_" in args.env:
        args.env = args.env.replace("_", "-")
    check_mode(args)                                  # the refusals of the online modes come before any GPU work
    from mobody_amd import dp
    rank, world, device = dp.init_from_env()          # one data-parallel rank per process when a launcher set WORLD_SIZE
    try:
        return _run(args, rank, world, device)
    finally:
        dp.shutdown()


def _run(args, rank, world, device):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    from mobody_amd.algo.dynamics.mobody_dynamics import MOBODYEnsembleDynamics
    from mobody_amd.algo.dynamics.mobody_module import MOBODYModule
    from mobody_amd.algo.mb_utils.terminal_funs import get_termination_fn

    say = print if rank == 0 else (lambda *a, **k: None)           # one set of prints
    synthetic_mode = args.synthetic
    if synthetic_mode is None:
        try:
            import d4rl  # noqa: F401
            import gym  # noqa: F401
            synthetic_mode = 0
        except Exception:
            synthetic_mode = 1
    state_dim, action_dim, task = synthetic.env_shape(args.env)
    src_ds = tar_ds = None
    if not synthetic_mode:
        src_ds, tar_ds = load_datasets(args)
        if src_ds["observations"].shape[1] != state_dim or src_ds["actions"].shape[1] != action_dim:
            raise ValueError(f"--src_data has shapes {src_ds['observations'].shape[1]}/{src_ds['actions'].shape[1]}, "
                             f"env {args.env} expects {state_dim}/{action_dim}")
    max_action = 1.0
    task_src = task_tar = None
    if synthetic_mode == 2:
        # the analytic control task: an unknown shift suffix ends the run here.  Every rank builds the same data from the seed.
        from mobody_amd.task import Task, TaskSpec
        task_src = Task(TaskSpec.from_env(args.env, args.shift_level, "source"), device, seed=args.seed)
        task_tar = Task(TaskSpec.from_env(args.env, args.shift_level, "target"), device, seed=args.seed)
    # the same seed on every rank: the mirror folds the rank into its device-RNG seeds (dp.rank_salt) and broadcasts rank 0's
    # replica before the first step (sync_replicas), and every rank builds the same buffers
    torch.manual_seed(args.seed); np.random.seed(args.seed); random.seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)
    config = build_config(args, state_dim, action_dim, max_action)
    if world > 1 and int(config.get("shard_refresh", 1)):
        # each rank appends 1 / world of the refresh's rows: a ring of 1 / world of the reference's capacity keeps rollouts
        # as long as the reference does
        config["fake_buffer_size"] = -(-int(1e6) // world)
    env_penalty_coef = 0.0 if args.mobile == 1 else args.env_penalty_coef
    say("-" * 60 + f"\nPolicy: {args.policy}, Env: {args.env}, Seed: {args.seed}\n" + "-" * 60)

    terminal_fn = get_termination_fn(task)
    policy = call_algo(args.policy, config, args.mode, device, terminal_fn=terminal_fn)
    if hasattr(policy, "max_train_steps") and int(config["max_step"]) > policy.max_train_steps():
        # BOSA without config['critic_actor']: only the VAE stage runs; refuse the run now, not after vae_iteration // 2 steps of
        # training (with the key there is no bound)
        raise SystemExit(f"--policy {args.policy}: --max_step {config['max_step']} runs past the VAE stage (vae_iteration "
                         f"{config['vae_iteration']}); the critic / actor stage is not built: the largest max_step is "
                         f"{policy.max_train_steps()}")
    src_rb = utils.ReplayBuffer(state_dim, action_dim, device, rng=args.rng, seed=args.seed + 1)
    tar_rb = utils.ReplayBuffer(state_dim, action_dim, device, rng=args.rng, seed=args.seed + 2)
    data_returns = None
    if synthetic_mode == 2:
        # lanes of 2000 steps under the data type's controller(s), the first `rows` rows kept; seeds of their own per domain
        # (online modes: the buffer the policy fills by interacting starts EMPTY at max_size -- the target's in mode 1, the source's
        # in mode 2 -- and nothing is collected for it)
        src_ds = task_src.collect(args.srctype, args.src_rows, seed=args.seed + 1) if args.mode != 2 else None
        tar_ds = task_tar.collect(args.tartype, args.tar_rows, seed=args.seed + 2) if args.mode != 1 else None
        for rb, d in ((src_rb, src_ds), (tar_rb, tar_ds)):
            if d is not None:
                rb.convert_D4RL(d)
        data_returns = tuple(None if d is None else float(np.mean(np.add.reduceat(
            np.asarray(d["rewards"], np.float64).reshape(-1), episode_starts(d["observations"], d["next_observations"], d["terminals"]))))
                             for d in (src_ds, tar_ds))
        told = ["online" if r is None else f"{k}, mean episode return {r:.1f}" for k, r in zip((args.srctype, args.tartype), data_returns)]
        say(f"task data: {src_rb.size} source ({told[0]}) / {tar_rb.size} target ({told[1]}) transitions")
        src_ds = tar_ds = None
    elif synthetic_mode:
        synthetic.fill_buffer(src_rb, args.src_rows, task, args.seed)
        synthetic.fill_buffer(tar_rb, args.tar_rows, task, args.seed + 100)
    else:                                             # train_mobody.py:548-557: both buffers adopt their datasets
        src_rb.convert_D4RL(src_ds)
        tar_rb.convert_D4RL(tar_ds)
        say(f"datasets: {src_rb.size} source / {tar_rb.size} target transitions")

    # Open-loop error of the learned target model over recorded target trajectories: two optional keys of the merged config,
    # off by default.  Rank 0 measures.  The windows are chosen once, here, before any model is built or trained: a horizon
    # longer than every episode of the target data ends the run now, not at the first evaluation.
    ol_rows, ol_h = None, int(config.get("model_error_horizon", 0))
    if ol_h > 0:
        if not uses_model(args.policy):
            say(f"model_error_horizon / model_error_windows ignored: {args.policy} has no model to measure")
        elif rank == 0:
            n = tar_rb.size
            term = 1.0 - tar_rb.not_done[:n].cpu().numpy()
            ol_rows = open_loop_windows(episode_starts(tar_rb.state[:n].cpu().numpy(), tar_rb.next_state[:n].cpu().numpy(), term),
                                        n, ol_h, int(config.get("model_error_windows", 256)), args.seed)

    outdir = f"{args.dir}/{args.policy}/{args.env}-srcdatatype-{args.srctype}-tardatatype-{args.tartype}-{args.shift_level}/r{args.seed}{args.out_dir_remark}"
    writer = None
    if args.scalars:                                                                   # train_mobody.py:455-458
        writer = ScalarLog(f"{outdir}/tb/scalars.csv") if rank == 0 else NullLog()
    dynamics = None
    if uses_model(args.policy):                       # a model-free baseline (TD3_BC) has no ensemble to build, load or train
        model = MOBODYModule(obs_dim=state_dim, action_dim=action_dim, hidden_dims=256, num_ensemble=7, num_elites=5,
                             weight_decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], device=device,
                             reward_relu=args.relu_reward, config=config)
        # no CLI flag (the reference's driver never passes one, train_mobody.py:805-812): an optional key of the merged config
        dynamics = MOBODYEnsembleDynamics(config, model, None, None, terminal_fn, penalty_coef=env_penalty_coef,
                                          uncertainty_mode=config.get("uncertainty_mode", "pairwise-diff"),
                                          rng=args.rng, seed=args.seed + 3)
        build_dynamics(args, dynamics, model, src_rb, tar_rb, writer, task, explicit_synthetic=args.synthetic == 1,
                       rank=rank, world=world)
        config.update({"dynamics": dynamics})
        policy.dynamics = dynamics
        if int(config.get("model_eval_dynamics", 0)):
            say(f"model_eval_dynamics ignored: {args.policy} builds its own model")
    elif int(config.get("model_eval_dynamics", 0)) and world > 1:
        # data-parallel baselines are not built: every rank would build and pre-train a model only rank 0 evaluates in
        raise SystemExit("model_eval_dynamics: not supported under a process group (run the baseline on one GPU)")
    elif int(config.get("model_eval_dynamics", 0)):
        # A baseline judged in the learned target model (optional key of the merged config, off by default): the same ensemble,
        # the same load-or-train branches and flags as above, handed to the policy as the reference's driver hands it to every
        # policy -- but an EVALUATOR only.  `dynamics` stays None here, so nothing below that samples a buffer for the model
        # runs; torch's generators and the buffers' draw counts are put back after the model is built and pre-trained, so the
        # trained policy and every non-`test/model` scalar row are bit for bit what they are without the key.
        rng_state = (torch.get_rng_state(), torch.cuda.get_rng_state_all(), np.random.get_state(), random.getstate())
        draws = (src_rb._draws, tar_rb._draws)
        model = MOBODYModule(obs_dim=state_dim, action_dim=action_dim, hidden_dims=256, num_ensemble=7, num_elites=5,
                             weight_decays=[2.5e-5, 5e-5, 7.5e-5, 7.5e-5, 1e-4], device=device,
                             reward_relu=args.relu_reward, config=config)
        eval_dynamics = MOBODYEnsembleDynamics(config, model, None, None, terminal_fn, penalty_coef=env_penalty_coef,
                                               uncertainty_mode=config.get("uncertainty_mode", "pairwise-diff"),
                                               rng=args.rng, seed=args.seed + 3)
        build_dynamics(args, eval_dynamics, model, src_rb, tar_rb, NullLog(), task, explicit_synthetic=args.synthetic == 1,
                       rank=rank, world=world)
        policy.dynamics = eval_dynamics
        torch.set_rng_state(rng_state[0]); torch.cuda.set_rng_state_all(rng_state[1])
        np.random.set_state(rng_state[2]); random.setstate(rng_state[3])
        src_rb._draws, tar_rb._draws = draws

    # Evaluation of the policy in the learned target model (no simulators in this build): two optional keys of the merged
    # config, off by default.  Rank 0 evaluates; start states are episode starts of the target data.
    eval_obs, ref_env_name = None, f"{args.env}-{args.shift_level}"               # train_mobody.py:331
    eval_members = False
    if int(config.get("model_eval_episodes", 0)) > 0:
        if policy.dynamics is None:
            say(f"model_eval_episodes / model_eval_horizon ignored: {args.policy} has no model to evaluate in")
        elif rank == 0:
            from mobody_amd.envs.infos import get_normalized_score
            get_normalized_score(0.0, ref_env_name)   # an unknown task raises KeyError here, not at the first evaluation
            n = tar_rb.size
            term = 1.0 - tar_rb.not_done[:n].cpu().numpy()
            rows = model_eval_rows(episode_starts(tar_rb.state[:n].cpu().numpy(), tar_rb.next_state[:n].cpu().numpy(), term),
                                   int(config["model_eval_episodes"]), args.seed)
            eval_obs = tar_rb.state[torch.as_tensor(rows, device=tar_rb.state.device)].contiguous()
            # one return per elite member and their spread next to the five tags (optional key, read only here)
            eval_members = bool(int(config.get("model_eval_members", 0)))

    # Fitted Q evaluation of the policy on the recorded target transitions (mobody_amd.fqe; every algorithm): optional keys of the
    # merged config, off by default.  Rank 0 evaluates alone; start states are episode starts of the target data, chosen once.
    fqe, fqe_obs = None, None
    if int(config.get("fqe_steps", 0)) > 0 and rank == 0:
        from mobody_amd.fqe import FQE
        n = tar_rb.size
        term = 1.0 - tar_rb.not_done[:n].cpu().numpy()
        rows = model_eval_rows(episode_starts(tar_rb.state[:n].cpu().numpy(), tar_rb.next_state[:n].cpu().numpy(), term),
                               int(config.get("fqe_episodes", 256)), args.seed)
        fqe_obs = tar_rb.state[torch.as_tensor(rows, device=tar_rb.state.device)].contiguous()
        net, head = policy.eval_policy()
        fqe = FQE(net, head, state_dim, action_dim, max_action, float(config["gamma"]), device, net.precision,
                  lr=float(config.get("fqe_lr", 3e-4)), tau=float(config.get("tau", 0.005)), batch_size=int(config.get("fqe_batch_size", 256)),
                  seed=args.seed, rng=args.rng)

    # The true task (--synthetic 2): rank 0 evaluates alone.  The two reference points of the normalized score, the `random` and
    # `expert` controllers' returns in the target, are measured once; the data's mean episode returns are logged once.
    task_ref_returns = None
    task_eval = (int(config.get("task_eval_episodes", 32)), int(config.get("task_episode_steps", 1000)))
    if task_tar is not None and rank == 0:
        task_ref_returns = tuple(task_tar.evaluate(None, 2, task_eval[0], task_eval[1], controller=c, rng=args.rng)["return_mean"]
                                 for c in ("random", "expert"))
        say(f"task reference points in the target: random {task_ref_returns[0]:.1f}, expert {task_ref_returns[1]:.1f}")
        if writer is not None:
            for tag, r in zip(("data/source return", "data/target return"), data_returns):
                if r is not None:
                    writer.add_scalar(tag, r, global_step=0)

    if args.save_model and rank == 0:
        os.makedirs(f"{outdir}/models", exist_ok=True)
    if config.get("info_pretrain") and hasattr(policy, "update_info"):
        # IGDF's contrastive encoders: the reference's driver never trains them (they keep their initial values); an optional key
        # of the merged config runs the class's update_info once, info_update_step steps, before the loop
        policy.update_info(src_rb, tar_rb, config["batch_size"], writer)
    # The online modes (train_mobody.py:675-770) in the analytic task: the policy's own net acts on `online_lanes` lanes (an optional
    # key of the merged config, default 1: the reference drives one environment) and the transition goes straight into the ring on
    # the device (mobody_task_interact).  Mode 1: one target interaction at every t % tar_env_interact_interval == 0, no exploration
    # noise (:683-685); mode 2: one source interaction with noise before every train call (:733-735).
    online, online_every, online_tag = None, 1, None
    if args.mode in (1, 2):
        lanes = int(config.get("online_lanes", 1))
        if args.mode == 1:
            online = task_tar.online(tar_rb, lanes, task_eval[1], 0.0, seed=args.seed + 2, rng=args.rng)
            online_every, online_tag = int(config["tar_env_interact_interval"]), "train/target return"
        else:
            online = task_src.online(src_rb, lanes, task_eval[1], ONLINE_EXPL_NOISE, seed=args.seed + 1, rng=args.rng)
            online_tag = "train/source return"
    start = time.time()
    for t in range(int(config["max_step"])):
        if online is not None and t % online_every == 0:
            online.interact(*policy.eval_policy())
        policy.train(src_rb, tar_rb, config["batch_size"], writer, None)
        if (t + 1) % args.log_every == 0:
            if hasattr(policy, "log_line"):           # BOSA: the stage's own losses under their own names
                line = policy.log_line()
            else:
                if world > 1:                         # losses() is this rank's share of the global means (kernels scale by
                    share = policy._loss[:3].clone()  # 1 / N_global): summed on log steps only
                    torch.distributed.all_reduce(share)
                    q, pi, bc = (float(x) for x in share.tolist())
                else:
                    q, pi, bc = policy.losses()
                third = getattr(policy, "third_loss_name", "bc_loss")       # IQL reports its V loss there
                line = f"q_loss {q:.4f} pi_loss {pi:.4f} {third} {bc:.4f}"
            dt = time.time() - start
            say(f"step {t + 1}: {line}  {args.log_every / dt:.1f} grad-steps/s")
            start = time.time()
        if (t + 1) % config["eval_freq"] == 0 and rank == 0:           # rank 0 alone: no collective in this block
            # The reference's evaluation block (train_mobody.py:928-975) rolls the policy out in the simulators; of it, what
            # does not need a simulator is kept on the same cadence: the transition model's error on TARGET transitions
            # (eval_policy_batch's obs-RMSE / reward-MSE, :100-133, here on a target-buffer batch) and the model checkpoint.
            if writer is not None and dynamics is not None:
                s_, a_, s2_, r_, _ = tar_rb.sample(min(1000, tar_rb.size))
                err = dynamics.model_error(s_, a_, s2_, r_)
                writer.add_scalar("test/model error next_obs", err["obs_mse"], global_step=t + 1)
                writer.add_scalar("test/model error reward", err["reward_mse"], global_step=t + 1)
            if writer is not None and ol_rows is not None:
                # the compounding-error curve (the model fed the recorded actions, reset_every = 0) and, on the same
                # windows, the one-step error at every offset (reset_every = 1); one host read per call
                ol = policy.open_loop_error(tar_rb, ol_rows, ol_h)
                curve = torch.stack([ol["obs_err_mean"], ol["rew_mse"], ol["term_agree"]]).tolist()
                for k in sorted({k for k in OPEN_LOOP_STEPS if k <= ol_h} | {ol_h}):
                    writer.add_scalar(f"test/open-loop obs error h{k}", curve[0][k - 1], global_step=t + 1)
                    writer.add_scalar(f"test/open-loop reward mse h{k}", curve[1][k - 1], global_step=t + 1)
                    writer.add_scalar(f"test/open-loop term agree h{k}", curve[2][k - 1], global_step=t + 1)
                one = policy.open_loop_error(tar_rb, ol_rows, ol_h, reset_every=1)["obs_err_mean"].mean().reshape(1).tolist()
                writer.add_scalar("test/one-step obs error", one[0], global_step=t + 1)
            if writer is not None and eval_obs is not None:
                # eval_policy_batch's return (:60-98) with the learned target model in the simulator's place: an ESTIMATE
                # whose error grows with the horizon -- hence tags of its own, never the simulator's 'test/target return'
                ev = policy.evaluate_in_model(eval_obs, int(config.get("model_eval_horizon", 1000)),
                                              **(dict(members=True) if eval_members else {}))
                writer.add_scalar("test/model target return", ev["return_mean"], global_step=t + 1)
                writer.add_scalar("test/model target normalized score", get_normalized_score(ev["return_mean"], ref_env_name),
                                  global_step=t + 1)
                writer.add_scalar("test/model episode length", ev["length_mean"], global_step=t + 1)
                writer.add_scalar("test/model penalty", ev["penalty_mean"], global_step=t + 1)
                writer.add_scalar("test/model alive frac", ev["alive_frac"], global_step=t + 1)
                if eval_members:
                    # every start state rolled once per elite, each episode under one member: the members' disagreement is an
                    # error bar on the estimate above
                    writer.add_scalar("test/model return member spread", ev["return_member_spread"], global_step=t + 1)
                    for k, v in enumerate(ev["return_member_means"]):
                        writer.add_scalar(f"test/model return member e{k}", v, global_step=t + 1)
            if writer is not None and task_ref_returns is not None:
                # the reference's own scalars (train_mobody.py:928-975), from the true task in the simulators' place
                ev_s = policy.evaluate_in_task(task_src, task_eval[0], task_eval[1], rng=args.rng)
                ev_t = policy.evaluate_in_task(task_tar, task_eval[0], task_eval[1], rng=args.rng)
                r_rand, r_exp = task_ref_returns
                writer.add_scalar("test/source return", ev_s["return_mean"], global_step=t + 1)
                writer.add_scalar("test/target return", ev_t["return_mean"], global_step=t + 1)
                writer.add_scalar("test/target episode length", ev_t["length_mean"], global_step=t + 1)
                # reference points that coincide (a shift in which the expert falls at once, a tiny task_episode_steps): NaN
                score = 100.0 * (ev_t["return_mean"] - r_rand) / (r_exp - r_rand) if r_exp != r_rand else float("nan")
                writer.add_scalar("test/target normalized score", score, global_step=t + 1)
            if writer is not None and online is not None:
                # the reference logs every finished episode (:700-704, :750-752), which would cost a host read per step; here the
                # mean over the episodes finished since the previous evaluation, nothing when there are none
                es = online.episode_stats()
                if es["episodes"] > 0:
                    writer.add_scalar(online_tag, es["return_mean"], global_step=t + 1)
                    writer.add_scalar("train/episodes", es["episodes"], global_step=t + 1)
                    writer.add_scalar("train/episode length", es["length_mean"], global_step=t + 1)
            if writer is not None and fqe is not None:
                # the discounted value at config['gamma'] of the policy as it is now, by FQE: an estimate whose bias grows with the
                # policy's distance from the data; not a return, so no normalized score is derived from it
                t0 = time.time()
                fqe.prepare(warm_start=bool(int(config.get("fqe_warm_start", 0))))
                if fqe.fit(tar_rb, int(config["fqe_steps"])):
                    ev = fqe.value(fqe_obs)
                    writer.add_scalar("test/fqe value", ev["value"], global_step=t + 1)
                    writer.add_scalar("test/fqe head gap", ev["head_gap"], global_step=t + 1)
                    writer.add_scalar("test/fqe td loss", fqe.td_loss(), global_step=t + 1)
                    writer.add_scalar("test/fqe seconds", time.time() - t0, global_step=t + 1)
            if writer is not None:
                writer.flush()
            if args.save_model:
                policy.save(f"{outdir}/models/model")
    if writer is not None:
        writer.close()
    torch.cuda.synchronize()
    policy._health_check()                   # a fault after the last check point must not end the run silently
    return policy


if __name__ == "__main__":
    main()
