"""Data-parallel exchange protocol of one MOBODY gradient step (host logic, device agnostic).

One process per GPU; every rank holds replicated weights and draws its own rows.  The engine
computes LOCAL shares of the GLOBAL means (losses and gradients are scaled by 1/N_global inside the
kernels), so plain SUM all-reduces make the N-rank update equal the 1-rank update on the
concatenated batch:

    critic gradients (one flat blob)          all_reduce(SUM)   -> Adam + Polyak on every rank
    stats = [sum|min Q(s,pi(s))|, sum|min Q(s_t,a_t)|]  all_reduce(SUM)   (needed BEFORE the actor backward:
                                              p_w = w / mean|q| and adv = q_b / mean|q_b| are global normalisers,
                                              mobody.py:318,259)
    actor gradients (one flat blob)           all_reduce(SUM)   -> Adam on every rank

`engine` is any object with the six methods used below; the product engine is
`MOBODY` (HIP kernels); `tests/test_dp_protocol.py` drives the same function with a CPU engine
built on the oracle under gloo, world size 2.

The second half of the file is how a training process becomes a rank: `init_from_env()` reads the launcher's
environment (RANK / LOCAL_RANK / WORLD_SIZE, as `torch.distributed.run` sets them) and creates the process group,
`launch()` / `python -m mobody_amd.dp --gpus N -- <train_mobody arguments>` is a launcher of the project's own.
"""
import os
import subprocess
import sys
import time

MAX_RANKS = 16


def rank_salt(dist=None):
    """Per-rank offset folded into every device-RNG seed (index draws, rollout noise, elite picks): 0 on one process."""
    if dist is None:
        import torch
        dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return 1000003 * dist.get_rank()
    return 0


def world_size(dist):
    return dist.get_world_size() if dist is not None and dist.is_available() and dist.is_initialized() else 1


def dp_update(engine, batch, n_rows, n_true, dist=None, equal_shards=True):
    world = world_size(dist)
    n_glob, nt_glob = n_rows * world, n_true * world          # every rank draws the same number of rows
    if world > 1 and not equal_shards:              # ragged shards: agree on the global counts first (costs a sync)
        import torch
        cnt = torch.tensor([n_rows, n_true], dtype=torch.int64, device=engine.comm_device())
        dist.all_reduce(cnt)
        n_glob, nt_glob = int(cnt[0]), int(cnt[1])
    if getattr(engine, "has_value_phase", lambda: False)():      # config['advantage']: V update first (mobody.py:533-537)
        engine.value_grad(batch, n_rows, n_true, n_glob, nt_glob)
        if world > 1:
            dist.all_reduce(engine.value_grad_buffer())
        engine.value_apply()
    engine.critic_grad(batch, n_rows, n_true, n_glob, nt_glob)
    if world > 1:
        dist.all_reduce(engine.critic_grad_buffer())
    engine.critic_apply()                           # Adam, then Polyak (mobody.py:546-552)
    engine.actor_stats(batch, n_rows, n_true, n_glob, nt_glob)
    if world > 1:
        dist.all_reduce(engine.stats_buffer())
    engine.actor_grad(batch, n_rows, n_true, n_glob, nt_glob)
    if world > 1:
        dist.all_reduce(engine.actor_grad_buffer())
    engine.actor_apply()
    return n_glob, nt_glob


# ---------------------------------------------------------------------------------------------- rank bootstrap
_owns_group = False       # the process group was created by init_from_env(): shutdown() destroys it (and only then)


def init_from_env(environ=None):
    """-> (rank, world, device).  WORLD_SIZE absent or 1: a single process, `torch.distributed` is not touched and the device
    is what the CLI always picked.  World > 1: BEFORE any GPU call the process binds to `LOCAL_RANK % device_count` (the
    modulo lets several ranks share the one GPU of a test box), then creates the process group from MASTER_ADDR /
    MASTER_PORT: RCCL ("nccl", bound to the device) by default, `MOBODY_DP_BACKEND=gloo` to rehearse with several ranks on
    one GPU (RCCL refuses duplicate devices).  A group the caller already created is used as it is."""
    global _owns_group
    import torch
    env = os.environ if environ is None else environ
    world = int(env.get("WORLD_SIZE", "1") or 1)
    if world <= 1:
        return 0, 1, torch.device("cuda" if torch.cuda.is_available() else "cpu")
    rank = int(env.get("RANK", "0"))
    n_dev = torch.cuda.device_count()
    if n_dev < 1:
        raise RuntimeError(f"WORLD_SIZE={world}: data-parallel training needs a GPU on every rank (none visible to rank {rank})")
    local = int(env.get("LOCAL_RANK", str(rank))) % n_dev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = torch.distributed
    if not dist.is_initialized():
        backend = env.get("MOBODY_DP_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        _owns_group = True
    return dist.get_rank(), dist.get_world_size(), dev


def shutdown():
    """Destroy the process group init_from_env() created (no-op for a single process or a caller-owned group)."""
    global _owns_group
    if _owns_group:
        import torch
        _owns_group = False
        if torch.distributed.is_initialized():
            torch.distributed.destroy_process_group()


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(n, cmd, env=None, stdout=None, poll=0.2, grace=20.0):
    """Start `cmd` (an argv list) `n` times as fresh child processes, rank r with RANK = LOCAL_RANK = r, WORLD_SIZE = n,
    MASTER_ADDR = 127.0.0.1 and one MASTER_PORT (the caller's, or a free one); rank 0 writes to `stdout` (default: this
    process's), the other ranks' stdout is dropped, stderr is shared.  Returns 0 when every rank exits 0.  Every child is
    polled: a rank that dies early would leave the others waiting in a collective, so on the first non-zero exit the rest are
    stopped and that rank's status is returned.

    The caller must not have initialised the GPU (children are started with Popen, never forked from or exec'd over a
    process that holds a HIP context); nothing here imports torch."""
    n = int(n)
    if not 1 <= n <= MAX_RANKS:
        raise ValueError(f"launch: {n} ranks asked for, 1..{MAX_RANKS} supported")
    base = dict(os.environ if env is None else env)
    port = str(base.get("MASTER_PORT") or _free_port())
    procs, failed = [], None
    try:
        for r in range(n):
            e = dict(base, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
            e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")               # as bench.py's launcher starts its ranks
            procs.append(subprocess.Popen(list(cmd), env=e, stdout=stdout if r == 0 else subprocess.DEVNULL))
        while failed is None and any(p.poll() is None for p in procs):
            for r, p in enumerate(procs):
                if p.poll() is not None and p.returncode != 0:
                    failed = r
                    break
            else:
                time.sleep(poll)
        if failed is None:                                                # the loop can end on the poll that saw the last exit
            failed = next((r for r, p in enumerate(procs) if p.returncode != 0), None)
    finally:                                                              # also on KeyboardInterrupt: leave nothing running
        for p in procs:
            if p.poll() is None:
                p.terminate()
        deadline = time.time() + grace
        for p in procs:
            try:
                p.wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    if failed is None:
        return 0
    print(f"mobody_amd.dp: rank {failed} exited with code {procs[failed].returncode}; stopped the other ranks", file=sys.stderr)
    return abs(procs[failed].returncode) or 1


def main(argv=None):
    """`python -m mobody_amd.dp --gpus N -- <train_mobody arguments>`: N ranks of the training CLI on this host."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m mobody_amd.dp",
                                 description="start N data-parallel ranks of train_mobody.py, one per GPU")
    ap.add_argument("--gpus", type=int, required=True, help=f"number of ranks (1..{MAX_RANKS})")
    ap.add_argument("train_args", nargs=argparse.REMAINDER, help="-- followed by the arguments of train_mobody.py")
    args = ap.parse_args(argv)
    if not 1 <= args.gpus <= MAX_RANKS:
        ap.error(f"--gpus must be in 1..{MAX_RANKS}")
    rest = args.train_args[1:] if args.train_args[:1] == ["--"] else args.train_args
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))     # where the `mobody_amd` package is importable from
    env = dict(os.environ)
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return launch(args.gpus, [sys.executable, "-m", "mobody_amd.train_mobody"] + rest, env=env)


if __name__ == "__main__":
    sys.exit(main())
