"""Restatement of the accounting of `mobody_ens_replay` (include/mobody_hip.h) in NumPy fp32: the data row of a window
step and its clamp, the sequential fp32 error sum with `np.sqrt` in float32, the reset rule and the action hand-over.
Shared by the CPU tests (hand-made tables) and the GPU tests (the composition of entry points the build already had)."""
import numpy as np


def data_row(row0, t, data_rows):
    """r = min(row0 + t, data_rows - 1) per window."""
    return np.minimum(np.asarray(row0, np.int64) + int(t), int(data_rows) - 1)


def is_reset(t, reset_every):
    return int(reset_every) > 0 and (int(t) + 1) % int(reset_every) == 0


def init(data, row0, data_rows):
    """(obs_state, act_state) before step 0: the recorded state and action of row0."""
    r = data_row(row0, 0, data_rows)
    return data["state"][r].astype(np.float32), data["action"][r].astype(np.float32)


def sq_sum32(model_next, rec_next):
    """sum_d (obs' - rec)^2 in fp32, sequential in increasing d, every operation rounded on its own (no fma)."""
    a, b = np.asarray(model_next, np.float32), np.asarray(rec_next, np.float32)
    s = np.zeros(a.shape[0], np.float32)
    for d in range(a.shape[1]):
        df = (a[:, d] - b[:, d]).astype(np.float32)
        s = (s + (df * df).astype(np.float32)).astype(np.float32)
    return s


def obs_err_f64(model_next, rec_next):
    """The same distance in fp64 from the same fp32 inputs."""
    d = np.asarray(model_next, np.float32).astype(np.float64) - np.asarray(rec_next, np.float32).astype(np.float64)
    return np.sqrt(np.sum(d * d, axis=1))


def account(data, row0, data_rows, t, reset_every, model_next, raw, pen, term):
    """One window step: (the tables' rows of step t, the next obs_state, the next act_state).  model_next [B][S], raw / pen
    fp32 [B], term bool [B] are the model's outputs of the step."""
    r = data_row(row0, t, data_rows)
    rec = data["next_state"][r].astype(np.float32)
    model_next = np.asarray(model_next, np.float32)
    row = dict(obs_err=np.sqrt(sq_sum32(model_next, rec)).astype(np.float32),
               rew_err=(np.asarray(raw, np.float32).reshape(-1) - data["reward"].reshape(-1)[r].astype(np.float32)).astype(np.float32),
               penalty=np.asarray(pen, np.float32).reshape(-1).copy(), term_model=np.asarray(term).reshape(-1).astype(bool))
    obs_state = rec.copy() if is_reset(t, reset_every) else model_next.copy()
    act_state = data["action"][np.minimum(r + 1, int(data_rows) - 1)].astype(np.float32)
    return row, obs_state, act_state


def replay(data, row0, data_rows, H, reset_every, step):
    """The whole call with `step(t, obs_state, act_state) -> (obs', raw, pen, term)` in the model's place.  Returns the
    [H][B] tables and the final row state."""
    obs, act = init(data, row0, data_rows)
    rows = []
    for t in range(H):
        nxt, raw, pen, term = step(t, obs, act)
        row, obs, act = account(data, row0, data_rows, t, reset_every, nxt, raw, pen, term)
        rows.append(row)
    B = len(np.asarray(row0))
    empty = dict(obs_err=np.zeros((0, B), np.float32), rew_err=np.zeros((0, B), np.float32), penalty=np.zeros((0, B), np.float32),
                 term_model=np.zeros((0, B), bool))
    tables = {k: np.stack([r[k] for r in rows]) if rows else empty[k] for k in empty}
    return tables, obs, act
