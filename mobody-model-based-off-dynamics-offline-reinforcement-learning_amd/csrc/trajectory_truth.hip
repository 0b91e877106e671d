// Open-loop model error over recorded trajectories: the two kernels of mobody_ens_replay (dynamics.hip) that the ensemble
// step does not already have.  The model is started at a recorded state, fed the RECORDED actions of that trajectory and
// compared with the recorded next state and reward at every step -- the compounding-error curve.
//
//   k_replay_account in k_dyn_finalize's place: raw reward = mean_e r_mu (k_dyn_finalize's expression and order), the
//                    errors of window step t against data row r = row0 + t, obs' (or the recorded next state) ->
//                    obs_state, the recorded action of row r + 1 -> act_state
//   k_replay_init    obs_state / act_state = the recorded state / action of row0
//
// A translation unit of its own, linked after the others: every code object of the existing kernels stays byte for byte
// what it was (tools/isa_diff.py) and where it was.  Both kernels stream B * (S + A) floats plus a few words per row:
// their cost is a launch's latency.  Data rows are addressed through gather.h's view_* (ring or five arrays); every row
// index is clamped into [0, data_rows - 1] before it is used, so no load leaves the view whatever row0 holds.
#include "common.h"
#include "gather.h"

namespace mobody {

struct ReplayAccountArgs {
  const float* r_mu;            // [E][B]
  const float* pen;             // [B]
  const float* next_obs;        // [B][S]
  const uint8_t* term;          // [B] the predicate on next_obs (the step ran under alive = NULL)
  MobodyBufferView data;
  long long data_rows;
  const long long* row0;        // [B]
  float *obs_state, *act_state; // [B][S], [B][A]
  float *obs_err, *rew_err, *penalty;   // [B]: row t of the tables
  uint8_t* term_model;          // [B]: row t
  long long B;
  int S, A, t, reset;
};

__device__ __forceinline__ long long replay_row(const long long* row0, long long b, long long t, long long data_rows) {
  const long long r = row0[b] + t, last = data_rows - 1;
  return r < 0 ? 0 : r > last ? last : r;
}

// One thread per element of [B][S] forms the next row state (consecutive lanes, consecutive addresses) and one per element
// of [B][A] fetches the next recorded action; the first B threads also own one row each: raw reward and the step's errors.
// Nothing is masked: a NaN from the model reaches the tables.
__global__ __launch_bounds__(256) void k_replay_account(ReplayAccountArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = a.S, A = a.A;
  if (i < a.B * S) {
    const long long b = i / S;
    const int d = (int)(i - b * S);
    const long long r = replay_row(a.row0, b, a.t, a.data_rows);
    const float rec = view_next_state(a.data, r, S)[d], mdl = a.next_obs[i];
    a.obs_state[i] = a.reset ? rec : mdl;
  }
  if (i < a.B * A) {
    const long long b = i / A;
    const int c = (int)(i - b * A);
    const long long r1 = replay_row(a.row0, b, a.t + 1LL, a.data_rows);     // min(r + 1, data_rows - 1)
    a.act_state[i] = view_action(a.data, r1, A)[c];
  }
  if (i >= a.B) return;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NENS; ++e) s += a.r_mu[(long long)e * a.B + i];
  const float raw = s * (1.f / NENS);                                      // reward.mean(0), mobody_dynamics.py:236
  const long long r = replay_row(a.row0, i, a.t, a.data_rows);
  const float* rec = view_next_state(a.data, r, S);
  const float* mdl = a.next_obs + i * S;
  float sq = 0.f;
  for (int d = 0; d < S; ++d) {                                            // sequential, increasing d, no fma (-ffp-contract=off)
    const float df = mdl[d] - rec[d];
    sq += df * df;
  }
  a.obs_err[i] = sqrtf(sq);
  a.rew_err[i] = raw - view_reward(a.data, r)[0];
  a.penalty[i] = a.pen[i];
  a.term_model[i] = a.term[i];
}

__global__ __launch_bounds__(256) void k_replay_init(MobodyBufferView data, long long data_rows, const long long* row0,
                                                     float* obs_state, float* act_state, long long B, int S, int A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * S) {
    const long long b = i / S;
    obs_state[i] = view_state(data, replay_row(row0, b, 0, data_rows), S)[(int)(i - b * S)];
  }
  if (i < B * A) {
    const long long b = i / A;
    act_state[i] = view_action(data, replay_row(row0, b, 0, data_rows), A)[(int)(i - b * A)];
  }
}

static unsigned replay_grid(long long B, int S, int A) { return (unsigned)cdiv(B * (S > A ? S : A), 256); }

int launch_replay_account(const float* r_mu, const float* penalty, const float* next_obs, const uint8_t* terminal,
                          const DynReplayHook& h, long long B, int S, int A, hipStream_t st) {
  ReplayAccountArgs ra{r_mu, penalty, next_obs, terminal, *h.data, h.data_rows, h.row0, h.obs_state, h.act_state,
                       h.obs_err, h.rew_err, h.penalty, h.term_model, B, S, A, h.t, h.reset};
  hipLaunchKernelGGL(k_replay_account, dim3(replay_grid(B, S, A)), dim3(256), 0, st, ra);
  MB_LAUNCH_OK("k_replay_account");
  return 0;
}

int launch_replay_init(const DynReplayHook& h, long long B, int S, int A, hipStream_t st) {
  hipLaunchKernelGGL(k_replay_init, dim3(replay_grid(B, S, A)), dim3(256), 0, st, *h.data, h.data_rows, h.row0, h.obs_state,
                     h.act_state, B, S, A);
  MB_LAUNCH_OK("k_replay_init");
  return 0;
}

}  // namespace mobody
