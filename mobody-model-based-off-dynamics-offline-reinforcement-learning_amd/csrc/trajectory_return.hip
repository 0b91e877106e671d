// Per-row return accounting of imagined trajectories: the two kernels of mobody_ens_evaluate (dynamics.hip) that the
// ensemble step does not already have.  eval_policy_batch's sums (train_mobody.py:60-98: the rewards of a row up to and
// including its terminating step) over the learned step instead of a simulator.
//
//   k_eval_account in k_dyn_finalize's place: raw reward = mean_e r_mu (k_dyn_finalize's expression and order), the
//                  accounting on the caller's row state, the alive commit, obs' -> obs_state
//   k_eval_init    the row state of resume == 0
//
// A translation unit of its own, linked after the others: every code object of the existing kernels stays byte for byte
// what it was (tools/isa_diff.py) and where it was.  Both kernels stream B * S floats plus a few words per row: their cost
// is a launch's latency.
#include "common.h"

namespace mobody {

struct EvalAccountArgs {
  const float* r_mu;            // [E][B]
  const float* penalty;         // [B]
  const float* next_obs;        // [B][S]
  const uint8_t* alive_next;    // [B] alive && !terminal, from the sample kernel (a workspace buffer, never `alive`)
  float* obs_state;             // [B][S]
  uint8_t* alive;               // [B] the mask the step ran under; committed to alive_next here
  float *ret, *pen_sum, *disc;  // [B]
  int32_t* length;              // [B]
  long long B;
  int S;
  float discount;
};

// One thread per element of [B][S] moves obs' into the row state (consecutive lanes, consecutive addresses); the first B
// threads also own one row each: raw reward, the accounting, the alive commit.  A dead row reads none of its (possibly
// NaN) reward or penalty.
__global__ __launch_bounds__(256) void k_eval_account(EvalAccountArgs a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < a.B * a.S) a.obs_state[i] = a.next_obs[i];
  if (i >= a.B) return;
  if (a.alive[i]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NENS; ++e) s += a.r_mu[(long long)e * a.B + i];
    const float raw = s * (1.f / NENS);                                   // reward.mean(0), mobody_dynamics.py:236
    const float d = a.disc[i];
    a.ret[i] = fmaf(d, raw, a.ret[i]);
    a.pen_sum[i] += a.penalty[i];
    a.length[i] += 1;
    a.disc[i] = d * a.discount;
  }
  a.alive[i] = a.alive_next[i];
}

__global__ __launch_bounds__(256) void k_eval_init(const float* init_obs, float* obs_state, uint8_t* alive, float* ret,
                                                   float* pen_sum, float* disc, int32_t* length, long long B, int S) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * S) obs_state[i] = init_obs[i];
  if (i >= B) return;
  alive[i] = 1;
  ret[i] = 0.f;
  pen_sum[i] = 0.f;
  disc[i] = 1.f;
  length[i] = 0;
}

int launch_eval_account(const float* r_mu, const float* penalty, const float* next_obs, const uint8_t* alive_next,
                        const DynEvalHook& h, long long B, int S, hipStream_t st) {
  EvalAccountArgs ea{r_mu, penalty, next_obs, alive_next, h.obs_state, h.alive, h.ret, h.pen_sum, h.disc, h.length, B, S, h.discount};
  hipLaunchKernelGGL(k_eval_account, dim3((unsigned)cdiv(B * S, 256)), dim3(256), 0, st, ea);
  MB_LAUNCH_OK("k_eval_account");
  return 0;
}

int launch_eval_init(const float* init_obs, const DynEvalHook& h, long long B, int S, hipStream_t st) {
  hipLaunchKernelGGL(k_eval_init, dim3((unsigned)cdiv(B * S, 256)), dim3(256), 0, st, init_obs, h.obs_state, h.alive, h.ret, h.pen_sum,
                     h.disc, h.length, B, S);
  MB_LAUNCH_OK("k_eval_init");
  return 0;
}

}  // namespace mobody
