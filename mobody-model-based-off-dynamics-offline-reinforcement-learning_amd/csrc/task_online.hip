// One interaction of the current policy with the analytic control task, recorded straight into a replay ring (the
// online modes 1 and 2 of the driver).  The reference steps a simulator on the host and calls ReplayBuffer.add
// (train_mobody.py:675-770); here the policy forward, the step and the ring write are three launches with no host read:
//
//   the packed 3-layer forward  pi(s) (head 0, out_mode 1) or the raw mu | logstd (head 1) of the lanes' current states
//   k_task_interact             action (sample, exploration noise, clamp), the step, the lane's bookkeeping, ring row (ptr + b) mod cap
//   k_task_commit               one thread: ptr, size and the interaction count
//
// k_task_interact has k_task's geometry (task.hip): a workgroup owns rpb = 256 / S whole lanes staged in LDS, one thread per (lane,
// dim) element, then one thread per lane.  The step is RESTATED here, operation for operation, instead of sharing k_task's body: a
// shared body would have to grow a mode, and every older code object keeps its bytes only while task.hip is untouched
// (tools/isa_diff.py).  tests/test_hip_task_online.py holds the two to the same bits.  Every product and sum is an fp32 operation of
// its own in a fixed order (the build has no contraction).  No flags, tickets or atomics; every loop is bounded by an argument; the
// kernel only READS ptr_size and the count word, k_task_commit alone writes them, and stream order is the only synchronisation.
// A translation unit of its own, linked after task.hip.  Cost: a lane is 2 S + A + 2 floats of ring traffic; the call is three
// launch latencies.
#include <math.h>

#include "common.h"
#include "gather.h"
#include "layers.h"
#include "rng.h"
#include "term.h"

namespace mobody {

constexpr int ONLINE_S_MAX = 256, ONLINE_A_MAX = 64;
constexpr int ONLINE_MAX_U = (256 / 3) * ONLINE_A_MAX;     // lanes per workgroup x A at the smallest S

struct InteractArgs {
  MobodyTaskParams p;
  const float* pol;           // head 0: pi [lanes][A]; head 1: mu | logstd [lanes][2 A]
  int head, time_limit, packed;
  float expl, init_std;
  uint32_t seed, call0;
  long long lanes, cap;
  MobodyBufferView ring;      // written
  const long long* ptr_size;  // read only
  const long long* count;     // read only
  float* lane_obs;            // [lanes][S]
  int32_t *lane_t, *lane_ep, *done_count, *len_sum;
  float *lane_ret, *ret_sum;
};

__global__ __launch_bounds__(256) void k_task_interact(InteractArgs a, int rpb) {
  __shared__ float s_z[256], s_nxt[256], s_vp[256], s_u[ONLINE_MAX_U];
  __shared__ int s_reset[256], s_ep[256];
  const MobodyTaskParams& p = a.p;
  const int S = p.S, A = p.A;
  const int tid = threadIdx.x;
  const int r = tid / S, d = tid - r * S;
  const long long row0 = (long long)blockIdx.x * rpb;
  const long long b = row0 + r;
  const bool has = r < rpb && b < a.lanes;
  const int rows_here = (int)min((long long)rpb, a.lanes - row0);
  const uint32_t count = (uint32_t)a.count[0];
  const uint32_t call = a.call0 + count;
  const long long ptr = a.ptr_size[0];
  const MobodyBufferView& g = a.ring;
  const long long ps = g.pitch ? g.pitch : S, pa = g.pitch ? g.pitch : A, p1 = g.pitch ? g.pitch : 1;
  float* g_state = const_cast<float*>(g.state); float* g_action = const_cast<float*>(g.action);
  float* g_next = const_cast<float*>(g.next_state);
  float sv = 0.f, mu_d = 0.f;
  if (has) {
    mu_d = p.mu[d];
    sv = a.lane_obs[b * S + d];
    s_z[tid] = sv - mu_d;                                                    // z = s - mu
  }
  __syncthreads();
  for (int t = tid; t < rows_here * A; t += 256) {                           // the action, and u_j = gain_j clamp(a_j / max_action, -1, 1)
    const int rr = t / A, j = t - rr * A;
    const long long bb = row0 + rr;
    const uint64_t e = (uint64_t)bb * A + j;
    float base;
    if (a.head == 0) {
      base = a.pol[bb * A + j];
    } else {                                                                 // select_action(test=False), iql.py:74-89,160-166
      const float mu = a.pol[bb * 2 * A + j], logstd = a.pol[bb * 2 * A + A + j];
      const float sd = expf(fminf(fmaxf(logstd, -20.f), 2.f));
      const float x = mu + sd * rng_normal_at(a.seed, MOBODY_TASK_STREAM_POLICY, count, e);
      base = p.max_action * tanhf(x);
    }
    float act = base;
    if (a.expl != 0.f) {                                                     // train_mobody.py:733-735
      const float x = base + (a.expl * p.max_action) * rng_normal_at(a.seed, MOBODY_TASK_STREAM_EXPLORE, count, e);
      act = fminf(fmaxf(x, -p.max_action), p.max_action);
    }
    g_action[((ptr + bb) % a.cap) * pa + j] = act;
    s_u[t] = p.gain[j] * fminf(fmaxf(act / p.max_action, -1.f), 1.f);
  }
  __syncthreads();
  float nxt = 0.f;
  if (has) {                                                                 // k_task's step (task.hip), restated
    const float* z = s_z + r * S;
    const float* u = s_u + r * A;
    const float zi = z[d], v = z[S - 1];
    float rhs;
    if (d == 0) {                                                            // height
      rhs = (-p.f * zi) - (p.h * p.grav) * (z[1] * z[1]);
    } else if (d == 1) {                                                     // angle
      rhs = ((p.lam * p.grav) * zi + p.g * u[0]) - p.k * v;
    } else if (d == S - 1) {                                                 // forward speed
      float fwd = u[0];
      if (A > 1) {
        float s = u[1];
        for (int j = 2; j < A; ++j) s += u[j];
        fwd = s / (float)(A - 1);
      }
      rhs = (-p.f * zi) + p.g * fwd;
    } else {
      const float* bm = p.bmat + (long long)d * A;
      float ds = bm[0] * u[0];
      for (int j = 1; j < A; ++j) ds += bm[j] * u[j];
      rhs = ((-p.f * zi) + p.g * ds) + p.c * sinf(z[d - 1]);
    }
    float zp = zi + p.dt * rhs;
    if (p.sigma != 0.f) zp += p.sigma * rng_normal_at(a.seed, MOBODY_TASK_STREAM_NOISE, call, (uint64_t)b * S + d);
    nxt = zp + mu_d;
    s_nxt[tid] = nxt;
    if (d == S - 1) s_vp[r] = zp;
    const long long row = (ptr + b) % a.cap;
    g_state[row * ps + d] = sv;
    g_next[row * ps + d] = nxt;
  }
  __syncthreads();
  if (tid < rows_here) {                                                     // one thread per lane
    const long long bb = row0 + tid;
    const float* u = s_u + tid * A;
    float m = u[0] * u[0];
    for (int j = 1; j < A; ++j) m += u[j] * u[j];
    m = m / (float)A;
    const float rew = (s_vp[tid] + p.alive_bonus) - p.ctrl_cost * m;
    const bool pred = term_predicate(p.task, s_nxt + tid * S, S);
    const int t_ep = a.lane_t[bb] + 1;                                       // train_mobody.py:684-709
    const bool done = pred && t_ep < a.time_limit;
    const int reset = (pred || t_ep >= a.time_limit) ? 1 : 0;
    const long long row = (ptr + bb) % a.cap;
    const_cast<float*>(g.reward)[row * p1] = rew;
    const_cast<float*>(g.not_done)[row * p1] = 1.f - (float)done;
    if (a.packed)                                                            // the row's padding: zeros, as k_ring_scatter leaves it
      for (int c = 2 * S + A + 2; c < (int)g.pitch; ++c) g_state[row * g.pitch + c] = 0.f;
    const float ret = a.lane_ret[bb] + rew;
    const int ep = a.lane_ep[bb] + reset;
    if (reset) {
      a.done_count[bb] += 1;
      a.ret_sum[bb] += ret;
      a.len_sum[bb] += t_ep;
    }
    a.lane_t[bb] = reset ? 0 : t_ep;
    a.lane_ret[bb] = reset ? 0.f : ret;
    a.lane_ep[bb] = ep;
    s_reset[tid] = reset;
    s_ep[tid] = ep;
  }
  __syncthreads();
  if (has)                                                                   // the lane goes on, or its next episode starts here
    a.lane_obs[b * S + d] = s_reset[r] ? mu_d + a.init_std * rng_normal_at(a.seed, MOBODY_TASK_STREAM_START, (uint32_t)s_ep[r], (uint64_t)b * S + d)
                                       : nxt;
}

__global__ void k_task_commit(long long* ptr_size, long long* count, long long lanes, long long cap) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long ptr = ptr_size[0], size = ptr_size[1];
  ptr_size[0] = (ptr + lanes) % cap;
  ptr_size[1] = size + lanes < cap ? size + lanes : cap;
  count[0] += 1;
}

static int check_online_task(const char* who, const MobodyTaskParams& p) {                 // what mobody_task_step refuses of the task
  MB_REQUIRE(p.S >= 3 && p.S <= ONLINE_S_MAX, "%s: S %d outside [3, %d]", who, p.S, ONLINE_S_MAX);
  MB_REQUIRE(p.A >= 1 && p.A <= ONLINE_A_MAX, "%s: A %d outside [1, %d]", who, p.A, ONLINE_A_MAX);
  MB_REQUIRE(p.task >= MOBODY_TERM_NEVER && p.task <= MOBODY_TERM_PEN, "%s: unknown termination id %d (task)", who, p.task);
  MB_REQUIRE(p.task != MOBODY_TERM_PEN || p.S > 26, "%s: pen predicate needs S > 26 (task)", who);
  MB_REQUIRE(p.max_action > 0.f, "%s: max_action %g is not positive", who, (double)p.max_action);
  MB_REQUIRE(p.mu != nullptr, "%s: null pointer mu", who);
  MB_REQUIRE(p.gain != nullptr, "%s: null pointer gain", who);
  MB_REQUIRE(p.bmat != nullptr, "%s: null pointer bmat", who);
  return 0;
}

#define MB_NONNULL(who, blk, f) MB_REQUIRE((blk).f != nullptr, "%s: null pointer " #f, who)

}  // namespace mobody

using namespace mobody;

extern "C" int64_t mobody_task_interact_workspace(const MobodyTaskInteract* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyTaskInteract) || a->lanes < 0 || a->p.A < 1 || a->head < 0 || a->head > 1)
    return fail(MOBODY_E_ARG, "mobody_task_interact_workspace: null struct, wrong struct_bytes, lanes < 0, A < 1 or head outside {0, 1}");
  Carver take{nullptr};
  take(a->lanes * (a->head == 1 ? 2 : 1) * a->p.A);
  return take.off;
}

extern "C" int mobody_task_interact(const MobodyTaskInteract* ap, void* stream) {
  const char* who = "mobody_task_interact";
  MB_BLOCK(who, ap, MobodyTaskInteract);
  const MobodyTaskInteract& a = *ap;
  const int S = a.p.S, A = a.p.A;
  int rc = check_online_task(who, a.p);
  if (rc) return rc;
  MB_REQUIRE(a.head == 0 || a.head == 1, "%s: head %d outside {0 (deterministic actor), 1 (Gaussian policy)}", who, a.head);
  MB_REQUIRE(a.head == 0 || 2 * A <= 128, "%s: A %d: the Gaussian policy's 2 A outputs must fit 128 columns (head 1)", who, A);
  MB_REQUIRE(a.lanes >= 0, "%s: lanes < 0", who);
  MB_REQUIRE(a.lanes <= a.cap, "%s: lanes %lld > cap %lld", who, (long long)a.lanes, (long long)a.cap);
  MB_REQUIRE(a.time_limit >= 1, "%s: time_limit %d < 1", who, a.time_limit);
  MB_REQUIRE(a.expl >= 0.f, "%s: expl %g is negative or NaN", who, (double)a.expl);
  rc = check_precision(who, a.precision, a.policy_blob_T != nullptr);
  if (rc) return rc;
  MB_NONNULL(who, a, policy_blob); MB_NONNULL(who, a, ring); MB_NONNULL(who, a, ptr_size); MB_NONNULL(who, a, count);
  MB_NONNULL(who, a, lane_obs); MB_NONNULL(who, a, lane_t); MB_NONNULL(who, a, lane_ep); MB_NONNULL(who, a, lane_ret);
  MB_NONNULL(who, a, done_count); MB_NONNULL(who, a, ret_sum); MB_NONNULL(who, a, len_sum); MB_NONNULL(who, a, workspace);
  const MobodyBufferView& g = *a.ring;
  MB_REQUIRE(g.state && g.action && g.next_state && g.reward && g.not_done, "%s: null pointer in the buffer view (ring)", who);
  MB_REQUIRE(g.pitch == 0 || g.pitch >= S, "%s: pitch %lld smaller than a state row (ring)", who, (long long)g.pitch);
  MobodyMlpLayout La{};
  rc = mobody_mlp_layout(S, a.head == 1 ? 2 * A : A, 1, &La);
  if (rc) return rc;
  if (a.lanes == 0) return 0;
  hipStream_t st = as_stream(stream);
  Mlp3FwdArgs f = fwd_net(a.policy_blob, La, a.lanes);                        // mobody_mlp3_forward's launch on the lanes' states
  fwd_set_src(f, 0, a.lane_obs, S, S);
  fwd_set_out(f, a.workspace, a.head == 0 ? 1 : 0, a.p.max_action);
  if (a.precision != PREC_F32) fwd_set_planes(f, a.policy_blob_T, La);
  rc = launch_mlp3_forward(f, 1, ACT_RELU, a.precision, st);
  if (rc) return rc;
  InteractArgs ia{};
  ia.p = a.p; ia.pol = a.workspace; ia.head = a.head; ia.time_limit = a.time_limit; ia.packed = view_packed(g, S, A) ? 1 : 0;
  ia.expl = a.expl; ia.init_std = a.init_std; ia.seed = a.seed; ia.call0 = a.call0; ia.lanes = a.lanes; ia.cap = a.cap; ia.ring = g;
  ia.ptr_size = (const long long*)a.ptr_size; ia.count = (const long long*)a.count; ia.lane_obs = a.lane_obs; ia.lane_t = a.lane_t;
  ia.lane_ep = a.lane_ep; ia.done_count = a.done_count; ia.len_sum = a.len_sum; ia.lane_ret = a.lane_ret; ia.ret_sum = a.ret_sum;
  const int rpb = 256 / S;
  hipLaunchKernelGGL(k_task_interact, dim3((unsigned)cdiv(a.lanes, rpb)), dim3(256), 0, st, ia, rpb);
  MB_LAUNCH_OK("k_task_interact");
  hipLaunchKernelGGL(k_task_commit, dim3(1), dim3(1), 0, st, (long long*)a.ptr_size, (long long*)a.count, (long long)a.lanes, (long long)a.cap);
  MB_LAUNCH_OK("k_task_commit");
  return 0;
}
