// The analytic off-dynamics control task, stepped on the device (the specification is the docstring of
// mobody_amd/task.py, the fp64 restatement tests/task_ref.py).  The reference has no counterpart: its ground truth is a simulator.
//
//   k_task<STEP>     mobody_task_step: next, reward, terminal of B rows
//   k_task<EVAL>     mobody_task_evaluate's k_task_advance: the step on the row state + k_eval_account's accounting; at head 2 it
//                    also forms the built-in controller's action
//   k_task<COLLECT>  mobody_task_collect: controller, step, record row b L + t, reset of a finished lane
//   k_task_lanes     the lanes' first start states
//
// One body for the three: k_dyn_sample's geometry, a workgroup owns rpb = 256 / S whole rows staged in LDS, one thread per (row,
// dim) element, then one thread per row for the reward, the predicate and the row's bookkeeping.  Every product and sum is an
// fp32 operation of its own in a fixed order (the build has no contraction), so the three kernels give one set of bits.  No flags,
// tickets or atomics; every loop is bounded by an argument.  A translation unit of its own, linked after trajectory_summary.hip:
// every older code object keeps its bytes (tools/isa_diff.py).  Cost: a row is 2 S + A + 2 floats of traffic and O(S A) flops; a
// step is a launch's latency until B S reaches millions.
#include <math.h>

#include "common.h"
#include "layers.h"
#include "rng.h"
#include "term.h"

namespace mobody {

constexpr uint32_t STREAM_TASK = MOBODY_TASK_STREAM_NOISE, STREAM_TASK_ACTION = MOBODY_TASK_STREAM_ACTION,
                   STREAM_TASK_START = MOBODY_TASK_STREAM_START;
constexpr int TASK_S_MAX = 256, TASK_A_MAX = 64;
constexpr int TASK_MAX_U = (256 / 3) * TASK_A_MAX;       // rows per workgroup x A at the smallest S

enum TaskMode { TASK_STEP = 0, TASK_EVAL = 1, TASK_COLLECT = 2 };

struct TaskArgs {
  MobodyTaskParams p;
  const float* obs;           // [B][S]: the rows' states (EVAL: obs_state, COLLECT: the lanes' states)
  const float* act;           // [B][A] (unused under a controller)
  const float* noise;         // [B][S] or null
  const uint8_t* alive_in;    // STEP: [B] or null
  uint32_t seed, call;
  const long long* call_dev;
  long long B;
  float* next_obs;            // [B][S] (EVAL: obs_state, COLLECT: the lanes' states)
  float* reward;              // STEP: [B]
  uint8_t* terminal;          // STEP: [B]
  // built-in controllers (EVAL head 2, COLLECT): rows b < split run controller 0, the others controller 1
  int use_ctrl, ctrl[2];
  float push[2], eps[2];
  long long split;
  // EVAL: the row state
  uint8_t* alive;
  float *ret, *disc;
  int32_t* length;
  float discount;
  // COLLECT: step t of L, the tables and the lanes' counters
  int t, L, time_limit;
  float init_std;
  float *observations, *actions, *next_observations, *rewards;
  uint8_t* terminals;
  int32_t *lane_t, *lane_ep;
};

// a_j of a built-in controller; i = b A + j is the element of the action stream
__device__ __forceinline__ float task_controller(int kind, float push, float eps, float z1, float v, int j, uint32_t seed,
                                                 uint32_t call, uint64_t i) {
  if (kind == MOBODY_TASK_CTRL_RANDOM) {
    const U4 r = philox4x32_10((uint32_t)(i >> 2), call, 0u, 0u, seed, STREAM_TASK_ACTION);
    const int w = (int)(i & 3);
    const uint32_t x = w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
    return 2.f * rng_u01(x) - 1.f;
  }
  const float base = j == 0 ? (-6.f * z1) + 0.15f * v : push;
  const float a = eps != 0.f ? base + eps * rng_normal_at(seed, STREAM_TASK_ACTION, call, i) : base;
  return fminf(fmaxf(a, -1.f), 1.f);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_task(TaskArgs a, int rpb) {
  __shared__ float s_z[256], s_nxt[256], s_vp[256], s_u[TASK_MAX_U];
  __shared__ int s_reset[256], s_ep[256];
  const MobodyTaskParams& p = a.p;
  const int S = p.S, A = p.A;
  const int tid = threadIdx.x;
  const int r = tid / S, d = tid - r * S;
  const long long row0 = (long long)blockIdx.x * rpb;
  const long long b = row0 + r;
  const bool has = r < rpb && b < a.B;
  const int rows_here = (int)min((long long)rpb, a.B - row0);
  const uint32_t call = a.call + (a.call_dev != nullptr ? (uint32_t)a.call_dev[0] : 0u);
  float sv = 0.f, mu_d = 0.f;
  if (has) {
    mu_d = p.mu[d];
    sv = a.obs[b * S + d];
    s_z[tid] = sv - mu_d;                                                    // z = s - mu
  }
  __syncthreads();
  for (int t = tid; t < rows_here * A; t += 256) {                           // u_j = gain_j clamp(a_j / max_action, -1, 1)
    const int rr = t / A, j = t - rr * A;
    const long long bb = row0 + rr;
    float act;
    if (MODE == TASK_STEP || (MODE == TASK_EVAL && !a.use_ctrl)) {
      act = a.act[bb * A + j];
    } else {
      const int w = bb < a.split ? 0 : 1;
      act = task_controller(a.ctrl[w], a.push[w], a.eps[w], s_z[rr * S + 1], s_z[rr * S + S - 1], j, a.seed, call, (uint64_t)bb * A + j);
      if (MODE == TASK_COLLECT) a.actions[(bb * a.L + a.t) * A + j] = act;
    }
    s_u[t] = p.gain[j] * fminf(fmaxf(act / p.max_action, -1.f), 1.f);
  }
  __syncthreads();
  float nxt = 0.f;
  if (has) {
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
    if (p.sigma != 0.f) {
      const float e = a.noise != nullptr ? a.noise[b * S + d] : rng_normal_at(a.seed, STREAM_TASK, call, (uint64_t)b * S + d);
      zp += p.sigma * e;
    }
    nxt = zp + mu_d;
    s_nxt[tid] = nxt;
    if (d == S - 1) s_vp[r] = zp;
    if (MODE == TASK_COLLECT) {
      const long long row = b * a.L + a.t;
      a.observations[row * S + d] = sv;
      a.next_observations[row * S + d] = nxt;
    } else {
      a.next_obs[b * S + d] = nxt;
    }
  }
  __syncthreads();
  if (tid < rows_here) {                                                     // one thread per row
    const long long bb = row0 + tid;
    const float* u = s_u + tid * A;
    float m = u[0] * u[0];
    for (int j = 1; j < A; ++j) m += u[j] * u[j];
    m = m / (float)A;
    const float rew = (s_vp[tid] + p.alive_bonus) - p.ctrl_cost * m;
    const bool done = term_predicate(p.task, s_nxt + tid * S, S);
    if (MODE == TASK_STEP) {
      const bool was_alive = a.alive_in != nullptr ? a.alive_in[bb] != 0 : true;
      a.reward[bb] = rew;
      a.terminal[bb] = (done && was_alive) ? 1 : 0;
    } else if (MODE == TASK_EVAL) {
      if (a.alive[bb]) {                                                     // k_eval_account's accounting
        const float dd = a.disc[bb];
        a.ret[bb] = fmaf(dd, rew, a.ret[bb]);
        a.length[bb] += 1;
        a.disc[bb] = dd * a.discount;
        if (done) a.alive[bb] = 0;
      }
    } else {
      const long long row = bb * a.L + a.t;
      a.rewards[row] = rew;
      a.terminals[row] = done ? 1 : 0;
      const int lt = a.lane_t[bb] + 1;
      const int reset = (done || lt >= a.time_limit) ? 1 : 0;
      const int ep = a.lane_ep[bb] + reset;
      a.lane_t[bb] = reset ? 0 : lt;
      a.lane_ep[bb] = ep;
      s_reset[tid] = reset;
      s_ep[tid] = ep;
    }
  }
  if (MODE == TASK_COLLECT) {
    __syncthreads();
    if (has)                                                                 // the lane goes on, or its next episode starts here
      a.next_obs[b * S + d] = s_reset[r] ? mu_d + a.init_std * rng_normal_at(a.seed, STREAM_TASK_START, (uint32_t)s_ep[r], (uint64_t)b * S + d)
                                         : nxt;
  }
}

__global__ __launch_bounds__(256) void k_task_lanes(const float* mu, float init_std, uint32_t seed, long long lanes, int S,
                                                    float* lane_obs, int32_t* lane_t, int32_t* lane_ep) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < lanes * S) lane_obs[i] = mu[i % S] + init_std * rng_normal_at(seed, STREAM_TASK_START, 0u, (uint64_t)i);
  if (i < lanes) { lane_t[i] = 0; lane_ep[i] = 0; }
}

static int check_task(const char* who, const MobodyTaskParams& p) {
  MB_REQUIRE(p.S >= 3 && p.S <= TASK_S_MAX, "%s: S %d outside [3, %d]", who, p.S, TASK_S_MAX);
  MB_REQUIRE(p.A >= 1 && p.A <= TASK_A_MAX, "%s: A %d outside [1, %d]", who, p.A, TASK_A_MAX);
  MB_REQUIRE(p.task >= MOBODY_TERM_NEVER && p.task <= MOBODY_TERM_PEN, "%s: unknown termination id %d (task)", who, p.task);
  MB_REQUIRE(p.task != MOBODY_TERM_PEN || p.S > 26, "%s: pen predicate needs S > 26 (task)", who);
  MB_REQUIRE(p.max_action > 0.f, "%s: max_action %g is not positive", who, (double)p.max_action);
  MB_REQUIRE(p.mu != nullptr, "%s: null pointer mu", who);
  MB_REQUIRE(p.gain != nullptr, "%s: null pointer gain", who);
  MB_REQUIRE(p.bmat != nullptr, "%s: null pointer bmat", who);
  return 0;
}

static int check_ctrl(const char* who, int ctrl) {
  MB_REQUIRE(ctrl == MOBODY_TASK_CTRL_RANDOM || ctrl == MOBODY_TASK_CTRL_FEEDBACK, "%s: ctrl %d outside {0 (random), 1 (feedback)}", who, ctrl);
  return 0;
}

#define MB_NONNULL(who, blk, f) MB_REQUIRE((blk).f != nullptr, "%s: null pointer " #f, who)

template <int MODE>
static int launch_task(const TaskArgs& ta, const char* name, hipStream_t st) {
  const int rpb = 256 / ta.p.S;
  hipLaunchKernelGGL(k_task<MODE>, dim3((unsigned)cdiv(ta.B, rpb)), dim3(256), 0, st, ta, rpb);
  MB_LAUNCH_OK(name);
  return 0;
}

struct TaskEvalWs { float *act, *act2; long long total; };
static void task_eval_carve(int A, long long B, int head, float* base, TaskEvalWs& w) {
  Carver take{base};
  w.act = take(B * A);
  w.act2 = head == 1 ? take(B * 2 * A) : nullptr;
  w.total = take.off;
}

struct TaskCollectWs { float* lane_obs; int32_t *lane_t, *lane_ep; long long total; };
static void task_collect_carve(int S, long long lanes, float* base, TaskCollectWs& w) {
  Carver take{base};
  w.lane_obs = take(lanes * S); w.lane_t = (int32_t*)take(lanes); w.lane_ep = (int32_t*)take(lanes);
  w.total = take.off;
}

}  // namespace mobody

using namespace mobody;

extern "C" int mobody_task_step(const MobodyTaskStep* ap, void* stream) {
  const char* who = "mobody_task_step";
  MB_BLOCK(who, ap, MobodyTaskStep);
  const MobodyTaskStep& a = *ap;
  int rc = check_task(who, a.p);
  if (rc) return rc;
  MB_REQUIRE(a.B >= 0, "%s: B < 0", who);
  if (a.B == 0) return 0;
  MB_NONNULL(who, a, obs); MB_NONNULL(who, a, act); MB_NONNULL(who, a, next_obs); MB_NONNULL(who, a, reward); MB_NONNULL(who, a, terminal);
  TaskArgs ta{};
  ta.p = a.p; ta.obs = a.obs; ta.act = a.act; ta.noise = a.noise; ta.alive_in = a.alive; ta.seed = a.seed; ta.call = a.call;
  ta.call_dev = (const long long*)a.call_dev; ta.B = a.B; ta.next_obs = a.next_obs; ta.reward = a.reward; ta.terminal = a.terminal;
  return launch_task<TASK_STEP>(ta, "k_task_step", as_stream(stream));
}

extern "C" int64_t mobody_task_evaluate_workspace(const MobodyTaskEval* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyTaskEval) || a->B < 0 || a->p.A < 1 || a->head < 0 || a->head > 2)
    return fail(MOBODY_E_ARG, "mobody_task_evaluate_workspace: null struct, wrong struct_bytes, B < 0, A < 1 or head outside {0, 1, 2}");
  TaskEvalWs w;
  task_eval_carve(a->p.A, a->B, a->head, nullptr, w);
  return w.total;
}

extern "C" int mobody_task_evaluate(const MobodyTaskEval* ap, void* stream) {
  const char* who = "mobody_task_evaluate";
  MB_BLOCK(who, ap, MobodyTaskEval);
  const MobodyTaskEval& a = *ap;
  const int S = a.p.S, A = a.p.A;
  const int64_t B = a.B;
  int rc = check_task(who, a.p);
  if (rc) return rc;
  MB_REQUIRE(B >= 0, "%s: B < 0", who);
  MB_REQUIRE(a.H >= 0, "%s: H < 0", who);
  MB_REQUIRE(a.resume == 0 || a.resume == 1, "%s: resume %d is neither 0 nor 1", who, a.resume);
  MB_REQUIRE(a.discount > 0.f && a.discount <= 1.f, "%s: discount %g outside (0, 1]", who, (double)a.discount);   // NaN fails both
  MB_REQUIRE(a.head >= 0 && a.head <= 2, "%s: head %d outside {0 (deterministic actor), 1 (Gaussian policy), 2 (built-in controller)}", who, a.head);
  if (a.head == 2 && (rc = check_ctrl(who, a.ctrl))) return rc;
  if (B == 0) return 0;
  MobodyMlpLayout La{};
  if (a.head != 2) {
    MB_REQUIRE(a.head == 0 || 2 * A <= 128, "%s: A %d: the Gaussian policy's 2 A outputs must fit 128 columns (head 1)", who, A);
    MB_NONNULL(who, a, policy_blob);
    rc = check_precision(who, a.precision, a.policy_blob_T != nullptr);
    if (rc) return rc;
    rc = mobody_mlp_layout(S, a.head == 1 ? 2 * A : A, 1, &La);
    if (rc) return rc;
  }
  MB_REQUIRE(a.resume == 1 || a.init_obs, "%s: null pointer init_obs (resume == 0)", who);
  MB_NONNULL(who, a, obs_state); MB_NONNULL(who, a, alive); MB_NONNULL(who, a, ret); MB_NONNULL(who, a, pen_sum);
  MB_NONNULL(who, a, disc); MB_NONNULL(who, a, length);
  MB_NONNULL(who, a, workspace);
  TaskEvalWs w;
  task_eval_carve(A, B, a.head, a.workspace, w);
  hipStream_t st = as_stream(stream);
  const DynEvalHook hook{a.obs_state, a.alive, a.ret, a.pen_sum, a.disc, a.length, a.discount};
  if (a.resume == 0 && (rc = launch_eval_init(a.init_obs, hook, B, S, st))) return rc;
  TaskArgs ta{};
  ta.p = a.p; ta.obs = a.obs_state; ta.act = w.act; ta.seed = a.seed; ta.call_dev = (const long long*)a.call_dev; ta.B = B;
  ta.next_obs = a.obs_state; ta.use_ctrl = a.head == 2; ta.ctrl[0] = ta.ctrl[1] = a.ctrl; ta.push[0] = ta.push[1] = a.ctrl_push;
  ta.eps[0] = ta.eps[1] = a.ctrl_eps; ta.split = B; ta.alive = a.alive; ta.ret = a.ret; ta.disc = a.disc; ta.length = a.length;
  ta.discount = a.discount;
  for (int t = 0; t < a.H; ++t) {
    if (a.head != 2) {                                   // a = pi(s): Policy::launch's forward (dynamics.hip)
      Mlp3FwdArgs f = fwd_net(a.policy_blob, La, B);
      fwd_set_src(f, 0, a.obs_state, S, S);
      fwd_set_out(f, a.head == 1 ? w.act2 : w.act, 1, a.p.max_action);
      if (a.precision != PREC_F32) fwd_set_planes(f, a.policy_blob_T, La);
      rc = launch_mlp3_forward(f, 1, ACT_RELU, a.precision, st);
      if (rc) return rc;
      if (a.head == 1 && (rc = launch_fqe_action(w.act2, 2 * A, B, A, w.act, st))) return rc;   // tanh(mu): columns [0, A)
    }
    ta.call = a.call0 + (uint32_t)t;
    rc = launch_task<TASK_EVAL>(ta, "k_task_advance", st);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int64_t mobody_task_collect_workspace(const MobodyTaskCollect* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyTaskCollect) || a->lanes < 0 || a->p.S < 1)
    return fail(MOBODY_E_ARG, "mobody_task_collect_workspace: null struct, wrong struct_bytes, lanes < 0 or S < 1");
  TaskCollectWs w;
  task_collect_carve(a->p.S, a->lanes, nullptr, w);
  return w.total;
}

extern "C" int mobody_task_collect(const MobodyTaskCollect* ap, void* stream) {
  const char* who = "mobody_task_collect";
  MB_BLOCK(who, ap, MobodyTaskCollect);
  const MobodyTaskCollect& a = *ap;
  int rc = check_task(who, a.p);
  if (rc) return rc;
  MB_REQUIRE(a.lanes >= 0, "%s: lanes < 0", who);
  MB_REQUIRE(a.L >= 0, "%s: L < 0", who);
  MB_REQUIRE(a.time_limit >= 1, "%s: time_limit %d < 1", who, a.time_limit);
  MB_REQUIRE(a.split >= 0 && a.split <= a.lanes, "%s: split %lld outside [0, lanes]", who, (long long)a.split);
  if ((rc = check_ctrl(who, a.ctrl[0])) || (rc = check_ctrl(who, a.ctrl[1]))) return rc;
  if (a.lanes == 0 || a.L == 0) return 0;
  MB_NONNULL(who, a, observations); MB_NONNULL(who, a, actions); MB_NONNULL(who, a, next_observations); MB_NONNULL(who, a, rewards);
  MB_NONNULL(who, a, terminals); MB_NONNULL(who, a, workspace);
  TaskCollectWs w;
  task_collect_carve(a.p.S, a.lanes, a.workspace, w);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_task_lanes, dim3((unsigned)cdiv(a.lanes * a.p.S, 256)), dim3(256), 0, st, a.p.mu, a.init_std, a.seed,
                     (long long)a.lanes, a.p.S, w.lane_obs, w.lane_t, w.lane_ep);
  MB_LAUNCH_OK("k_task_lanes");
  TaskArgs ta{};
  ta.p = a.p; ta.obs = w.lane_obs; ta.next_obs = w.lane_obs; ta.seed = a.seed; ta.B = a.lanes; ta.use_ctrl = 1; ta.split = a.split;
  for (int k = 0; k < 2; ++k) { ta.ctrl[k] = a.ctrl[k]; ta.push[k] = a.ctrl_push[k]; ta.eps[k] = a.ctrl_eps[k]; }
  ta.L = a.L; ta.time_limit = a.time_limit; ta.init_std = a.init_std; ta.observations = a.observations; ta.actions = a.actions;
  ta.next_observations = a.next_observations; ta.rewards = a.rewards; ta.terminals = a.terminals; ta.lane_t = w.lane_t; ta.lane_ep = w.lane_ep;
  for (int t = 0; t < a.L; ++t) {
    ta.t = t; ta.call = a.call0 + (uint32_t)t;
    rc = launch_task<TASK_COLLECT>(ta, "k_task_collect", st);
    if (rc) return rc;
  }
  return 0;
}
