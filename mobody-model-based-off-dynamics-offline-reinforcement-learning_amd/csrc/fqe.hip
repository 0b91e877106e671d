// Fitted Q evaluation: the bootstrap value mean Q_targ(s', pi(s')) of a frozen policy and the estimate over start
// states, for both policy head forms of the six algorithm classes.  The reference has no counterpart.  No flags, tickets or
// atomics; every loop is bounded by an argument; every sum and maximum runs in a fixed order.
#include <math.h>

#include "common.h"

namespace mobody {

// dst [n][A] = columns [0, A) of src [n][pitch], one element per thread and trip: the Gaussian head's tanh(mu) half
__global__ __launch_bounds__(256) void k_fqe_action(const float* src, int pitch, long long n, int A, float* dst) {
  const long long total = n * A;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / A;
    dst[i] = src[row * pitch + (i - row * A)];
  }
}

// A row with a NaN among its state or action: the packed forwards' ReLU is fmaxf(., 0), which turns a NaN pre-activation into 0,
// so the NaN never reaches q (k_bosa_qnext).
__device__ __forceinline__ bool fqe_row_bad(const float* state, const float* act, long long i, int S, int A) {
  bool bad = false;
  for (int d = 0; d < S; ++d) bad = bad || state[i * S + d] != state[i * S + d];
  for (int j = 0; j < A; ++j) bad = bad || act[i * A + j] != act[i * A + j];
  return bad;
}

// q_next[i] = (q[0][i] + q[1][i]) * 0.5, two fp32 operations each rounded once; a row with a NaN input gets NaN.  action_out
// (nullable) takes the row's a' on the way.
__global__ __launch_bounds__(256) void k_fqe_qnext(const float* q, const float* next_state, const float* a2, long long N, int S, int A,
                                                   float* q_next, float* action_out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
    const float v = __fmul_rn(__fadd_rn(q[i], q[N + i]), 0.5f);
    q_next[i] = fqe_row_bad(next_state, a2, i, S, A) ? __builtin_nanf("") : v;
    if (action_out != nullptr)
      for (int j = 0; j < A; ++j) action_out[i * A + j] = a2[i * A + j];
  }
}

// the start-value rows: a row with a NaN input gets q = NaN in both members (in place); q_out (nullable) takes the rows
__global__ __launch_bounds__(256) void k_fqe_value_rows(float* q, const float* state, const float* act, long long B, int S, int A,
                                                        float* q_out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < B; i += (long long)gridDim.x * 256) {
    if (fqe_row_bad(state, act, i, S, A)) q[i] = q[B + i] = __builtin_nanf("");
    if (q_out != nullptr) { q_out[i] = q[i]; q_out[B + i] = q[B + i]; }
  }
}

// out[4] = (mean q0, mean q1, mean 0.5 (q0 + q1), max |q0 - q1|), nan_flag = 1 when a q is NaN.  One workgroup: thread t takes
// rows t, t + 256, ... in ascending order, then a fixed tree (k_bosa_stage2_words' scheme).  The third word is (sum q0 + sum q1) /
// (2 B) of the two reduced sums.  A NaN gives NaN in all four words.
__global__ __launch_bounds__(256) void k_fqe_value(const float* q, long long B, float* out, int* nan_flag) {
  __shared__ float r0[256], r1[256], rgap[256];
  __shared__ int rbad[256];
  const int t = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, gap = 0.f;
  int bad = 0;
  for (long long i = t; i < B; i += 256) {
    const float q0 = q[i], q1 = q[B + i];
    s0 += q0;
    s1 += q1;
    bad |= (q0 != q0) | (q1 != q1);
    gap = fmaxf(gap, fabsf(__fsub_rn(q0, q1)));
  }
  r0[t] = s0; r1[t] = s1; rgap[t] = gap; rbad[t] = bad;
  __syncthreads();
#pragma unroll
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) { r0[t] += r0[t + h]; r1[t] += r1[t + h]; rgap[t] = fmaxf(rgap[t], rgap[t + h]); rbad[t] |= rbad[t + h]; }
    __syncthreads();
  }
  if (t != 0) return;
  const float n = (float)B;
  out[0] = r0[0] / n;
  out[1] = r1[0] / n;
  out[2] = __fadd_rn(r0[0], r1[0]) / (2.f * n);
  out[3] = rbad[0] ? __builtin_nanf("") : rgap[0];
  nan_flag[0] = rbad[0];
}

static constexpr unsigned FQE_PREC = 1u << PREC_F32 | 1u << PREC_BF16X3 | 1u << PREC_F16X2;
constexpr long long FQE_MAX_ROWS = 1 << 21;
constexpr long long FQE_MAX_GRID = 1 << 16;      // workgroups of a grid-stride launch: sized from the rows, bounded by the device's reach

static unsigned fqe_grid(long long n) { return (unsigned)(cdiv(n, 256) < FQE_MAX_GRID ? cdiv(n, 256) : FQE_MAX_GRID); }

// the checks the two blocks share (their leading fields are the same; `rows` is N or B under its own name)
static int fqe_dims(const char* who, int head, int S, int A, long long rows, const char* rows_name) {
  MB_REQUIRE(head == 0 || head == 1, "%s: head %d outside {0 (deterministic actor), 1 (Gaussian policy)}", who, head);
  MB_REQUIRE(S >= 1 && S <= 256, "%s: S %d outside [1, 256]", who, S);
  if (head == 0)
    MB_REQUIRE(A >= 1 && A <= 128, "%s: A %d outside [1, 128]", who, A);
  else
    MB_REQUIRE(A >= 1 && 2 * A <= 128, "%s: A %d: the Gaussian head's 2 A outputs must fit 128 columns", who, A);
  MB_REQUIRE(S + A <= 256, "%s: S + A = %d > 256", who, S + A);
  MB_REQUIRE(rows >= 1 && rows <= FQE_MAX_ROWS, "%s: %s %lld outside [1, 2^21]", who, rows_name, rows);
  return 0;
}

// the launch of k_fqe_action (declared in common.h: mobody_ens_evaluate_policy's head 1 takes the same copy)
int launch_fqe_action(const float* src, int pitch, long long n, int A, float* dst, hipStream_t st) {
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_fqe_action, dim3(fqe_grid(n * A)), dim3(256), 0, st, src, pitch, n, A, dst);
  MB_LAUNCH_OK("k_fqe_action");
  return 0;
}

struct FqeWs {
  float *pi2, *pi, *q;
  long long floats;
};
static void fqe_carve(int head, int A, long long rows, float* base, FqeWs& w) {
  Carver take{base};
  w.pi = take(rows * A);
  w.q = take(2 * rows);
  w.pi2 = head == 1 ? take(rows * 2 * A) : nullptr;
  w.floats = take.off;
}

// pi(state) by the head rule into w.pi, then the twin-Q forward on [state | pi] into w.q: 2 launches (head 0) or 3 (head 1)
static int fqe_forwards(int prec, int head, int S, int A, long long rows, const float* policy_blob, const float* policy_blob_T,
                        const float* q_blob, const float* q_blob_T, const float* state, float max_action, const FqeWs& w, void* stream) {
  hipStream_t st = as_stream(stream);
  const float *pT = prec != PREC_F32 ? policy_blob_T : nullptr, *qT = prec != PREC_F32 ? q_blob_T : nullptr;
  int rc;
  if ((rc = mobody_mlp3_forward(policy_blob, pT, prec, S, head == 1 ? 2 * A : A, 1, state, S, nullptr, 0, rows, 1, max_action,
                                head == 1 ? w.pi2 : w.pi, nullptr, nullptr, nullptr, stream)))
    return rc;
  if (head == 1 && (rc = launch_fqe_action(w.pi2, 2 * A, rows, A, w.pi, st))) return rc;
  return mobody_mlp3_forward(q_blob, qT, prec, S + A, 1, 2, state, S, w.pi, A, rows, 0, 1.f, w.q, nullptr, nullptr, nullptr, stream);
}

}  // namespace mobody

using namespace mobody;

static int fqe_target_dims(const char* who, const MobodyFqeTarget* a) {
  MB_BLOCK(who, a, MobodyFqeTarget);
  return fqe_dims(who, a->head, a->S, a->A, (long long)a->N, "N");
}

extern "C" int64_t mobody_fqe_target_workspace(const MobodyFqeTarget* a) {
  if (fqe_target_dims("mobody_fqe_target_workspace", a)) return -1;
  FqeWs w;
  fqe_carve(a->head, a->A, a->N, nullptr, w);
  return w.floats;
}

extern "C" int mobody_fqe_target(const MobodyFqeTarget* a, void* stream) {
  const char* who = "mobody_fqe_target";
  int rc = fqe_target_dims(who, a);
  if (rc) return rc;
  if ((rc = check_precision(who, a->precision, a->policy_blob_T && a->q_blob_T, FQE_PREC))) return rc;
  MB_REQUIRE(a->policy_blob != nullptr, "%s: policy_blob is NULL", who);
  MB_REQUIRE(a->q_blob != nullptr, "%s: q_blob is NULL", who);
  MB_REQUIRE(a->next_state != nullptr, "%s: next_state is NULL", who);
  MB_REQUIRE(a->q_next != nullptr, "%s: q_next is NULL", who);
  MB_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
  MB_REQUIRE(a->max_action > 0.f, "%s: max_action %g <= 0 (or NaN)", who, (double)a->max_action);
  FqeWs w;
  fqe_carve(a->head, a->A, a->N, a->workspace, w);
  if ((rc = fqe_forwards(a->precision, a->head, a->S, a->A, a->N, a->policy_blob, a->policy_blob_T, a->q_blob, a->q_blob_T, a->next_state,
                         a->max_action, w, stream)))
    return rc;
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_fqe_qnext, dim3(fqe_grid(a->N)), dim3(256), 0, st, (const float*)w.q, a->next_state, (const float*)w.pi, (long long)a->N,
                     a->S, a->A, a->q_next, a->action_out);
  MB_LAUNCH_OK("k_fqe_qnext");
  return 0;
}

static int fqe_value_dims(const char* who, const MobodyFqeValue* a) {
  MB_BLOCK(who, a, MobodyFqeValue);
  return fqe_dims(who, a->head, a->S, a->A, (long long)a->B, "B");
}

extern "C" int64_t mobody_fqe_value_workspace(const MobodyFqeValue* a) {
  if (fqe_value_dims("mobody_fqe_value_workspace", a)) return -1;
  FqeWs w;
  fqe_carve(a->head, a->A, a->B, nullptr, w);
  return w.floats;
}

extern "C" int mobody_fqe_value(const MobodyFqeValue* a, void* stream) {
  const char* who = "mobody_fqe_value";
  int rc = fqe_value_dims(who, a);
  if (rc) return rc;
  if ((rc = check_precision(who, a->precision, a->policy_blob_T && a->q_blob_T, FQE_PREC))) return rc;
  MB_REQUIRE(a->policy_blob != nullptr, "%s: policy_blob is NULL", who);
  MB_REQUIRE(a->q_blob != nullptr, "%s: q_blob is NULL", who);
  MB_REQUIRE(a->state != nullptr, "%s: state is NULL", who);
  MB_REQUIRE(a->out != nullptr, "%s: out is NULL", who);
  MB_REQUIRE(a->nan_flag != nullptr, "%s: nan_flag is NULL", who);
  MB_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
  MB_REQUIRE(a->max_action > 0.f, "%s: max_action %g <= 0 (or NaN)", who, (double)a->max_action);
  FqeWs w;
  fqe_carve(a->head, a->A, a->B, a->workspace, w);
  if ((rc = fqe_forwards(a->precision, a->head, a->S, a->A, a->B, a->policy_blob, a->policy_blob_T, a->q_blob, a->q_blob_T, a->state,
                         a->max_action, w, stream)))
    return rc;
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_fqe_value_rows, dim3(fqe_grid(a->B)), dim3(256), 0, st, w.q, a->state, (const float*)w.pi, (long long)a->B, a->S, a->A,
                     a->q_out);
  MB_LAUNCH_OK("k_fqe_value_rows");
  hipLaunchKernelGGL(k_fqe_value, dim3(1), dim3(256), 0, st, (const float*)w.q, (long long)a->B, a->out, a->nan_flag);
  MB_LAUNCH_OK("k_fqe_value");
  return 0;
}
