// BOSA's critic / actor stage, the row-wise pieces between its launches (the reference's bosa.py:565-634): the clipped
// target action and the bootstrap value min Q_target(s', a'), the critic's row weights, the estimator's addend to d loss / d pi, and
// the eight logged words.  With these a stage-2 call holds only this library's launches and can be captured as a HIP graph.  No
// flags, tickets or atomics; every loop is bounded by an argument; every sum and maximum runs in a fixed order.
#include <math.h>

#include "common.h"
#include "rng.h"

namespace mobody {

constexpr int BOSA_ROW_GRID = 4;     // workgroups of the grid-stride kernels: the stage's batches are a few hundred rows

// torch.clamp(x, lo, hi) with lo <= hi: a NaN stays a NaN
__device__ __forceinline__ float clamp_nan(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// a' = clamp(pi + clamp(noise * expl_noise, -clip, clip), -max_action, max_action) in place over pi [N][A], one element per thread
// and trip (bosa.py:571-575).  noise == null: element i of stream MOBODY_BOSA_STREAM_TARGET_NOISE at call + call_dev[0].  Four fp32
// operations, each rounded once (the build contracts nothing; the intrinsics say so here).
struct TargetActionArgs {
  float* pi;
  const float* noise;
  long long total;
  uint32_t seed, call;
  const long long* call_dev;
  float expl_noise, noise_clip, max_action;
};
__global__ __launch_bounds__(256) void k_bosa_target_action(TargetActionArgs a) {
  const uint32_t call = a.call + (a.call_dev ? (uint32_t)a.call_dev[0] : 0u);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (long long)gridDim.x * 256) {
    const float n = a.noise != nullptr ? a.noise[i] : rng_normal_at(a.seed, MOBODY_BOSA_STREAM_TARGET_NOISE, call, (uint64_t)i);
    const float scaled = __fmul_rn(n, a.expl_noise);
    const float clipped = clamp_nan(scaled, -a.noise_clip, a.noise_clip);
    const float moved = __fadd_rn(a.pi[i], clipped);
    a.pi[i] = clamp_nan(moved, -a.max_action, a.max_action);
  }
}

// q_next[i] = min(q[0][i], q[1][i]); a NaN member gives NaN, as torch.min and k_bosa_ll_reduce's min_ll do (fminf would skip it).
// The packed forwards' ReLU is fmaxf(., 0), which turns a NaN pre-activation into 0, so a NaN in a row's s' or a' never reaches q;
// torch's relu keeps it.  The row's inputs are therefore looked at here: a NaN among them gives the row NaN, as torch would.
__global__ __launch_bounds__(256) void k_bosa_qnext(const float* q, const float* next_state, const float* a2, long long N, int S, int A,
                                                    float* q_next) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
    const float q0 = q[i], q1 = q[N + i];
    float v = q0 != q0 ? q0 : (q1 != q1 ? q1 : fminf(q0, q1));
    bool bad = false;
    for (int d = 0; d < S; ++d) bad = bad || next_state[i * S + d] != next_state[i * S + d];
    for (int j = 0; j < A; ++j) bad = bad || a2[i * A + j] != a2[i * A + j];
    q_next[i] = bad ? __builtin_nanf("") : v;
  }
}

// row_weight = mask * 0.5 (n_mask elements) and / or dpi = dll * scale (n_dll elements): single multiplies, torch.mul's bits
__global__ __launch_bounds__(256) void k_bosa_stage2_rows(const float* mask, long long n_mask, float* row_weight, const float* dll,
                                                          long long n_dll, float scale, float* dpi) {
  const long long step = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long i = first; i < n_mask; i += step) row_weight[i] = __fmul_rn(mask[i], 0.5f);
  for (long long i = first; i < n_dll; i += step) dpi[i] = __fmul_rn(dll[i], scale);
}

// The logged words, one workgroup.  Critic part (closs != null): words[0] = mask_mean, [1] = closs[0], [3] = closs[1], [2] = closs[0]
// - cons_coef * closs[1].  Actor part (ll != null): words[5] = mean(-ll), words[6] = max(-ll) with a NaN kept, words[4] = aloss[0] +
// lamda * words[5]; thread t takes rows t, t + 256, ... in ascending order, then a fixed tree.  Last, thread 0 adds bump_inc[k] to
// bump[k]: a captured call advances its call id, step counts and draw count here.
struct Stage2WordsArgs {
  const float *mask_mean, *closs, *ll, *aloss;
  long long N;
  float cons_coef, lamda;
  float* words;
  long long* bump;
  long long bump_inc[4];
  int nbump;
};
__global__ __launch_bounds__(256) void k_bosa_stage2_words(Stage2WordsArgs a) {
  __shared__ float rsum[256], rmax[256];
  __shared__ int rbad[256];
  const int t = threadIdx.x;
  if (a.ll != nullptr) {
    float s = 0.f, mx = -INFINITY;
    int bad = 0;
    for (long long i = t; i < a.N; i += 256) {
      const float v = -a.ll[i];
      s += v;
      bad |= v != v;
      mx = fmaxf(mx, v);
    }
    rsum[t] = s; rmax[t] = mx; rbad[t] = bad;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
      if (t < h) { rsum[t] += rsum[t + h]; rmax[t] = fmaxf(rmax[t], rmax[t + h]); rbad[t] |= rbad[t + h]; }
      __syncthreads();
    }
  }
  if (t != 0) return;
  if (a.closs != nullptr) {
    const float c0 = a.closs[0], c1 = a.closs[1];
    a.words[0] = a.mask_mean[0];
    a.words[1] = c0;
    a.words[3] = c1;
    a.words[2] = __fsub_rn(c0, __fmul_rn(c1, a.cons_coef));
  }
  if (a.ll != nullptr) {
    const float mean = rsum[0] / (float)a.N;
    a.words[5] = mean;
    a.words[6] = rbad[0] ? __builtin_nanf("") : rmax[0];
    a.words[4] = __fadd_rn(a.aloss[0], __fmul_rn(mean, a.lamda));
  }
  for (int k = 0; k < a.nbump; ++k) a.bump[k] += a.bump_inc[k];
}

static constexpr unsigned BOSA_TARGET_PREC = 1u << PREC_F32 | 1u << PREC_BF16X3 | 1u << PREC_F16X2;
constexpr long long BOSA_MAX_ROWS = 1 << 21;

static int target_dims(const char* who, const MobodyBosaTarget* a) {
  MB_BLOCK(who, a, MobodyBosaTarget);
  MB_REQUIRE(a->S >= 1 && a->S <= 256, "%s: S %d outside [1, 256]", who, a->S);
  MB_REQUIRE(a->A >= 1 && a->A <= 128, "%s: A %d outside [1, 128]", who, a->A);
  MB_REQUIRE(a->S + a->A <= 256, "%s: S + A = %d > 256", who, a->S + a->A);
  MB_REQUIRE(a->N >= 1 && a->N <= BOSA_MAX_ROWS, "%s: N %lld outside [1, 2^21]", who, (long long)a->N);
  return 0;
}

struct TargetWs {
  float *pi, *q;
  long long floats;
};
static void target_carve(const MobodyBosaTarget* a, float* base, TargetWs& w) {
  Carver take{base};
  w.pi = take(a->N * a->A);
  w.q = take(2 * a->N);
  w.floats = take.off;
}

static unsigned row_grid(long long n) { return (unsigned)(cdiv(n, 256) < BOSA_ROW_GRID ? cdiv(n, 256) : BOSA_ROW_GRID); }

}  // namespace mobody

using namespace mobody;

extern "C" int64_t mobody_bosa_target_workspace(const MobodyBosaTarget* a) {
  if (target_dims("mobody_bosa_target_workspace", a)) return -1;
  TargetWs w;
  target_carve(a, nullptr, w);
  return w.floats;
}

extern "C" int mobody_bosa_target(const MobodyBosaTarget* a, void* stream) {
  const char* who = "mobody_bosa_target";
  int rc = target_dims(who, a);
  if (rc) return rc;
  if ((rc = check_precision(who, a->precision, a->actor_blob_T && a->q_blob_T, BOSA_TARGET_PREC))) return rc;
  MB_REQUIRE(a->actor_blob != nullptr, "%s: actor_blob is NULL", who);
  MB_REQUIRE(a->q_blob != nullptr, "%s: q_blob is NULL", who);
  MB_REQUIRE(a->next_state != nullptr, "%s: next_state is NULL", who);
  MB_REQUIRE(a->q_next != nullptr, "%s: q_next is NULL", who);
  MB_REQUIRE(a->workspace != nullptr, "%s: workspace is NULL", who);
  MB_REQUIRE(a->noise_clip >= 0.f, "%s: noise_clip %g < 0 (or NaN)", who, (double)a->noise_clip);
  MB_REQUIRE(a->max_action > 0.f, "%s: max_action %g <= 0 (or NaN)", who, (double)a->max_action);
  MB_REQUIRE(a->expl_noise == a->expl_noise, "%s: expl_noise is NaN", who);
  TargetWs w;
  target_carve(a, a->workspace, w);
  hipStream_t st = as_stream(stream);
  const long long N = a->N;
  const int S = a->S, A = a->A, prec = a->precision;
  const float *aT = prec != PREC_F32 ? a->actor_blob_T : nullptr, *qT = prec != PREC_F32 ? a->q_blob_T : nullptr;
  if ((rc = mobody_mlp3_forward(a->actor_blob, aT, prec, S, A, 1, a->next_state, S, nullptr, 0, N, 1, a->max_action, w.pi, nullptr, nullptr,
                                nullptr, stream)))
    return rc;
  {
    TargetActionArgs t{};
    t.pi = w.pi; t.noise = a->noise; t.total = N * A; t.seed = a->seed; t.call = a->call; t.call_dev = (const long long*)a->call_dev;
    t.expl_noise = a->expl_noise; t.noise_clip = a->noise_clip; t.max_action = a->max_action;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_target_action, dim3(row_grid(t.total)), dim3(256), 0, st, t);
    MB_LAUNCH_OK("k_bosa_target_action");
  }
  if ((rc = mobody_mlp3_forward(a->q_blob, qT, prec, S + A, 1, 2, a->next_state, S, w.pi, A, N, 0, 1.f, w.q, nullptr, nullptr, nullptr, stream)))
    return rc;
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_qnext, dim3(row_grid(N)), dim3(256), 0, st, (const float*)w.q, a->next_state, (const float*)w.pi, N, S, A, a->q_next);
  MB_LAUNCH_OK("k_bosa_qnext");
  return 0;
}

static int stage2_check(const char* who, const MobodyBosaStage2* a) {
  MB_BLOCK(who, a, MobodyBosaStage2);
  MB_REQUIRE(a->N >= 1 && a->N <= BOSA_MAX_ROWS, "%s: N %lld outside [1, 2^21]", who, (long long)a->N);
  return 0;
}

extern "C" int mobody_bosa_stage2_rows(const MobodyBosaStage2* a, void* stream) {
  const char* who = "mobody_bosa_stage2_rows";
  int rc = stage2_check(who, a);
  if (rc) return rc;
  MB_REQUIRE(a->mask != nullptr || a->dll != nullptr, "%s: neither mask nor dll is given", who);
  MB_REQUIRE(a->mask == nullptr || a->row_weight != nullptr, "%s: row_weight is NULL", who);
  MB_REQUIRE(a->dll == nullptr || a->dpi != nullptr, "%s: dpi is NULL", who);
  MB_REQUIRE(a->dll == nullptr || (a->A >= 1 && a->A <= 128), "%s: A %d outside [1, 128]", who, a->A);
  MB_REQUIRE(a->dll == nullptr || a->dpi_scale == a->dpi_scale, "%s: dpi_scale is NaN", who);
  const long long n_mask = a->mask ? a->N : 0, n_dll = a->dll ? a->N * a->A : 0;
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_stage2_rows, dim3(row_grid(n_mask > n_dll ? n_mask : n_dll)), dim3(256), 0, st, a->mask, n_mask, a->row_weight, a->dll,
                     n_dll, a->dpi_scale, a->dpi);
  MB_LAUNCH_OK("k_bosa_stage2_rows");
  return 0;
}

extern "C" int mobody_bosa_stage2_words(const MobodyBosaStage2* a, void* stream) {
  const char* who = "mobody_bosa_stage2_words";
  int rc = stage2_check(who, a);
  if (rc) return rc;
  MB_REQUIRE(a->words != nullptr, "%s: words is NULL", who);
  MB_REQUIRE(a->closs != nullptr || a->ll != nullptr, "%s: neither closs nor ll is given", who);
  MB_REQUIRE(a->closs == nullptr || a->mask_mean != nullptr, "%s: mask_mean is NULL", who);
  MB_REQUIRE(a->ll == nullptr || a->aloss != nullptr, "%s: aloss is NULL", who);
  MB_REQUIRE(a->nbump >= 0 && a->nbump <= 4, "%s: nbump %d outside [0, 4]", who, a->nbump);
  MB_REQUIRE(a->nbump == 0 || a->bump != nullptr, "%s: bump is NULL", who);
  Stage2WordsArgs k{};
  k.mask_mean = a->mask_mean; k.closs = a->closs; k.ll = a->ll; k.aloss = a->aloss; k.N = a->N; k.cons_coef = a->cons_coef; k.lamda = a->lamda;
  k.words = a->words; k.bump = (long long*)a->bump; k.nbump = a->nbump;
  for (int i = 0; i < 4; ++i) k.bump_inc[i] = a->bump_inc[i];
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_stage2_words, dim3(1), dim3(256), 0, st, k);
  MB_LAUNCH_OK("k_bosa_stage2_words");
  return 0;
}
