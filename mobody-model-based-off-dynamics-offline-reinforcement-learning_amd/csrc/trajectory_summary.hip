// What mobody_ens_evaluate_policy adds to the evaluation's row state: the member every episode keeps for its whole
// length, and the figures of the finished row state by member group.  The reference has no counterpart.
//
//   k_eval_members   member[b] = elites[b % n_elites]: the row state of member_mode 1, resume == 0
//   k_eval_summary   (mean return, mean length, mean penalty sum, alive share) per group b % G and over all rows, the NaN flag
//
// A translation unit of its own, linked after fqe.hip: every code object of the existing kernels stays byte for byte what it was
// (tools/isa_diff.py).  No flags, tickets or atomics; every loop is bounded by an argument; every sum runs in a fixed order.
#include "common.h"

namespace mobody {

struct EliteList { int32_t id[NENS]; int32_t n; };

__global__ __launch_bounds__(256) void k_eval_members(EliteList e, long long B, int32_t* member) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int g = (int)(b % e.n);
  int32_t pick = e.id[0];
#pragma unroll
  for (int k = 1; k < NENS; ++k) pick = g == k ? e.id[k] : pick;       // a select chain: the by-value list stays in registers
  member[b] = pick;
}

constexpr int SUMMARY_SLOTS = NENS + 1;       // up to 7 groups and the slot of all rows

// out[G + 1][4], nan_flag[1].  One workgroup: thread t takes rows t, t + 256, ... in ascending order and adds each row into the
// accumulators of its group b % G and into those of all rows (two accumulator sets, each fed in row order); then, slot by slot, a
// fixed tree joins the 256 partial results (k_fqe_value's scheme).  Returns and penalty sums are fp32 sums, lengths and alive
// counts 64-bit integer sums (exact); a group's row count is the closed form of B and G.  A mean is one division by the count; the
// two integer means are divided in fp64 and rounded to fp32 once.  A group without rows (B <= g) gets four NaNs.
__global__ __launch_bounds__(256) void k_eval_summary(const float* ret, const float* pen_sum, const int32_t* length,
                                                      const uint8_t* alive, long long B, int G, float* out, int* nan_flag) {
  __shared__ float r_ret[256], r_pen[256];
  __shared__ long long r_len[256], r_alive[256];
  __shared__ int r_bad[256];
  const int t = threadIdx.x;
  float s_ret[SUMMARY_SLOTS], s_pen[SUMMARY_SLOTS];
  long long s_len[SUMMARY_SLOTS], s_alive[SUMMARY_SLOTS];
#pragma unroll
  for (int k = 0; k < SUMMARY_SLOTS; ++k) { s_ret[k] = 0.f; s_pen[k] = 0.f; s_len[k] = 0; s_alive[k] = 0; }
  int bad = 0;
  for (long long b = t; b < B; b += 256) {
    const float r = ret[b], p = pen_sum[b];
    const long long len = length[b], al = alive[b] != 0 ? 1 : 0;
    const int g = (int)(b % G);
    bad |= (r != r) | (p != p);
#pragma unroll
    for (int k = 0; k < NENS; ++k)             // static indices: the accumulators stay in registers
      if (g == k) { s_ret[k] += r; s_pen[k] += p; s_len[k] += len; s_alive[k] += al; }
    s_ret[NENS] += r; s_pen[NENS] += p; s_len[NENS] += len; s_alive[NENS] += al;
  }
  r_bad[t] = bad;
#pragma unroll
  for (int k = 0; k < SUMMARY_SLOTS; ++k) {
    if (k < NENS && k >= G) continue;          // uniform: G is an argument
    __syncthreads();                           // the previous slot's result has been read
    r_ret[t] = s_ret[k]; r_pen[t] = s_pen[k]; r_len[t] = s_len[k]; r_alive[t] = s_alive[k];
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (t < h) {
        r_ret[t] += r_ret[t + h]; r_pen[t] += r_pen[t + h]; r_len[t] += r_len[t + h]; r_alive[t] += r_alive[t + h];
        if (k == NENS) r_bad[t] |= r_bad[t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      const int row = k == NENS ? G : k;
      const long long count = k == NENS ? B : (B > k ? (B - k - 1) / G + 1 : 0);
      float* o = out + 4 * row;
      if (count == 0) {
        o[0] = o[1] = o[2] = o[3] = __builtin_nanf("");
      } else {
        o[0] = r_ret[0] / (float)count;
        o[1] = (float)((double)r_len[0] / (double)count);
        o[2] = r_pen[0] / (float)count;
        o[3] = (float)((double)r_alive[0] / (double)count);
      }
      if (k == NENS) nan_flag[0] = r_bad[0];
    }
  }
}

int launch_eval_members(const int32_t* elites, int n_elites, long long B, int32_t* member, hipStream_t st) {
  EliteList e{};
  for (int k = 0; k < NENS; ++k) e.id[k] = k < n_elites ? elites[k] : 0;
  e.n = n_elites;
  hipLaunchKernelGGL(k_eval_members, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, e, B, member);
  MB_LAUNCH_OK("k_eval_members");
  return 0;
}

}  // namespace mobody

using namespace mobody;

extern "C" int mobody_eval_summary(const float* ret, const float* pen_sum, const int32_t* length, const uint8_t* alive, int64_t B, int G,
                                   float* out, int32_t* nan_flag, void* stream) {
  const char* who = "mobody_eval_summary";
  MB_REQUIRE(G >= 1 && G <= NENS, "%s: G %d outside 1..7", who, G);
  MB_REQUIRE(B >= 1, "%s: B %lld < 1", who, (long long)B);
  MB_REQUIRE(ret != nullptr, "%s: null pointer ret", who);
  MB_REQUIRE(pen_sum != nullptr, "%s: null pointer pen_sum", who);
  MB_REQUIRE(length != nullptr, "%s: null pointer length", who);
  MB_REQUIRE(alive != nullptr, "%s: null pointer alive", who);
  MB_REQUIRE(out != nullptr, "%s: null pointer out", who);
  MB_REQUIRE(nan_flag != nullptr, "%s: null pointer nan_flag", who);
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_eval_summary, dim3(1), dim3(256), 0, st, ret, pen_sum, length, alive, (long long)B, G, out, (int*)nan_flag);
  MB_LAUNCH_OK("k_eval_summary");
  return 0;
}
