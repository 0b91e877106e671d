// Host-side helpers shared by the C-ABI translation units.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string>

#include "../../include/mobody_hip.h"
#include "tile.h"

namespace mobody {

std::string& last_error();
int fail(int code, const char* fmt, ...);

#define MB_REQUIRE(cond, ...)                                   \
  do {                                                          \
    if (!(cond)) return ::mobody::fail(MOBODY_E_ARG, __VA_ARGS__); \
  } while (0)

#define MB_LAUNCH_OK(what)                                                                   \
  do {                                                                                       \
    hipError_t e_ = hipGetLastError();                                                       \
    if (e_ != hipSuccess) return ::mobody::fail(MOBODY_E_LAUNCH, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

// The head of every entry point that takes an argument block: the block is there and was built against this header.
#define MB_BLOCK(who, a, Block)                                                                                  \
  do {                                                                                                           \
    MB_REQUIRE((a) != nullptr, "%s: null argument struct", who);                                                 \
    MB_REQUIRE((a)->struct_bytes == (int32_t)sizeof(Block), "%s: struct_bytes %d != sizeof(" #Block ") %d", who, \
               (a)->struct_bytes, (int)sizeof(Block));                                                           \
  } while (0)

// Precision ids of the C ABI (MobodyHyper.precision and the `precision` arguments; names as _lib.PRECISIONS).  Host code
// compares against these; the kernels' template arguments PM / NPL carry the same numbers.
enum Precision { PREC_F32 = 0, PREC_BF16 = 1, PREC_BF16X2 = 2, PREC_BF16X3 = 3, PREC_F16X2 = 4 };
constexpr unsigned PREC_ALL = 0x1f, PREC_F32_OR_F16X2 = 1u << PREC_F32 | 1u << PREC_F16X2;   // `allowed` sets of check_precision

// The one range check of a precision argument: a known id, one of `allowed` (bit k = id k), and -- for every id but f32 --
// the 16-bit weight planes the split-precision kernels stream (T blobs / the ensemble's plane blob).
inline int check_precision(const char* who, int precision, bool have_planes, unsigned allowed = PREC_ALL) {
  static const char* const names[] = {"0 (f32)", "1 (bf16)", "2 (bf16x2)", "3 (bf16x3)", "4 (f16x2)"};
  if (precision < PREC_F32 || precision > PREC_F16X2 || !((allowed >> precision) & 1)) {
    std::string list;
    for (int k = PREC_F32; k <= PREC_F16X2; ++k)
      if ((allowed >> k) & 1) list += (list.empty() ? "" : ", ") + std::string(names[k]);
    return fail(MOBODY_E_ARG, "%s: precision %d: must be one of %s", who, precision, list.c_str());
  }
  MB_REQUIRE(precision == PREC_F32 || have_planes, "%s: the split-precision modes need the T blobs / plane blob (16-bit planes) of every net", who);
  return 0;
}

constexpr size_t TILE_LDS_BYTES = (size_t)BM * LDX * sizeof(float);   // 66,560 B: one activation image

// Opt a kernel into > 64 KiB of dynamic LDS once per process.
template <class K>
inline int allow_big_lds(K kernel, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) return fail(MOBODY_E_LAUNCH, "hipFuncSetAttribute: %s", hipGetErrorString(e));
  return 0;
}

// Optional per-kernel timing (bench.py): when enabled, the launch helpers bracket each launch of a kernel
// family with a HIP event pair on the launch stream.  Disabled (one branch) in normal operation.
enum ProfId { PROF_MLP_FWD = 0, PROF_MLP_BWD, PROF_WGRAD, PROF_DYN_FWD, PROF_DYN_TAIL, PROF_ROWWISE, PROF_OPTIM, PROF_REPLAY, PROF_COUNT };
struct ProfScope {
  int slot;
  hipStream_t st;
  ProfScope(int id, hipStream_t stream);
  ~ProfScope();
};


inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ring append (replay.hip): block scan (+ commit of the new {ptr, size} by the last block) and the row scatter
int launch_ring_append(const MobodyBufferView& ring, long long cap, long long* ptr_size, int S, int A, const float* obs,
                       const float* act, const float* next_obs, const float* reward, const uint8_t* terminal,
                       const uint8_t* keep, long long M, int32_t* scan_ws, hipStream_t st);
__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// hands a workspace out front to back, every piece rounded up to 4 floats; base == null: the sizes alone (no device is touched)
struct Carver {
  float* base;
  long long off = 0;
  float* operator()(long long n) { float* p = base ? base + off : nullptr; off += (n + 3) & ~3LL; return p; }
};

// return accounting of mobody_ens_evaluate (trajectory_return.hip): the caller's row state, which the step's tail launch
// updates in k_dyn_finalize's place (the step's obs / alive ARE obs_state / alive), and the two launches
struct DynEvalHook {
  float* obs_state;
  uint8_t* alive;
  float *ret, *pen_sum, *disc;
  int32_t* length;
  float discount;
};
int launch_eval_account(const float* r_mu, const float* penalty, const float* next_obs, const uint8_t* alive_next,
                        const DynEvalHook& h, long long B, int S, hipStream_t st);
int launch_eval_init(const float* init_obs, const DynEvalHook& h, long long B, int S, hipStream_t st);

// what mobody_ens_evaluate_policy adds to those launches: member[b] = elites[b % n_elites] (k_eval_members,
// trajectory_summary.hip; `elites` is the host array) and the Gaussian head's compaction dst [n][A] = columns [0, A) of
// src [n][pitch] (k_fqe_action, fqe.hip: the one copy of that kernel)
int launch_eval_members(const int32_t* elites, int n_elites, long long B, int32_t* member, hipStream_t st);
int launch_fqe_action(const float* src, int pitch, long long n, int A, float* dst, hipStream_t st);

// open-loop error accounting of mobody_ens_replay (trajectory_truth.hip): the caller's row state and the tables' rows of
// window step t, which the step's tail launch fills in k_dyn_finalize's place (the step's obs / act ARE obs_state /
// act_state), and the two launches
struct DynReplayHook {
  const MobodyBufferView* data;
  long long data_rows;
  const long long* row0;               // [B] device
  float *obs_state, *act_state;        // [B][S], [B][A]
  float *obs_err, *rew_err, *penalty;  // [B] each: row t of the [H][B] tables
  uint8_t* term_model;                 // [B]: row t
  int t, reset;                        // window step; obs_state <- the recorded next state after this step
};
int launch_replay_account(const float* r_mu, const float* penalty, const float* next_obs, const uint8_t* terminal,
                          const DynReplayHook& h, long long B, int S, int A, hipStream_t st);
int launch_replay_init(const DynReplayHook& h, long long B, int S, int A, hipStream_t st);

// device-side view of one packed MLP (member 0 pointers + strides), built from MobodyMlpLayout
struct MlpView {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int64_t member_floats;
  int Kp1, Np3, in_dim, out_dim;
};
inline MlpView mlp_view(const float* blob, const MobodyMlpLayout& L) {
  MlpView v;
  v.w1 = blob + L.w1; v.b1 = blob + L.b1; v.w2 = blob + L.w2; v.b2 = blob + L.b2; v.w3 = blob + L.w3; v.b3 = blob + L.b3;
  v.member_floats = L.member_floats; v.Kp1 = L.Kp1; v.Np3 = L.Np3; v.in_dim = L.in_dim; v.out_dim = L.out_dim;
  return v;
}

// Phase timeline of the fused MLP kernels (diagnostic builds only: MOBODY_TRACE=1 python build.py --force).
// TR(k) stores the 100 MHz wall clock of workgroup (blockIdx.y, blockIdx.x) at phase k; tools/trace_mlp.py reads it.
// (k_actor_bwd_chain runs two tiles in a continuing workgroup: the actor tile's stamps overwrite the dX tile's in its slots.)
#ifdef MOBODY_TRACE
constexpr int TRACE_BLOCKS = 16384, TRACE_SLOTS = 8;
extern __device__ unsigned long long g_trace[TRACE_BLOCKS * TRACE_SLOTS];
#define TR(k)                                                                                                     \
  do {                                                                                                            \
    if (threadIdx.x == 0)                                                                                         \
      g_trace[((size_t)(blockIdx.y * gridDim.x + blockIdx.x) % TRACE_BLOCKS) * TRACE_SLOTS + (k)] = wall_clock64(); \
  } while (0)
#else
#define TR(k)
#endif

}  // namespace mobody
