// Device code of the minibatch gather shared by its two homes: the stand-alone gather kernels (replay.hip) and the
// gathering input stage of the fused MLP forward (layers.h fwd_gather_tile: the first forward launch of the train step
// draws and fetches its own rows).  Which ring row an output row is, how it is addressed and how it is loaded live here
// once, so the two forms cannot drift apart.
#pragma once
#include "common.h"
#include "rng.h"

namespace mobody {

__host__ __device__ inline bool view_packed(const MobodyBufferView& b, int S, int A) {
  return b.pitch > 0 && b.pitch % 16 == 0 && b.pitch >= 2LL * S + A + 2 && (reinterpret_cast<uintptr_t>(b.state) & 15) == 0 &&
         b.action == b.state + S && b.next_state == b.action + A && b.reward == b.next_state + S && b.not_done == b.reward + 1;
}

// Field pointers of row `row` of a view, either storage form (pitch 0: five contiguous arrays of their own widths).
__host__ __device__ inline const float* view_state(const MobodyBufferView& b, long long row, int S) { return b.state + row * (b.pitch ? b.pitch : S); }
__host__ __device__ inline const float* view_action(const MobodyBufferView& b, long long row, int A) { return b.action + row * (b.pitch ? b.pitch : A); }
__host__ __device__ inline const float* view_next_state(const MobodyBufferView& b, long long row, int S) { return b.next_state + row * (b.pitch ? b.pitch : S); }
__host__ __device__ inline const float* view_reward(const MobodyBufferView& b, long long row) { return b.reward + row * (b.pitch ? b.pitch : 1); }

struct GatherArgs {
  MobodyBufferView bufs[3];
  int packed[3];            // view_packed(bufs[k])
  const int32_t* idx[3];    // explicit row indices, or null -> drawn on the fly from the device generator
  long long start[4];       // row offsets of each source inside the output, start[nbuf] = N
  int nbuf, S, A, WS;       // WS = staged floats per row (2S+A+2 rounded up to 4)
  float *state, *action, *next_state, *reward, *not_done;
  // device-RNG mode (idx[k] == null): index i of source k = philox(seed[k], STREAM_SAMPLE, call)[i] * size >> 32,
  // call = (counter ? counter[0] : 0) + call_offset[k], size read from the device word size[k][0]
  uint32_t seed[3];
  long long call_offset[3];
  const long long* counter;
  const long long* size[3];
  long long* bump[4];       // device words incremented by one thread (never `counter`): graph replay advances its step counts here
  int nbump;
};

// e / n for 0 <= e < 2^16 and 1 <= n <= 2^16 through one multiply-high with ceil(2^32 / n) (exact in that range; a runtime
// integer division costs ~20 vector instructions per element of the staging loops)
__host__ __device__ inline uint32_t div_magic(int n) { return (uint32_t)((0x100000000ULL + (uint32_t)n - 1) / (uint32_t)n); }
__device__ __forceinline__ int fast_div(int e, uint32_t magic, int n) { return n == 1 ? e : (int)__umulhi((uint32_t)e, magic); }

// Source row of output row r (and which buffer it comes from): an explicit index, or one Philox draw.
__device__ __forceinline__ long long gather_src(const GatherArgs& a, long long r, int& k) {
  k = 0;
  if (a.nbuf > 1 && r >= a.start[1]) k = 1;
  if (a.nbuf > 2 && r >= a.start[2]) k = 2;
  if (a.idx[k] != nullptr) return a.idx[k][r - a.start[k]];
  const uint32_t call = (uint32_t)((a.counter ? a.counter[0] : 0) + a.call_offset[k]);
  const long long sz = a.size[k][0];
  return rng_index_at(a.seed[k], STREAM_SAMPLE, call, (uint64_t)(r - a.start[k]), (uint32_t)(sz > 0 ? sz : 1));
}

// A packed ring row as 16-byte chunks.  (Plain vector types and global-address-space pointers: with HIP's float4 struct and a
// pointer rebuilt from two shuffled words the compiler emitted flat loads and kept the rows in SCRATCH memory -- 131 us per
// million rows instead of 85.)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) v4f* gather_ptr_t;

// Row pointer `mine` of lane p of this thread's 16-lane group, handed over by shuffle (no LDS, no barrier).
__device__ __forceinline__ gather_ptr_t gather_group_row(const float* mine, int p) {
  const unsigned long long up = (unsigned long long)mine;
  const unsigned lo = (unsigned)__shfl((int)(unsigned)up, (threadIdx.x & 48) + p, 64), hi = (unsigned)__shfl((int)(unsigned)(up >> 32), (threadIdx.x & 48) + p, 64);
  return (gather_ptr_t)(((unsigned long long)hi << 32) | lo);
}

// replay.hip: fills the argument block of the device-RNG gather from the C ABI's arrays (range checks included; N = rows
// of the minibatch), and launches the stand-alone gather
int gather_args_rng(const char* who, GatherArgs& a, const MobodyBufferView* bufs, const int64_t* counts, int nbuf, int S, int A,
                    const uint32_t* seeds, const int64_t* call_offsets, const int64_t* counter, const int64_t* const* sizes,
                    float* state, float* action, float* next_state, float* reward, float* not_done, int64_t* const* bump,
                    int nbump, long long& N);
int launch_gather(const GatherArgs& a, long long N, hipStream_t st);

}  // namespace mobody
