// Device health word: range faults of the f16x2 weight planes and non-finite optimizer results, seen on the device.
#pragma once
#include <math.h>

#include "common.h"
#include "tile_bf.h"

namespace mobody {

// ---- device health word (mobody_health_bind, include/mobody_hip.h) ----
// words[0] fault mask (MOBODY_HEALTH_*), words[1] Adam step count of the first faulting optimizer launch (for the host's
// message), words[2..3] ONE 64-bit key (tag << 32 | step) of that launch, published with a single compare-and-swap so that two
// launches faulting at once cannot mix their halves.  A lane that sees a violation publishes the key and then ORs its bit into
// the mask; nobody writes in the common case.  Every optimizer launch reads the mask on entry (one uniform load per wave) and applies
// nothing when a bit is set -- unless the key names the launch itself: the launch in which the fault happens runs to its end
// (its workgroups start at different times).  The tag is a host count of optimizer launches (constant in a captured graph,
// where the device step count tells the replays apart).
// LIMIT of the protocol: the decision is per wave at its start, so it is the same for a whole launch only if no OTHER
// optimizer launch raises a fault while this one runs.  Pre-training runs its nets' optimizer launches on two streams
// (pretrain.hip PreSide): a launch that overlaps the faulting one may be applied in part (every element it did apply is a
// complete, finite Adam step from healthy planes; p, m and v of one element always move together).  The mirror says so in its
// report.
int* health_words();                               // block bound on the current device, or null (core.hip)
int health_next_tag();
constexpr float F16_W_LIMIT = 65504.f / (float)(1 << F16_WSHIFT);      // first magnitude whose fp16 plane term overflows

__device__ __forceinline__ unsigned long long health_key(int tag, int step) {
  return ((unsigned long long)(unsigned)tag << 32) | (unsigned)step;
}
__device__ __forceinline__ void health_flag(int* words, int bits, int tag, int step) {
  if (tag != 0) {
    atomicCAS(reinterpret_cast<unsigned long long*>(words + 2), 0ULL, health_key(tag, step));
    atomicCAS(words + 1, 0, step);
    __threadfence();
  }
  atomicOr(words, bits);
}
// the plane builders' check: a value about to be written into a precision-4 plane
__device__ __forceinline__ void health_check_f16(int* words, float w) {
  if (words != nullptr && !(fabsf(w) < F16_W_LIMIT)) health_flag(words, MOBODY_HEALTH_F16_RANGE, 0, 0);
}

}  // namespace mobody
