// The termination predicates of the environments (terminal_funs.py), shared by the learned step (dynamics.hip) and the
// analytic task (task.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mobody_hip.h"

namespace mobody {

__device__ __forceinline__ bool term_predicate(int task, const float* n, int S) {
  // terminal_funs.py; comparisons with NaN are false exactly as in NumPy
  bool in_box = true, finite = true, lt100_from1 = true;
  for (int d = 0; d < S; ++d) {
    const float x = n[d];
    in_box = in_box && (x > -100.f) && (x < 100.f);
    finite = finite && isfinite(x);
    if (d >= 1) lt100_from1 = lt100_from1 && (x < 100.f);
  }
  switch (task) {
    case MOBODY_TERM_HALFCHEETAH: return !in_box;                                                   // :10-16
    case MOBODY_TERM_HOPPER: return !(finite && lt100_from1 && (n[0] > 0.7f) && (fabsf(n[1]) < 0.2f));   // :18-30
    case MOBODY_TERM_ANT: return !(finite && (n[0] >= 0.2f) && (n[0] <= 1.0f));                      // :39-61
    case MOBODY_TERM_WALKER2D:                                                                       // :63-75
      return !(in_box && (n[0] > 0.8f) && (n[0] < 2.0f) && (n[1] > -1.0f) && (n[1] < 1.0f));
    case MOBODY_TERM_HUMANOID: return (n[0] < 1.0f) || (n[0] > 2.0f);                                // :98-104
    case MOBODY_TERM_PEN: return n[26] < 0.075f;                                                     // :106-113
    default: return false;
  }
}

}  // namespace mobody
