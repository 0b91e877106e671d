// What the DARA translation units share (dara.hip, mlp_bwd.hip, train.hip): the classifier's double-softmax arithmetic -- ONE copy,
// used by the row-wise loss kernel and by seed mode 7 of the backward prologue -- and the launchers of the two row-wise kernels
// the fused classifier step and the relabel are built from.
#pragma once
#include <stdint.h>

#include "common.h"

namespace mobody {

__device__ __forceinline__ void softmax2(float z0, float z1, float& p0, float& p1) {
  const float m = fmaxf(z0, z1);
  const float e0 = expf(z0 - m), e1 = expf(z1 - m);
  const float inv = 1.f / (e0 + e1);
  p0 = e0 * inv; p1 = e1 * inv;
}

// loss = CE(softmax(z)) with CE's own log_softmax (double softmax); returns -log q[label] and dL/dz
__device__ __forceinline__ float ce_on_probs(float z0, float z1, int label, float scale, float& dz0, float& dz1) {
  float p0, p1, q0, q1;
  softmax2(z0, z1, p0, p1);                   // head output (torch.nn.Softmax, :25,31)
  softmax2(p0, p1, q0, q1);                   // F.cross_entropy's softmax over the probabilities (:169-170)
  const float g0 = q0 - (label == 0 ? 1.f : 0.f), g1 = q1 - (label == 1 ? 1.f : 0.f);      // dL/dp
  const float dot = g0 * p0 + g1 * p1;
  dz0 = scale * p0 * (g0 - dot);               // through the first softmax
  dz1 = scale * p1 * (g1 - dot);
  return -logf(label == 0 ? q0 : q1);
}

struct DaraInArgs {
  const float *s, *a, *s2;
  const float *noise_sas, *noise_sa;     // explicit unit normals [N][2S+A], [N][S+A] or null -> device generator
  long long N;
  int S, A;
  float std;
  uint32_t seed, call;
  float *x_sas, *x_sa;                   // [N][2S+A], [N][S+A]
};
// k_dara_inputs; call_dev != null: the generator's call id is (uint32_t)(call_dev[0] + call_offset) instead of a.call (a captured
// step reads the device call word)
int launch_dara_inputs(const DaraInArgs& a, const long long* call_dev, long long call_offset, hipStream_t st);
// k_dara_penalty on n rows of logits [n][2]
int launch_dara_penalty(const float* z_sas, const float* z_sa, long long n, float coef, float* reward, float* delta_out, hipStream_t st);

}  // namespace mobody
