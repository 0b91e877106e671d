// DARA domain-classifier pieces used inside MOBODY (algo/offline_offline/mobody.py:11-33 Classifier,
// :146-181 update_classifier, :354-381 one-off warm-up + reward penalty), plus the generic
// "gradients of one packed MLP from dz3 and saved activations" entry the classifier update is built from.
//
// Reference quirks reproduced: the heads output softmax PROBABILITIES, the loss applies
// cross_entropy (log_softmax) to those probabilities, and the penalty applies softmax to them once more.
// Row-wise kernels: HBM streaming over a few floats per row.
#include "common.h"
#include "dara.h"
#include "layers.h"
#include "rng.h"
#include "train.h"

namespace mobody {

constexpr uint32_t STREAM_CLS_SAS = 4, STREAM_CLS_SA = 5;

// classifier inputs with additive Gaussian noise  (Classifier.forward with_noise=True, mobody.py:19-31)
__device__ __forceinline__ void dara_inputs_body(const DaraInArgs& a) {
  const int W3 = 2 * a.S + a.A, W2 = a.S + a.A;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= a.N * W3) return;
  const long long row = gid / W3;
  const int c = (int)(gid - row * W3);
  const float v = c < a.S ? a.s[row * a.S + c] : (c < W2 ? a.a[row * a.A + (c - a.S)] : a.s2[row * a.S + (c - W2)]);
  float e = 0.f;
  if (a.std != 0.f) e = a.noise_sas ? a.noise_sas[gid] : rng_normal_at(a.seed, STREAM_CLS_SAS, a.call, (uint64_t)gid);
  a.x_sas[gid] = v + e * a.std;
  if (c < W2) {
    const long long g2 = row * W2 + c;
    float e2 = 0.f;
    if (a.std != 0.f) e2 = a.noise_sa ? a.noise_sa[g2] : rng_normal_at(a.seed, STREAM_CLS_SA, a.call, (uint64_t)g2);
    a.x_sa[g2] = v + e2 * a.std;
  }
}
__global__ __launch_bounds__(256) void k_dara_inputs(DaraInArgs a) { dara_inputs_body(a); }
// the same rows with the generator's call id read from a device word (a captured DARA step, dara.py:131-144)
__global__ __launch_bounds__(256) void k_dara_inputs_dev(DaraInArgs a, const long long* call_dev, long long call_offset) {
  a.call = (uint32_t)(call_dev[0] + call_offset);
  dara_inputs_body(a);
}

struct DaraLossArgs {
  const float *z_sas, *z_sa;        // logits [N][2]
  const int32_t* labels;            // [N] or null -> rows < n_src are label 0, the rest label 1
  long long N, n_src;
  int Np3;
  float *dz_sas, *dz_sa;            // [N][Np3]
  float* lossp;                     // [blocks][2] partial sums (sa, sas)
};

__device__ __forceinline__ float block_sum256(float v, float* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(256) void k_dara_loss(DaraLossArgs a) {
  __shared__ float sm[4];
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float l_sa = 0.f, l_sas = 0.f;
  if (row < a.N) {
    const int label = a.labels ? a.labels[row] : (row < a.n_src ? 0 : 1);
    const float scale = 1.f / (float)a.N;
    float d0, d1;
    l_sas = ce_on_probs(a.z_sas[2 * row], a.z_sas[2 * row + 1], label, scale, d0, d1);
    float* o = a.dz_sas + row * a.Np3;
    o[0] = d0; o[1] = d1;
    for (int k = 2; k < a.Np3; ++k) o[k] = 0.f;
    l_sa = ce_on_probs(a.z_sa[2 * row], a.z_sa[2 * row + 1], label, scale, d0, d1);
    o = a.dz_sa + row * a.Np3;
    o[0] = d0; o[1] = d1;
    for (int k = 2; k < a.Np3; ++k) o[k] = 0.f;
  }
  l_sa = block_sum256(l_sa, sm);
  l_sas = block_sum256(l_sas, sm);
  if (threadIdx.x == 0) { a.lossp[2 * blockIdx.x] = l_sa; a.lossp[2 * blockIdx.x + 1] = l_sas; }
}

__global__ __launch_bounds__(256) void k_dara_loss_final(const float* lossp, int nparts, long long N, float* loss_out) {
  __shared__ float sm[4];
  float s0 = 0.f, s1 = 0.f;
  for (int k = threadIdx.x; k < nparts; k += blockDim.x) { s0 += lossp[2 * k]; s1 += lossp[2 * k + 1]; }
  s0 = block_sum256(s0, sm);
  s1 = block_sum256(s1, sm);
  if (threadIdx.x == 0) { loss_out[0] = s0 / (float)N; loss_out[1] = s1 / (float)N; }     // (loss_sa, loss_sas)
}

// reward += coef * clamp(log p~_sas[1] - log p~_sa[1] - log p~_sas[0] + log p~_sa[0], -10, 10),
// p~ = softmax(head probabilities) + 1e-10                                      (mobody.py:373-379)
__global__ __launch_bounds__(256) void k_dara_penalty(const float* z_sas, const float* z_sa, long long n, float coef,
                                                      float* reward, float* delta_out) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  float p0, p1, s0, s1, t0, t1, u0, u1;
  softmax2(z_sas[2 * row], z_sas[2 * row + 1], p0, p1);
  softmax2(p0, p1, s0, s1);
  softmax2(z_sa[2 * row], z_sa[2 * row + 1], t0, t1);
  softmax2(t0, t1, u0, u1);
  float d = logf(s1 + 1e-10f) - logf(u1 + 1e-10f) - logf(s0 + 1e-10f) + logf(u0 + 1e-10f);
  d = fminf(fmaxf(d, -10.f), 10.f);
  if (delta_out) delta_out[row] = d;
  if (reward) reward[row] += coef * d;
}

int launch_dara_inputs(const DaraInArgs& a, const long long* call_dev, long long call_offset, hipStream_t st) {
  if (a.N <= 0) return 0;
  const dim3 grid((unsigned)cdiv(a.N * (2 * a.S + a.A), 256));
  if (call_dev != nullptr) hipLaunchKernelGGL(k_dara_inputs_dev, grid, dim3(256), 0, st, a, call_dev, call_offset);
  else hipLaunchKernelGGL(k_dara_inputs, grid, dim3(256), 0, st, a);
  MB_LAUNCH_OK("k_dara_inputs");
  return 0;
}

int launch_dara_penalty(const float* z_sas, const float* z_sa, long long n, float coef, float* reward, float* delta_out, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dara_penalty, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, z_sas, z_sa, n, coef, reward, delta_out);
  MB_LAUNCH_OK("k_dara_penalty");
  return 0;
}

// ---- generic MLP gradient (dz3 + saved activations -> gradient blob) ----
// its scratch: the backward half of a net's record (the caller owns x, h1, h2)
static NetScratch carve_bwd(const MobodyMlpLayout& L, long long rows, float* base, long long& total) {
  Carver take{base};
  const NetScratch s = carve_net(L, rows, false, L.Np3, take);
  total = take.off;
  return s;
}

}  // namespace mobody
using namespace mobody;

extern "C" int64_t mobody_mlp3_backward_workspace(int in_dim, int out_dim, int members, int64_t rows) {
  MobodyMlpLayout L;
  if (mobody_mlp_layout(in_dim, out_dim, members, &L) || rows < 1) return -1;
  long long total = 0;
  carve_bwd(L, rows, nullptr, total);
  return total;
}

extern "C" int mobody_mlp3_backward(const float* blob_T, int in_dim, int out_dim, int members, const float* dz3,
                                    const float* x, const float* h1, const float* h2, int64_t rows, float* grad,
                                    float* workspace, void* stream) {
  MobodyMlpLayout L;
  int rc = mobody_mlp_layout(in_dim, out_dim, members, &L);
  if (rc) return rc;
  MB_REQUIRE(rows >= 1, "mobody_mlp3_backward: rows < 1");
  MB_REQUIRE(blob_T && dz3 && x && h1 && h2 && grad && workspace, "mobody_mlp3_backward: null pointer");
  long long total = 0;
  const NetScratch w = carve_bwd(L, rows, workspace, total);
  hipStream_t st = as_stream(stream);
  Mlp3BwdArgs b = bwd_net(L, blob_T, rows);       // exact fp32 on the saved activations: no planes, no sign words
  bwd_set_acts(b, h1, h2, nullptr, nullptr, 0);
  bwd_set_grads(b, dz3, w.dz2, w.dz1, w.dbp);
  rc = launch_mlp3_bwd(b, members, false, st);
  if (rc) return rc;
  Mlp3WgradArgs g = wgrad_net(L, rows, w.nsplit);
  wgrad_set_saves(g, x, 0, h1, h2);               // the members share the input rows
  wgrad_set_grads(g, dz3, w.dz2, w.dz1, w.dbp, w.ntiles);
  wgrad_set_scratch(g, w.slabs, nullptr);
  wgrad_set_result(g, grad, LossFinal{}, AdamTarget{}, PREC_F32);
  return mlp3_weight_grads(g, st);
}

extern "C" int mobody_dara_inputs(const float* s, const float* a, const float* s2, int64_t N, int S, int A, float std,
                                  const float* noise_sas, const float* noise_sa, uint32_t seed, uint32_t call,
                                  float* x_sas, float* x_sa, void* stream) {
  MB_REQUIRE(N >= 0 && S >= 1 && A >= 1, "mobody_dara_inputs: bad sizes");
  if (N == 0) return 0;
  MB_REQUIRE(s && a && s2 && x_sas && x_sa, "mobody_dara_inputs: null pointer");
  DaraInArgs d{s, a, s2, noise_sas, noise_sa, N, S, A, std, seed, call, x_sas, x_sa};
  return launch_dara_inputs(d, nullptr, 0, as_stream(stream));
}

extern "C" int mobody_dara_loss_grad(const float* z_sas, const float* z_sa, const int32_t* labels, int64_t N,
                                     int64_t n_src, float* dz_sas, float* dz_sa, float* loss_out, float* lossp_ws,
                                     void* stream) {
  MB_REQUIRE(N >= 1, "mobody_dara_loss_grad: N < 1");
  MB_REQUIRE(z_sas && z_sa && dz_sas && dz_sa && loss_out && lossp_ws, "mobody_dara_loss_grad: null pointer");
  MobodyMlpLayout L;
  mobody_mlp_layout(1, 2, 1, &L);
  const int nb = (int)cdiv(N, 256);
  DaraLossArgs d{z_sas, z_sa, labels, N, n_src, L.Np3, dz_sas, dz_sa, lossp_ws};
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_dara_loss, dim3(nb), dim3(256), 0, st, d);
  MB_LAUNCH_OK("k_dara_loss");
  hipLaunchKernelGGL(k_dara_loss_final, dim3(1), dim3(256), 0, st, lossp_ws, nb, (long long)N, loss_out);
  MB_LAUNCH_OK("k_dara_loss_final");
  return 0;
}

extern "C" int mobody_dara_penalty(const float* z_sas, const float* z_sa, int64_t n, float coef, float* reward,
                                   float* delta_out, void* stream) {
  MB_REQUIRE(n >= 0, "mobody_dara_penalty: n < 0");
  if (n == 0) return 0;
  MB_REQUIRE(z_sas && z_sa && (reward || delta_out), "mobody_dara_penalty: null pointer");
  return launch_dara_penalty(z_sas, z_sa, n, coef, reward, delta_out, as_stream(stream));
}
