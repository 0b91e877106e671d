// What the IGDF translation units share (igdf.hip, train.hip): the launchers of the row-wise kernels the contrastive update and
// the per-step filter are built from (the reference's algo/offline_offline/igdf.py).
#pragma once
#include <stdint.h>

#include "common.h"

namespace mobody {

constexpr int IGDF_MAX_N = 4096, IGDF_MAX_Z = 128, IGDF_TILE = 32;

// k_igdf_contrast (igdf.py:427-440): loss partials lossp[ceil(n / 32)], dz3_sa [n][Np3], dz3_ss [2n-1][Np3]
int launch_igdf_contrast(const float* phi, const float* psi_tar, const float* psi_src, long long n, int Z, int ldz, int Np3,
                         float* dz3_sa, float* dz3_ss, float* lossp, hipStream_t st);
// loss_out[0] = scale * sum lossp[0 .. nparts)
int launch_igdf_sum(const float* parts, int nparts, float scale, float* out, hipStream_t st);
// k_igdf_score (igdf.py:500-504): score[i] = phi_i . psi_i / (|phi_i| |psi_i|) over Z columns
int launch_igdf_score(const float* phi, const float* psi, long long n, int Z, int ldz, float* score, hipStream_t st);

// what k_igdf_select writes besides kept / w when it also compacts the staged batch (all null: the selection alone)
struct IgdfBatch {
  const float *s, *a, *s2, *r, *nd;          // staged rows [src(n) | tar(n_tar)]
  float *os, *oa, *os2, *orw, *ond, *w;       // [k + n_tar] rows: [kept src | tar]; w: row weights
  long long n_tar;
  int S, A;
};
// k_igdf_select (igdf.py:505-524); kept / w_sel may be null when `b` carries the outputs
int launch_igdf_select(const float* score, long long n, long long k, float iw, int32_t* kept, float* w_sel, const IgdfBatch& b,
                       hipStream_t st);

}  // namespace mobody
