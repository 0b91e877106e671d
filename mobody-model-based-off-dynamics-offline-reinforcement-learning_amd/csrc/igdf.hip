// IGDF's row-wise kernels (the reference's algo/offline_offline/igdf.py): the in-batch contrastive loss and its
// gradient with respect to the two encoders' outputs (update_info, :427-440), the per-row score of the data filter (:500-504) and
// the top-k selection with the compaction of the training batch (:505-524).  No float atomics: every sum runs in a fixed order.
#include <math.h>

#include "common.h"
#include "igdf.h"

namespace mobody {

constexpr int CT = IGDF_TILE;             // 32 x 32 logits per step of a workgroup
constexpr int CLD = IGDF_MAX_Z + 1;       // LDS row pitch of a 32-row tile of representations (odd: no bank conflicts)

__device__ __forceinline__ float sigmoidf_stable(float l) {
  if (l >= 0.f) return 1.f / (1.f + expf(-l));
  const float e = expf(l);
  return e / (1.f + e);
}
// binary_cross_entropy_with_logits against target 0: max(l, 0) + log1p(exp(-|l|))
__device__ __forceinline__ float softplusf_stable(float l) { return fmaxf(l, 0.f) + log1pf(expf(-fabsf(l))); }

struct ContrastArgs {
  const float *phi, *psi_tar, *psi_src;   // [n][ldz], [n][ldz], [n-1][ldz]
  long long n;
  int Z, ldz, Np3;
  float *dz3_sa, *dz3_ss, *lossp;         // [n][Np3], [2n-1][Np3], [ceil(n / 32)]
};

// Workgroups [0, ceil(n / 32)) own 32 rows of phi each: they form their rows of the logits against every column, the loss partial
// and dL/dphi, and -- column 0, the row's own target next state -- dL/dpsi_tar.  The workgroups behind them own 32 source next
// states each and form dL/dpsi_src, a sum over all n rows, from the same logits formed once more: the n x n matrix is computed
// twice and never stored, and no sum is split between workgroups.  Thread (ti, tj) = (t / 8, t % 8): logits (ti, tj + 8 c), gradient
// columns tj + 8 m of owner row ti.
__global__ __launch_bounds__(256) void k_igdf_contrast(ContrastArgs a) {
  __shared__ float As[CT * CLD], Bs[CT * CLD], Gs[CT * (CT + 1)], red[4];
  const int t = threadIdx.x, ti = t >> 3, tj = t & 7;
  const long long n = a.n;
  const int Z = a.Z, ldz = a.ldz, Np3 = a.Np3;
  const int nrt = (int)cdiv(n, CT);
  const bool rowrole = (int)blockIdx.x < nrt;
  const int tile = rowrole ? (int)blockIdx.x : (int)blockIdx.x - nrt;
  const long long nA = rowrole ? n : n - 1, nB = rowrole ? n - 1 : n;
  const float* A = rowrole ? a.phi : a.psi_src;
  const float* B = rowrole ? a.psi_src : a.phi;
  const long long a0 = (long long)tile * CT;
  const int arows = (int)min((long long)CT, nA - a0);
  const float inv = 1.f / ((float)n * (float)n);
  for (int e = t; e < CT * Z; e += 256) {
    const int r = e / Z, z = e - r * Z;
    As[r * CLD + z] = r < arows ? A[(a0 + r) * ldz + z] : 0.f;
  }
  const bool ok = ti < arows;
  const long long arow = a0 + (ok ? ti : 0);
  float acc[IGDF_MAX_Z / 8];
#pragma unroll
  for (int m = 0; m < IGDF_MAX_Z / 8; ++m) acc[m] = 0.f;
  float loss = 0.f;
  __syncthreads();
  if (rowrole) {                                     // column 0: target 1 (:436-437)
    const float* pt = a.psi_tar + arow * ldz;
    float l0 = 0.f;
    for (int z = 0; z < Z; ++z) l0 += As[ti * CLD + z] * pt[z];
    const float g0 = ok ? -sigmoidf_stable(-l0) * inv : 0.f;          // (sigma(l) - 1) / n^2 without the cancellation
    if (ok && tj == 0) loss += softplusf_stable(-l0);               // max(l, 0) - l + log1p(exp(-|l|))
#pragma unroll
    for (int m = 0; m < IGDF_MAX_Z / 8; ++m) {
      const int z = tj + 8 * m;
      if (z < Z) acc[m] = g0 * pt[z];
      if (ok && z < Np3) a.dz3_ss[arow * Np3 + z] = z < Z ? g0 * As[ti * CLD + z] : 0.f;      // dL/dpsi_tar
    }
  }
  for (long long b0 = 0; b0 < nB; b0 += CT) {
    __syncthreads();                                 // the previous tile's Bs / Gs have been read
    const int brows = (int)min((long long)CT, nB - b0);
    for (int e = t; e < CT * Z; e += 256) {
      const int r = e / Z, z = e - r * Z;
      Bs[r * CLD + z] = r < brows ? B[(b0 + r) * ldz + z] : 0.f;
    }
    __syncthreads();
    float l[4] = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < Z; ++z) {
      const float av = As[ti * CLD + z];
#pragma unroll
      for (int c = 0; c < 4; ++c) l[c] += av * Bs[(tj + 8 * c) * CLD + z];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool valid = ok && tj + 8 * c < brows;
      Gs[ti * (CT + 1) + tj + 8 * c] = valid ? sigmoidf_stable(l[c]) * inv : 0.f;            // target 0
      if (rowrole && valid) loss += softplusf_stable(l[c]);
    }
    __syncthreads();
    for (int cc = 0; cc < CT; ++cc) {
      const float g = Gs[ti * (CT + 1) + cc];
#pragma unroll
      for (int m = 0; m < IGDF_MAX_Z / 8; ++m)
        if (tj + 8 * m < Z) acc[m] += g * Bs[cc * CLD + tj + 8 * m];
    }
  }
  if (ok) {
    float* dst = rowrole ? a.dz3_sa + arow * Np3 : a.dz3_ss + (n + arow) * Np3;
#pragma unroll
    for (int m = 0; m < IGDF_MAX_Z / 8; ++m) {
      const int z = tj + 8 * m;
      if (z < Np3) dst[z] = z < Z ? acc[m] : 0.f;
    }
  }
  if (rowrole) {                                     // loss partial of these 32 rows, fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o);
    if ((t & 63) == 0) red[t >> 6] = loss;
    __syncthreads();
    if (t == 0) a.lossp[tile] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

__global__ __launch_bounds__(256) void k_igdf_sum(const float* parts, int n, float scale, float* out) {
  __shared__ float red[4];
  float s = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) s += parts[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + (red[2] + red[3])) * scale;
}

// score_i = phi_i . psi_i / (|phi_i| |psi_i|), no epsilon (:500-504); eight lanes per row
__global__ __launch_bounds__(256) void k_igdf_score(const float* phi, const float* psi, long long n, int Z, int ldz, float* score) {
  const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int sub = threadIdx.x & 7;
  const long long rc = row < n ? row : 0;
  float d = 0.f, pa = 0.f, pb = 0.f;
  for (int z = sub; z < Z; z += 8) {
    const float x = phi[rc * ldz + z], y = psi[rc * ldz + z];
    d += x * y; pa += x * x; pb += y * y;
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) { d += __shfl_xor(d, o); pa += __shfl_xor(pa, o); pb += __shfl_xor(pb, o); }
  if (row < n && sub == 0) score[row] = d / (sqrtf(pa) * sqrtf(pb));
}

// The total order of the selection: an integer key of the float that grows with it (-0 below +0); every non-finite score gets
// key 0, below the most negative finite one (key 0x00800000).  Ties go to the lower index.
__device__ __forceinline__ uint32_t igdf_key(float s) {
  const uint32_t u = __float_as_uint(s);
  if ((u & 0x7f800000u) == 0x7f800000u) return 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Rank by counting (n <= 4096 keys in LDS): row i's ascending rank is the number of rows below it in the total order, so the ranks
// are a permutation whatever the bits.  Rows of rank >= n - k are kept at position rank - (n - k).  A workgroup ranks SEL_ROWS rows,
// sixteen lanes to a row, each counting every sixteenth key (integer partial counts, summed by shuffles): n / 16 workgroups, so
// that 4096 rows fill the device instead of sixteen CUs.  With a batch to compact, the workgroup then copies its kept rows, and
// the target rows of its index range, into the training batch.
constexpr int SEL_ROWS = 16, SEL_SPLIT = 256 / SEL_ROWS;
__global__ __launch_bounds__(256) void k_igdf_select(const float* score, int n, int k, float iw, int32_t* kept, float* w_sel, IgdfBatch b) {
  __shared__ uint32_t keys[IGDF_MAX_N];
  __shared__ int spos[SEL_ROWS];
  const int t = threadIdx.x;
  for (int e = t; e < n; e += 256) keys[e] = igdf_key(score[e]);
  __syncthreads();
  const int rl = t / SEL_SPLIT, sub = t % SEL_SPLIT;
  const int i = (int)blockIdx.x * SEL_ROWS + rl;
  int pos = -1;
  {
    const int ic = i < n ? i : 0;
    const uint32_t ki = keys[ic];
    int rank = 0;
    for (int j = sub; j < n; j += SEL_SPLIT) {
      const uint32_t kj = keys[j];
      rank += (kj < ki || (kj == ki && j < ic)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < SEL_SPLIT; o <<= 1) rank += __shfl_xor(rank, o);
    if (i < n) pos = rank - (n - k);
    if (pos >= 0 && sub == 0) {
      const float wv = expf(iw * score[i]);
      if (kept != nullptr) kept[pos] = i;
      if (w_sel != nullptr) w_sel[pos] = wv;
      if (b.w != nullptr) b.w[pos] = wv;
    }
  }
  if (b.os == nullptr) return;
  if (sub == 0) spos[rl] = pos;
  __syncthreads();
  const int S = b.S, A = b.A, W = 2 * S + A + 2;
  const long long r0 = (long long)blockIdx.x * SEL_ROWS;
  for (int e = t; e < SEL_ROWS * W; e += 256) {
    const int r = e / W, c = e - r * W;
    for (int pass = 0; pass < 2; ++pass) {           // pass 0: a kept source row; pass 1: the target row of the same index
      long long src, dst;
      if (pass == 0) {
        if (spos[r] < 0) continue;
        src = r0 + r; dst = spos[r];
      } else {
        if (r0 + r >= b.n_tar) continue;
        src = n + r0 + r; dst = k + r0 + r;
      }
      if (c < S) b.os[dst * S + c] = b.s[src * S + c];
      else if (c < S + A) b.oa[dst * A + (c - S)] = b.a[src * A + (c - S)];
      else if (c < 2 * S + A) b.os2[dst * S + (c - S - A)] = b.s2[src * S + (c - S - A)];
      else if (c == 2 * S + A) b.orw[dst] = b.r[src];
      else { b.ond[dst] = b.nd[src]; if (pass == 1 && b.w != nullptr) b.w[dst] = 1.f; }
    }
  }
}

int launch_igdf_contrast(const float* phi, const float* psi_tar, const float* psi_src, long long n, int Z, int ldz, int Np3,
                         float* dz3_sa, float* dz3_ss, float* lossp, hipStream_t st) {
  ContrastArgs a{phi, psi_tar, psi_src, n, Z, ldz, Np3, dz3_sa, dz3_ss, lossp};
  ProfScope prof(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_igdf_contrast, dim3((unsigned)(cdiv(n, CT) + cdiv(n - 1, CT))), dim3(256), 0, st, a);
  MB_LAUNCH_OK("k_igdf_contrast");
  return 0;
}

int launch_igdf_sum(const float* parts, int nparts, float scale, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_igdf_sum, dim3(1), dim3(256), 0, st, parts, nparts, scale, out);
  MB_LAUNCH_OK("k_igdf_sum");
  return 0;
}

int launch_igdf_score(const float* phi, const float* psi, long long n, int Z, int ldz, float* score, hipStream_t st) {
  ProfScope prof(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_igdf_score, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, st, phi, psi, n, Z, ldz, score);
  MB_LAUNCH_OK("k_igdf_score");
  return 0;
}

int launch_igdf_select(const float* score, long long n, long long k, float iw, int32_t* kept, float* w_sel, const IgdfBatch& b,
                       hipStream_t st) {
  const long long rows = b.os != nullptr && b.n_tar > n ? b.n_tar : n;
  ProfScope prof(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_igdf_select, dim3((unsigned)cdiv(rows, SEL_ROWS)), dim3(256), 0, st, score, (int)n, (int)k, iw, kept, w_sel, b);
  MB_LAUNCH_OK("k_igdf_select");
  return 0;
}

}  // namespace mobody

using namespace mobody;

static int igdf_check_nz(const char* who, long long n, int Z) {
  MB_REQUIRE(n >= 2 && n <= IGDF_MAX_N, "%s: n %lld outside [2, %d]", who, n, IGDF_MAX_N);
  MB_REQUIRE(Z >= 1 && Z <= IGDF_MAX_Z, "%s: Z %d outside [1, %d]", who, Z, IGDF_MAX_Z);
  return 0;
}

// igdf.py:427-440 (the logits, the target matrix, binary_cross_entropy_with_logits and its backward to the representations)
extern "C" int mobody_igdf_contrast(const float* phi, const float* psi_tar, const float* psi_src, int64_t n, int32_t Z, int32_t ldz,
                                    float* dz3_sa, float* dz3_ss, float* lossp, float* loss_out, void* stream) {
  const char* who = "mobody_igdf_contrast";
  int rc = igdf_check_nz(who, n, Z);
  if (rc) return rc;
  MB_REQUIRE(ldz >= Z, "%s: ldz %d < Z %d", who, ldz, Z);
  MB_REQUIRE(phi && psi_tar && psi_src && dz3_sa && dz3_ss && lossp && loss_out, "%s: null pointer", who);
  const int Np3 = (Z + 15) & ~15;
  hipStream_t st = as_stream(stream);
  rc = launch_igdf_contrast(phi, psi_tar, psi_src, n, Z, ldz, Np3, dz3_sa, dz3_ss, lossp, st);
  if (rc) return rc;
  return launch_igdf_sum(lossp, (int)cdiv(n, IGDF_TILE), 1.f / ((float)n * (float)n), loss_out, st);
}

// igdf.py:505-508, :515 (argsort, the last k, exp(importance_weight * score))
extern "C" int mobody_igdf_select(const float* score, int64_t n, int64_t k, float importance_weight, int32_t* kept, float* w, void* stream) {
  const char* who = "mobody_igdf_select";
  MB_REQUIRE(n >= 1 && n <= IGDF_MAX_N, "%s: n %lld outside [1, %d]", who, (long long)n, IGDF_MAX_N);
  MB_REQUIRE(k >= 1 && k <= n, "%s: k %lld outside [1, n = %lld]", who, (long long)k, (long long)n);
  MB_REQUIRE(score && kept && w, "%s: null pointer", who);
  return launch_igdf_select(score, n, k, importance_weight, kept, w, IgdfBatch{}, as_stream(stream));
}
