// Packed 3-layer MLPs whose hidden width is a parameter (BOSA's 750-wide VAE nets): layout, forward, backward and
// Adam.  Every matrix product -- X W, dZ W^T, X^T dZ -- is one launch of k_wide_gemm on v_mfma_f32_32x32x2_f32 (exact fp32, a
// k-ordered fma chain per output element) with the bias / ReLU / tanh / ReLU-mask epilogue folded in.  A workgroup owns a
// 64 x 64 output tile over the WHOLE contraction, so the weight gradient sums over batch rows in a fixed order: no split-K,
// no float atomics, the same bits on every run.  fp32 only: the split-precision planes of tile_bf.h are built around HID = 256.
#include <math.h>

#include "common.h"
#include "train.h"

namespace mobody {

constexpr int WBM = 64, WBN = 64, WBK = 16;   // output tile of a workgroup (4 waves, one 32 x 32 accumulator each), K chunk
constexpr int WLD = WBM + 1;                  // LDS row pitch of the [k][m] / [k][n] images (odd: conflict-free transposing stores)

enum WideEpi { WEPI_STORE = 0, WEPI_BIAS = 1, WEPI_BIAS_RELU = 2, WEPI_BIAS_TANH = 3, WEPI_RELU_MASK = 4 };

// C[e](m, n) = epi(sum_k A[e](m, k) B[e](k, n)), element (i, j) of an operand at base + e * s_e + i * s_i + j * s_j.
// Reads outside [0, MA) x [0, K) of A and [0, K) x [0, NB) of B give 0; (m, n) is stored for m < M, n < N.
struct WideGemm {
  const float *A, *B;
  float* C;
  long long sAe, sAm, sAk, sBe, sBk, sBn, sCe, ldc;
  int M, N, K, MA, NB;
  int epi;
  const float* bias;       // [e][sbe + n]                 (WEPI_BIAS*)
  long long sbe;
  const float* mask;       // [e][m * ldmask + n] > 0      (WEPI_RELU_MASK: the saved post-ReLU activation)
  long long sme, ldmask;
  float max_action;        // WEPI_BIAS_TANH
};

__device__ __forceinline__ void wide_stage(const float* P, long long s_i, long long s_k, int i0, int k0, int I, int K, float* img, int t) {
  // 64 x 16 elements, 4 per thread; consecutive threads walk the operand's unit-stride index
  const bool kfast = s_k == 1;
#pragma unroll
  for (int q = 0; q < (WBM * WBK) / 256; ++q) {
    const int idx = t + 256 * q;
    const int i = kfast ? idx / WBK : idx % WBM, k = kfast ? idx % WBK : idx / WBM;
    const int gi = i0 + i, gk = k0 + k;
    img[k * WLD + i] = (gi < I && gk < K) ? P[(long long)gi * s_i + (long long)gk * s_k] : 0.f;
  }
}

__global__ __launch_bounds__(256) void k_wide_gemm(WideGemm g) {
  __shared__ float As[WBK * WLD], Bs[WBK * WLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int e = blockIdx.z, m0 = blockIdx.y * WBM, n0 = blockIdx.x * WBN;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const float* A = g.A + (long long)e * g.sAe;
  const float* B = g.B + (long long)e * g.sBe;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < g.K; k0 += WBK) {
    wide_stage(A, g.sAm, g.sAk, m0, k0, g.MA, g.K, As, t);
    wide_stage(B, g.sBn, g.sBk, n0, k0, g.NB, g.K, Bs, t);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < WBK; kk += 2) {            // lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]
      const int k = kk + (lane >> 5);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * WLD + wm + (lane & 31)], Bs[k * WLD + wn + (lane & 31)], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int n = n0 + wn + (lane & 31);
  if (n >= g.N) return;
  float bias = 0.f;
  if (g.epi >= WEPI_BIAS && g.epi <= WEPI_BIAS_TANH) bias = g.bias[(long long)e * g.sbe + n];
  float* C = g.C + (long long)e * g.sCe;
#pragma unroll
  for (int r = 0; r < 16; ++r) {                     // C/D: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= g.M) continue;
    float v = acc[r];
    switch (g.epi) {
      case WEPI_BIAS: v += bias; break;
      case WEPI_BIAS_RELU: v = fmaxf(v + bias, 0.f); break;
      case WEPI_BIAS_TANH: v = g.max_action * tanhf(v + bias); break;
      case WEPI_RELU_MASK: v = g.mask[(long long)e * g.sme + (long long)m * g.ldmask + n] > 0.f ? v : 0.f; break;
      default: break;
    }
    C[(long long)m * g.ldc + n] = v;
  }
}

static int launch_wide_gemm(const WideGemm& g, int members, hipStream_t st, int prof) {
  ProfScope scope(prof, st);
  hipLaunchKernelGGL(k_wide_gemm, dim3((unsigned)cdiv(g.N, WBN), (unsigned)cdiv(g.M, WBM), (unsigned)members), dim3(256), 0, st, g);
  MB_LAUNCH_OK("k_wide_gemm");
  return 0;
}

// x[e][r][0, Kp1) = [src0 | src1 | src2 | 0]: source i is [period_i][w_i] row major, read at row r % period_i, member e at
// src_i + e * ms_i (0: shared)
struct WideConcat {
  const float* src[3];
  int w[3];
  long long ms[3], period[3];
  float* x;
  long long rows;
  int Kp1, xm;
};
__global__ __launch_bounds__(256) void k_wide_concat(WideConcat a) {
  const long long total = (long long)a.xm * a.rows * a.Kp1;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % a.Kp1);
  const long long r = (i / a.Kp1) % a.rows;
  const int e = (int)(i / ((long long)a.Kp1 * a.rows));
  float v = 0.f;
  int c0 = 0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (c >= c0 && c < c0 + a.w[s]) v = a.src[s][(long long)e * a.ms[s] + (r % a.period[s]) * a.w[s] + (c - c0)];
    c0 += a.w[s];
  }
  a.x[i] = v;
}

// Bias gradients of the three layers in one launch: db[e][n] = sum_r dz[e][r][n].  A workgroup owns 32 columns; row group
// g = t / 32 sums rows r = g (mod 8) in ascending order, then thread g = 0 adds the eight partial sums in ascending g.
struct WideBiasJob { const float* dz; long long ld, se; float* db; long long sde; int N, NB; };
struct WideBias { WideBiasJob job[3]; long long rows; };
__global__ __launch_bounds__(256) void k_wide_bias(WideBias a) {
  __shared__ float part[8][32];
  const WideBiasJob j = a.job[blockIdx.y];
  const int e = blockIdx.z, col = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + col;
  if (blockIdx.x * 32 >= j.N) return;
  float s = 0.f;
  if (n < j.NB)
    for (long long r = grp; r < a.rows; r += 8) s += j.dz[(long long)e * j.se + r * j.ld + n];
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0 && n < j.N) {
    float tot = part[0][col];
#pragma unroll
    for (int q = 1; q < 8; ++q) tot += part[q][col];
    j.db[(long long)e * j.sde + n] = tot;
  }
}

// torch.optim.Adam (defaults) on a flat blob: the op forms of train.h's adam_element, without its transposes and planes
struct WideAdamArgs { float *p, *m, *v; const float* g; long long n; const long long* t_dev; float lr, step_size, bc2_sqrt; };
__global__ __launch_bounds__(256) void k_wide_adam(WideAdamArgs a) {
  __shared__ float sm2[2];
  float step_size = a.step_size, bc2_sqrt = a.bc2_sqrt;
  if (a.t_dev != nullptr) {                      // graph replay: bias corrections of the device step count, once per workgroup
    if (threadIdx.x == 0) adam_dev_consts(a.t_dev, a.lr, sm2);
    __syncthreads();
    step_size = sm2[0]; bc2_sqrt = sm2[1];
  }
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const float gj = a.g[j], m0 = a.m[j];
  const float mj = m0 + ADAM_W1 * (gj - m0);
  const float vj = ADAM_B2 * a.v[j] + ADAM_W2 * (gj * gj);
  a.p[j] = a.p[j] - step_size * (mj / (sqrtf(vj) / bc2_sqrt + ADAM_EPS));
  a.m[j] = mj; a.v[j] = vj;
}

static int check_wide_layout(const char* who, const MobodyWideLayout* L) {
  MB_REQUIRE(L != nullptr, "%s: null layout", who);
  MobodyWideLayout w;
  const int rc = mobody_wide_layout(L->in_dim, L->hidden, L->out_dim, L->members, &w);
  if (rc) return rc;
  MB_REQUIRE(w.Kp1 == L->Kp1 && w.Hp == L->Hp && w.Np3 == L->Np3 && w.w1 == L->w1 && w.b1 == L->b1 && w.w2 == L->w2 && w.b2 == L->b2 &&
                 w.w3 == L->w3 && w.b3 == L->b3 && w.member_floats == L->member_floats && w.total_floats == L->total_floats,
             "%s: the layout is not mobody_wide_layout's", who);
  return 0;
}

// The three products of the input-gradient chain, shared by mobody_wide_mlp3_backward and mobody_wide_mlp3_input_grad (the same
// problems, so the same bits).  dz2 = (dz3 W3^T) [h2 > 0]
static WideGemm gemm_dz2(const MobodyWideBwd* a, float* dz2) {
  const MobodyWideLayout& L = a->layout;
  const long long rows = a->rows, act = rows * L.Hp;
  WideGemm g{};
  g.A = a->dz3; g.sAe = rows * L.out_dim; g.sAm = L.out_dim; g.sAk = 1;
  g.B = a->blob + L.w3; g.sBe = L.member_floats; g.sBk = 1; g.sBn = L.Np3;
  g.C = dz2; g.sCe = act; g.ldc = L.Hp;
  g.M = g.MA = (int)rows; g.N = g.NB = L.Hp; g.K = L.out_dim;
  g.epi = WEPI_RELU_MASK; g.mask = a->h2; g.sme = act; g.ldmask = L.Hp;
  return g;
}
// dz1 = (dz2 W2^T) [h1 > 0]
static WideGemm gemm_dz1(const MobodyWideBwd* a, const float* dz2, float* dz1) {
  const MobodyWideLayout& L = a->layout;
  const long long rows = a->rows, act = rows * L.Hp;
  WideGemm g{};
  g.A = dz2; g.sAe = act; g.sAm = L.Hp; g.sAk = 1;
  g.B = a->blob + L.w2; g.sBe = L.member_floats; g.sBk = 1; g.sBn = L.Hp;
  g.C = dz1; g.sCe = act; g.ldc = L.Hp;
  g.M = g.MA = (int)rows; g.N = g.NB = L.Hp; g.K = L.Hp;
  g.epi = WEPI_RELU_MASK; g.mask = a->h1; g.sme = act; g.ldmask = L.Hp;
  return g;
}
// dX[:, col0:col1] = dz1 W1[col0:col1, :]^T
static WideGemm gemm_dx(const MobodyWideBwd* a, const float* dz1) {
  const MobodyWideLayout& L = a->layout;
  const long long rows = a->rows, act = rows * L.Hp;
  const int w = a->dx_col1 - a->dx_col0;
  WideGemm g{};
  g.A = dz1; g.sAe = act; g.sAm = L.Hp; g.sAk = 1;
  g.B = a->blob + L.w1 + (long long)a->dx_col0 * L.Hp; g.sBe = L.member_floats; g.sBk = 1; g.sBn = L.Hp;
  g.C = a->dx; g.sCe = rows * w; g.ldc = w;
  g.M = g.MA = (int)rows; g.N = g.NB = w; g.K = L.Hp; g.epi = WEPI_STORE;
  return g;
}

}  // namespace mobody

using namespace mobody;

extern "C" int mobody_wide_layout(int in_dim, int hidden, int out_dim, int members, MobodyWideLayout* out) {
  const char* who = "mobody_wide_layout";
  MB_REQUIRE(out != nullptr, "%s: null output", who);
  MB_REQUIRE(in_dim >= 1 && in_dim <= 256, "%s: in_dim %d outside [1, 256]", who, in_dim);
  MB_REQUIRE(hidden >= 8 && hidden <= 1024, "%s: hidden %d outside [8, 1024]", who, hidden);
  MB_REQUIRE(out_dim >= 1 && out_dim <= 256, "%s: out_dim %d outside [1, 256]", who, out_dim);
  MB_REQUIRE(members >= 1 && members <= 8, "%s: members %d outside [1, 8]", who, members);
  MobodyWideLayout L{};
  L.in_dim = in_dim; L.hidden = hidden; L.out_dim = out_dim; L.members = members;
  L.Kp1 = round_up(in_dim, WBK); L.Hp = round_up(hidden, 32); L.Np3 = round_up(out_dim, 32);
  L.w1 = 0;
  L.b1 = L.w1 + (int64_t)L.Kp1 * L.Hp;
  L.w2 = L.b1 + L.Hp;
  L.b2 = L.w2 + (int64_t)L.Hp * L.Hp;
  L.w3 = L.b2 + L.Hp;
  L.b3 = L.w3 + (int64_t)L.Hp * L.Np3;
  L.member_floats = L.b3 + L.Np3;
  L.total_floats = L.member_floats * members;
  *out = L;
  return 0;
}

extern "C" int64_t mobody_wide_mlp3_forward_workspace(const MobodyWideLayout* L, int64_t rows) {
  if (L == nullptr || rows < 0) return -1;
  return (int64_t)L->members * rows * (L->Kp1 + 2 * (int64_t)L->Hp);
}

extern "C" int mobody_wide_mlp3_forward(const MobodyWideFwd* a, void* stream) {
  const char* who = "mobody_wide_mlp3_forward";
  MB_BLOCK(who, a, MobodyWideFwd);
  int rc = check_wide_layout(who, &a->layout);
  if (rc) return rc;
  const MobodyWideLayout& L = a->layout;
  MB_REQUIRE(a->precision == PREC_F32, "%s: precision %d: the wide nets run in exact fp32 (precision 0) only", who, a->precision);
  MB_REQUIRE(a->rows >= 1 && a->rows <= (1 << 21), "%s: rows %lld outside [1, 2^21]", who, (long long)a->rows);
  MB_REQUIRE(a->out_mode == MOBODY_WIDE_OUT_RAW || a->out_mode == MOBODY_WIDE_OUT_TANH, "%s: out_mode %d", who, a->out_mode);
  MB_REQUIRE(a->blob && a->out, "%s: null pointer", who);
  const float* const src[3] = {a->src0, a->src1, a->src2};
  const int src_width[3] = {a->src_width0, a->src_width1, a->src_width2};
  const long long src_stride[3] = {a->src_member_stride0, a->src_member_stride1, a->src_member_stride2};
  const long long src_rows[3] = {a->src_rows0, a->src_rows1, a->src_rows2};
  int width = 0;
  bool shared = true;
  for (int s = 0; s < 3; ++s) {
    MB_REQUIRE(src_width[s] >= 0 && (src_width[s] == 0 || src[s] != nullptr), "%s: source %d: width %d, pointer %p", who, s, src_width[s],
               (const void*)src[s]);
    MB_REQUIRE(src_stride[s] >= 0, "%s: source %d: negative member stride", who, s);
    MB_REQUIRE(src_rows[s] >= 0 && src_rows[s] <= a->rows, "%s: source %d: src_rows %lld outside [0, rows]", who, s, src_rows[s]);
    width += src_width[s];
    if (src_width[s] > 0 && src_stride[s] != 0) shared = false;
  }
  MB_REQUIRE(width == L.in_dim, "%s: the sources' widths add up to %d, the net's in_dim is %d", who, width, L.in_dim);
  MB_REQUIRE(a->x_shared == (shared ? 1 : 0), "%s: x_shared %d, but the sources are %s", who, a->x_shared,
             shared ? "all shared between members" : "not all shared between members");
  const long long rows = a->rows;
  const int E = L.members, xm = shared ? 1 : E;
  float *x = a->save_x, *h1 = a->save_h1, *h2 = a->save_h2;
  if (!x || !h1 || !h2) {
    MB_REQUIRE(a->workspace != nullptr, "%s: a null save needs the workspace", who);
    float* w = a->workspace;
    if (!x) x = w;
    w += (long long)E * rows * L.Kp1;
    if (!h1) h1 = w;
    w += (long long)E * rows * L.Hp;
    if (!h2) h2 = w;
  }
  hipStream_t st = as_stream(stream);
  {
    WideConcat c{};
    for (int s = 0; s < 3; ++s) { c.src[s] = src[s]; c.w[s] = src_width[s]; c.ms[s] = src_stride[s]; c.period[s] = src_rows[s] > 0 ? src_rows[s] : a->rows; }
    c.x = x; c.rows = rows; c.Kp1 = L.Kp1; c.xm = xm;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_wide_concat, dim3((unsigned)cdiv((long long)xm * rows * L.Kp1, 256)), dim3(256), 0, st, c);
    MB_LAUNCH_OK("k_wide_concat");
  }
  const long long act = rows * L.Hp;
  WideGemm g{};
  g.A = x; g.sAe = shared ? 0 : rows * L.Kp1; g.sAm = L.Kp1; g.sAk = 1;
  g.B = a->blob + L.w1; g.sBe = L.member_floats; g.sBk = L.Hp; g.sBn = 1;
  g.C = h1; g.sCe = act; g.ldc = L.Hp;
  g.M = g.MA = (int)rows; g.N = g.NB = L.Hp; g.K = L.Kp1;
  g.epi = WEPI_BIAS_RELU; g.bias = a->blob + L.b1; g.sbe = L.member_floats;
  if ((rc = launch_wide_gemm(g, E, st, PROF_MLP_FWD))) return rc;
  g.A = h1; g.sAe = act; g.sAm = L.Hp;
  g.B = a->blob + L.w2; g.C = h2; g.K = L.Hp; g.bias = a->blob + L.b2;
  if ((rc = launch_wide_gemm(g, E, st, PROF_MLP_FWD))) return rc;
  g.A = h2;
  g.B = a->blob + L.w3; g.sBk = L.Np3;
  g.C = a->out; g.sCe = rows * L.out_dim; g.ldc = L.out_dim;
  g.N = g.NB = L.out_dim; g.bias = a->blob + L.b3;
  g.epi = a->out_mode == MOBODY_WIDE_OUT_TANH ? WEPI_BIAS_TANH : WEPI_BIAS; g.max_action = a->max_action;
  return launch_wide_gemm(g, E, st, PROF_MLP_FWD);
}

extern "C" int64_t mobody_wide_mlp3_backward_workspace(const MobodyWideLayout* L, int64_t rows) {
  if (L == nullptr || rows < 0) return -1;
  return 2 * (int64_t)L->members * rows * L->Hp;
}

extern "C" int mobody_wide_mlp3_backward(const MobodyWideBwd* a, void* stream) {
  const char* who = "mobody_wide_mlp3_backward";
  MB_BLOCK(who, a, MobodyWideBwd);
  int rc = check_wide_layout(who, &a->layout);
  if (rc) return rc;
  const MobodyWideLayout& L = a->layout;
  MB_REQUIRE(a->precision == PREC_F32, "%s: precision %d: the wide nets run in exact fp32 (precision 0) only", who, a->precision);
  MB_REQUIRE(a->rows >= 1 && a->rows <= (1 << 21), "%s: rows %lld outside [1, 2^21]", who, (long long)a->rows);
  MB_REQUIRE(a->blob && a->dz3 && a->x && a->h1 && a->h2 && a->grad && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(a->x_shared == 0 || a->x_shared == 1, "%s: x_shared %d", who, a->x_shared);
  const bool want_dx = a->dx != nullptr;
  MB_REQUIRE(!want_dx || (a->dx_col0 >= 0 && a->dx_col0 < a->dx_col1 && a->dx_col1 <= L.in_dim), "%s: dx columns [%d, %d) outside [0, %d)", who,
             a->dx_col0, a->dx_col1, L.in_dim);
  const long long rows = a->rows, act = rows * L.Hp;
  const int E = L.members;
  float *dz2 = a->workspace, *dz1 = a->workspace + E * act;
  hipStream_t st = as_stream(stream);
  WideGemm g{};
  // dW3 = h2^T dz3 (padded columns of dz3 read as 0, so the gradient's padding is written as 0)
  g.A = a->h2; g.sAe = act; g.sAm = 1; g.sAk = L.Hp;
  g.B = a->dz3; g.sBe = rows * L.out_dim; g.sBk = L.out_dim; g.sBn = 1;
  g.C = a->grad + L.w3; g.sCe = L.member_floats; g.ldc = L.Np3;
  g.M = g.MA = L.Hp; g.N = L.Np3; g.NB = L.out_dim; g.K = (int)rows; g.epi = WEPI_STORE;
  if ((rc = launch_wide_gemm(g, E, st, PROF_WGRAD))) return rc;
  if ((rc = launch_wide_gemm(gemm_dz2(a, dz2), E, st, PROF_MLP_BWD))) return rc;
  // dW2 = h1^T dz2
  g.A = a->h1; g.sAe = act; g.sAm = 1; g.sAk = L.Hp;
  g.B = dz2; g.sBe = act; g.sBk = L.Hp; g.sBn = 1;
  g.C = a->grad + L.w2; g.sCe = L.member_floats; g.ldc = L.Hp;
  g.M = g.MA = L.Hp; g.N = g.NB = L.Hp; g.K = (int)rows; g.epi = WEPI_STORE;
  if ((rc = launch_wide_gemm(g, E, st, PROF_WGRAD))) return rc;
  if ((rc = launch_wide_gemm(gemm_dz1(a, dz2, dz1), E, st, PROF_MLP_BWD))) return rc;
  // dW1 = x^T dz1
  g.A = a->x; g.sAe = a->x_shared ? 0 : rows * L.Kp1; g.sAm = 1; g.sAk = L.Kp1;
  g.B = dz1; g.sBe = act; g.sBk = L.Hp; g.sBn = 1;
  g.C = a->grad + L.w1; g.sCe = L.member_floats; g.ldc = L.Hp;
  g.M = g.MA = L.Kp1; g.N = g.NB = L.Hp; g.K = (int)rows; g.epi = WEPI_STORE;
  if ((rc = launch_wide_gemm(g, E, st, PROF_WGRAD))) return rc;
  {
    WideBias b{};
    b.rows = rows;
    b.job[0] = {dz1, L.Hp, act, a->grad + L.b1, L.member_floats, L.Hp, L.Hp};
    b.job[1] = {dz2, L.Hp, act, a->grad + L.b2, L.member_floats, L.Hp, L.Hp};
    b.job[2] = {a->dz3, L.out_dim, rows * L.out_dim, a->grad + L.b3, L.member_floats, L.Np3, L.out_dim};
    ProfScope scope(PROF_WGRAD, st);
    hipLaunchKernelGGL(k_wide_bias, dim3((unsigned)((L.Hp > L.Np3 ? L.Hp : L.Np3) / 32), 3, (unsigned)E), dim3(256), 0, st, b);
    MB_LAUNCH_OK("k_wide_bias");
  }
  if (want_dx && (rc = launch_wide_gemm(gemm_dx(a, dz1), E, st, PROF_MLP_BWD))) return rc;
  return 0;
}

extern "C" int mobody_wide_mlp3_input_grad(const MobodyWideBwd* a, void* stream) {
  const char* who = "mobody_wide_mlp3_input_grad";
  MB_BLOCK(who, a, MobodyWideBwd);
  int rc = check_wide_layout(who, &a->layout);
  if (rc) return rc;
  const MobodyWideLayout& L = a->layout;
  MB_REQUIRE(a->precision == PREC_F32, "%s: precision %d: the wide nets run in exact fp32 (precision 0) only", who, a->precision);
  MB_REQUIRE(a->rows >= 1 && a->rows <= (1 << 21), "%s: rows %lld outside [1, 2^21]", who, (long long)a->rows);
  MB_REQUIRE(a->grad == nullptr, "%s: grad must be NULL: the parameter gradient is mobody_wide_mlp3_backward's", who);
  MB_REQUIRE(a->dx != nullptr, "%s: dx is NULL: the input gradient is all this entry writes", who);
  MB_REQUIRE(a->blob && a->dz3 && a->h1 && a->h2 && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(a->x_shared == 0 || a->x_shared == 1, "%s: x_shared %d", who, a->x_shared);
  MB_REQUIRE(a->dx_col0 >= 0 && a->dx_col0 < a->dx_col1 && a->dx_col1 <= L.in_dim, "%s: dx columns [%d, %d) outside [0, %d)", who, a->dx_col0,
             a->dx_col1, L.in_dim);
  const int E = L.members;
  float *dz2 = a->workspace, *dz1 = a->workspace + E * a->rows * L.Hp;
  hipStream_t st = as_stream(stream);
  if ((rc = launch_wide_gemm(gemm_dz2(a, dz2), E, st, PROF_MLP_BWD))) return rc;
  if ((rc = launch_wide_gemm(gemm_dz1(a, dz2, dz1), E, st, PROF_MLP_BWD))) return rc;
  return launch_wide_gemm(gemm_dx(a, dz1), E, st, PROF_MLP_BWD);
}

extern "C" int mobody_wide_adam(const MobodyWideAdam* a, void* stream) {
  const char* who = "mobody_wide_adam";
  MB_BLOCK(who, a, MobodyWideAdam);
  MB_REQUIRE(a->blob && a->grad && a->m && a->v, "%s: null pointer", who);
  MB_REQUIRE(a->n >= 1, "%s: n %lld < 1", who, (long long)a->n);
  MB_REQUIRE(a->t_dev != nullptr || a->t >= 1, "%s: step t must be >= 1", who);
  WideAdamArgs k{};
  k.p = a->blob; k.m = a->m; k.v = a->v; k.g = a->grad; k.n = a->n; k.t_dev = (const long long*)a->t_dev; k.lr = a->lr;
  const double tt = a->t_dev ? 1.0 : (double)a->t;
  k.step_size = (float)((double)a->lr / (1.0 - pow(0.9, tt)));
  k.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, tt));
  hipStream_t st = as_stream(stream);
  ProfScope scope(PROF_OPTIM, st);
  hipLaunchKernelGGL(k_wide_adam, dim3((unsigned)cdiv(a->n, 256)), dim3(256), 0, st, k);
  MB_LAUNCH_OK("k_wide_adam");
  return 0;
}
