// BOSA's VAE stage (the reference's algo/offline_offline/bosa.py): the row-wise kernels between the wide nets'
// matrix products -- clamp / exp / reparameterise with the KL term and both gradient seeds, the reconstruction loss and its seed,
// the importance-weighted log-likelihood with logsumexp, min over members and the critic mask -- and the two entry points that
// chain them with csrc/wide.hip's forward / backward / Adam.  No float atomics: every sum runs in a fixed order.
#include <math.h>

#include "common.h"
#include "rng.h"

namespace mobody {

constexpr float LOG_STD_MIN = -4.f, LOG_STD_MAX = 15.f;      // bosa.py:116, :309
constexpr float LOG_SQRT_2PI = 0.9189385332046727f;

// latent noise: an explicit tensor, or element i of the device generator's stream (seed, stream, call + call_dev[0])
struct EpsSrc {
  const float* p;
  uint32_t seed, stream, call;
  const long long* call_dev;
};
__device__ __forceinline__ float eps_at(const EpsSrc& e, long long i) {
  if (e.p != nullptr) return e.p[i];
  return rng_normal_at(e.seed, e.stream, e.call + (e.call_dev ? (uint32_t)e.call_dev[0] : 0u), (uint64_t)i);
}

// sum of the workgroup's 256 values in a fixed tree order; the result is valid in thread 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// One thread per latent element i = row * Lz + l.  Forward (z != null): z = mean + exp(clamp(log_std)) * eps.  KL (lossp != null):
// the workgroup's sum of 1 + log(std^2) - mean^2 - std^2.  Seeds (denc != null): d(L + beta KL)/d(mean | log_std) from dz = dL/dz.
struct ReparamArgs {
  const float* enc;   // [n][2 Lz]
  EpsSrc eps;
  const float* dz;    // [n][Lz] or null
  long long total;    // n Lz
  int Lz;
  float beta_over_n;  // beta / (n Lz): the KL term's weight per element
  float *z, *denc, *lossp;
};
__global__ __launch_bounds__(256) void k_bosa_reparam(ReparamArgs a) {
  __shared__ float red[256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float term = 0.f;
  if (i < a.total) {
    const long long row = i / a.Lz;
    const int l = (int)(i - row * a.Lz);
    const float mean = a.enc[row * 2 * a.Lz + l], pre = a.enc[row * 2 * a.Lz + a.Lz + l];
    const float std = expf(fminf(fmaxf(pre, LOG_STD_MIN), LOG_STD_MAX));
    const float eps = eps_at(a.eps, i);
    if (a.z != nullptr) a.z[i] = mean + std * eps;
    term = 1.f + logf(std * std) - mean * mean - std * std;                       // :521
    if (a.denc != nullptr) {
      const float g = a.dz[i];
      const bool pass = pre >= LOG_STD_MIN && pre <= LOG_STD_MAX;                 // torch's clamp backward: both ends inclusive
      a.denc[row * 2 * a.Lz + l] = g + a.beta_over_n * mean;
      a.denc[row * 2 * a.Lz + a.Lz + l] = pass ? g * eps * std + a.beta_over_n * (std * std - 1.f) : 0.f;
    }
  }
  if (a.lossp != nullptr) {
    const float s = block_sum256(term, red);
    if (threadIdx.x == 0) a.lossp[blockIdx.x] = s;
  }
}

// reconstruction loss and its seed (:520, :538): one thread per output element i = (e * B + b) * D + d
struct ReconArgs {
  const float *u, *target;   // [E][B][D], [B][D]
  long long total, BD;
  float two_over_n, max_action;
  int tanh_out;
  float *dz3, *lossp;
};
__global__ __launch_bounds__(256) void k_bosa_recon(ReconArgs a) {
  __shared__ float red[256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  float sq = 0.f;
  if (i < a.total) {
    const float u = a.u[i], diff = u - a.target[i % a.BD];
    sq = diff * diff;
    float g = a.two_over_n * diff;
    if (a.tanh_out) {                                  // u = max_action * y, y = tanh(.): dy = 1 - y^2
      const float y = u / a.max_action;
      g = g * a.max_action * (1.f - y * y);
    }
    a.dz3[i] = g;
  }
  const float s = block_sum256(sq, red);
  if (threadIdx.x == 0) a.lossp[blockIdx.x] = s;
}

// out = (recon, KL, recon + beta KL) from the two partial-sum arrays, or out[0] = KL when recp is null.  One workgroup.
__global__ __launch_bounds__(256) void k_bosa_finish(const float* klp, int nkl, const float* recp, int nrec, float inv_nkl, float inv_nrec,
                                                     float beta, float* out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int j = threadIdx.x; j < nkl; j += 256) s += klp[j];
  const float kl = -0.5f * (block_sum256(s, red) * inv_nkl);
  __syncthreads();
  if (recp == nullptr) {
    if (threadIdx.x == 0) out[0] = kl;
    return;
  }
  s = 0.f;
  for (int j = threadIdx.x; j < nrec; j += 256) s += recp[j];
  const float rec = block_sum256(s, red) * inv_nrec;
  if (threadIdx.x == 0) { out[0] = rec; out[1] = kl; out[2] = rec + beta * kl; }
}

// Estimator, sampling half (:84-86, :94-98 | :275-277, :287-291): one thread per (member e, sample s, row b).  Writes the decoder's
// latent rows z[e][s B + b][Lz] and pq[e][s B + b] = (sum log N(z; 0, 1), sum log N(z; mean, std)).
struct LlSampleArgs {
  const float* enc;   // [E][B][2 Lz]
  EpsSrc eps;
  long long B;
  int E, n, Lz, policy_layout;
  float *z, *pq;
};
__global__ __launch_bounds__(256) void k_bosa_ll_sample(LlSampleArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.E * a.n * a.B) return;
  const long long b = i % a.B;
  const int s = (int)((i / a.B) % a.n), e = (int)(i / (a.B * a.n));
  const float* enc = a.enc + ((long long)e * a.B + b) * 2 * a.Lz;
  const long long erow = a.policy_layout ? b * a.n + s : ((long long)s * a.E + e) * a.B + b;      // [B][n] | [n][E][B]
  float* z = a.z + ((long long)e * a.n * a.B + (long long)s * a.B + b) * a.Lz;
  float pz = 0.f, qzx = 0.f;
  for (int l = 0; l < a.Lz; ++l) {
    const float mean = enc[l];
    const float std = expf(fminf(fmaxf(enc[a.Lz + l], LOG_STD_MIN), LOG_STD_MAX));
    const float zz = mean + std * eps_at(a.eps, erow * a.Lz + l);
    z[l] = zz;
    const float d = zz - mean;
    pz += -(zz * zz) / 2.f - LOG_SQRT_2PI;                                  // td.Normal(0, 1).log_prob: var 1, log(scale) 0
    qzx += -(d * d) / (2.f * (std * std)) - logf(std) - LOG_SQRT_2PI;
  }
  a.pq[2 * i] = pz;
  a.pq[2 * i + 1] = qzx;
}

// Estimator, reducing half (:100-104 | :293-297, :585-590): one thread per row b; members in ascending order.
// torch.min propagates NaN (dyna_ll.min(dim=0), :585) and NaN > log(eps) is False, so a row on which one member's ll is NaN has
// min_ll = NaN and mask = 0; fminf would drop the NaN and let the row through on the other members (csrc/dynamics.hip's norms
// follow the same rule).
struct LlReduceArgs {
  const float *dec, *x;   // [E][n B][D], [B][D]
  float* pq;              // in: (pz, qzx); the w of each sample is kept in its first slot
  long long B;
  int E, n, D;
  float sd, log_n, log_eps;
  float *ll, *min_ll, *mask, *w_out;
};
__global__ __launch_bounds__(256) void k_bosa_ll_reduce(LlReduceArgs a) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const float var2 = 2.f * (a.sd * a.sd), log_sd = logf(a.sd);
  float lo = INFINITY;
  bool bad = false;
  for (int e = 0; e < a.E; ++e) {
    float mx = -INFINITY;
    for (int s = 0; s < a.n; ++s) {
      const long long r = (long long)e * a.n * a.B + (long long)s * a.B + b;
      const float* dec = a.dec + r * a.D;
      float pxz = 0.f;
      for (int d = 0; d < a.D; ++d) {
        const float df = a.x[b * a.D + d] - dec[d];
        pxz += -(df * df) / var2 - log_sd - LOG_SQRT_2PI;
      }
      const float w = pxz + a.pq[2 * r] - a.pq[2 * r + 1];                   // :103
      a.pq[2 * r] = w;
      if (a.w_out != nullptr) a.w_out[r] = w;
      mx = fmaxf(mx, w);
    }
    float sum = 0.f;
    for (int s = 0; s < a.n; ++s) sum += expf(a.pq[2 * ((long long)e * a.n * a.B + (long long)s * a.B + b)] - mx);
    const float ll = mx + logf(sum) - a.log_n;
    a.ll[(long long)e * a.B + b] = ll;
    bad = bad || (ll != ll);
    lo = fminf(lo, ll);
  }
  if (bad) lo = __builtin_nanf("");
  if (a.min_ll != nullptr) a.min_ll[b] = lo;
  if (a.mask != nullptr) a.mask[b] = lo > a.log_eps ? 1.f : 0.f;
}

// Estimator's gradient, decoder half: one thread per row b, as k_bosa_ll_reduce.  p_k = softmax_k(w_k) from the w kept in
// pq's first slot, the maximum subtracted as that kernel does, written into pq's second slot for the encoder half; then per action
// column the direct term -sum_k p_k (a - u_k) / var and the decoder's seed on row k B + b (the tanh's derivative folded in); samples in
// ascending order.  var = sd * sd with the forward's sd = (float)sqrt(beta / 4), so that the term is the derivative of the pxz the
// forward formed (var2 = 2 sd sd there); the rounded beta / 4 differs from it in the last place.
struct LlgSeedArgs {
  const float *u, *action;   // [n B][A], [B][A]
  float* pq;
  long long B;
  int n, A;
  float sd, max_action;
  float *direct, *seed;      // [B][A], [n B][A]
};
__global__ __launch_bounds__(256) void k_bosa_llg_seed(LlgSeedArgs a) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const float var = a.sd * a.sd;
  float mx = -INFINITY;
  for (int k = 0; k < a.n; ++k) mx = fmaxf(mx, a.pq[2 * ((long long)k * a.B + b)]);
  float sum = 0.f;
  for (int k = 0; k < a.n; ++k) sum += expf(a.pq[2 * ((long long)k * a.B + b)] - mx);
  for (int k = 0; k < a.n; ++k) {
    const long long r = (long long)k * a.B + b;
    a.pq[2 * r + 1] = expf(a.pq[2 * r] - mx) / sum;
  }
  for (int j = 0; j < a.A; ++j) {
    const float act = a.action[b * a.A + j];
    float direct = 0.f;
    for (int k = 0; k < a.n; ++k) {
      const long long r = (long long)k * a.B + b;
      const float u = a.u[r * a.A + j], y = u / a.max_action;
      const float pr = a.pq[2 * r + 1] * ((act - u) / var);
      direct -= pr;
      a.seed[r * a.A + j] = pr * a.max_action * (1.f - y * y);
    }
    a.direct[b * a.A + j] = direct;
  }
}

// Encoder half: one thread per latent element (b, l).  g_k = dz_k - p_k z_k; denc[b] = [sum_k g_k | pass (sum_k g_k eps_k std + 1)],
// pass as in k_bosa_reparam.
struct LlgEncArgs {
  const float *enc, *z, *dz, *pq;   // [B][2 Lz], [n B][Lz], [n B][Lz], p_k in the second slot
  EpsSrc eps;                       // [B][n][Lz]
  long long B;
  int n, Lz;
  float* denc;                      // [B][2 Lz]
};
__global__ __launch_bounds__(256) void k_bosa_llg_enc(LlgEncArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.Lz) return;
  const long long b = i / a.Lz;
  const int l = (int)(i - b * a.Lz);
  const float pre = a.enc[b * 2 * a.Lz + a.Lz + l];
  const float std = expf(fminf(fmaxf(pre, LOG_STD_MIN), LOG_STD_MAX));
  float gm = 0.f, gs = 0.f;
  for (int k = 0; k < a.n; ++k) {
    const long long r = (long long)k * a.B + b;
    const float g = a.dz[r * a.Lz + l] - a.pq[2 * r + 1] * a.z[r * a.Lz + l];
    gm += g;
    gs += g * eps_at(a.eps, (b * a.n + k) * a.Lz + l) * std;
  }
  const bool pass = pre >= LOG_STD_MIN && pre <= LOG_STD_MAX;
  a.denc[b * 2 * a.Lz + l] = gm;
  a.denc[b * 2 * a.Lz + a.Lz + l] = pass ? gs + 1.f : 0.f;
}

__global__ __launch_bounds__(256) void k_bosa_llg_sum(const float* direct, const float* dxa, long long total, float* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) out[i] = direct[i] + dxa[i];
}

__global__ __launch_bounds__(256) void k_bosa_mask_mean(const float* mask, long long B, float* out) {
  __shared__ float red[256];
  float s = 0.f;                                       // a count below 2^24: exact in any order
  for (long long j = threadIdx.x; j < B; j += 256) s += mask[j];
  const float tot = block_sum256(s, red);
  if (threadIdx.x == 0) out[0] = tot / (float)B;
}

struct BosaNets {
  MobodyWideLayout enc, dec;
  int Lz, D, E;
  bool policy;
};
struct BosaWs {
  float *enc_x, *enc_h1, *enc_h2, *enc_out, *z, *dec_x, *dec_h1, *dec_h2, *u, *dz3_dec, *dxz, *denc, *bwd, *klp, *recp, *pq;
  long long floats;
};

static int bosa_nets(const char* who, const MobodyBosaVae* a, BosaNets& n) {
  MB_REQUIRE(a->kind == MOBODY_BOSA_POLICY || a->kind == MOBODY_BOSA_DYNAMICS, "%s: kind %d", who, a->kind);
  MB_REQUIRE(a->S >= 1 && a->A >= 1, "%s: S %d, A %d", who, a->S, a->A);
  n.policy = a->kind == MOBODY_BOSA_POLICY;
  MB_REQUIRE(!n.policy || a->members == 1, "%s: members %d: the policy VAE has one member", who, a->members);
  n.E = a->members;
  int rc;
  if (n.policy) {
    n.Lz = 2 * a->A; n.D = a->A;
    if ((rc = mobody_wide_layout(a->S + a->A, a->hidden, 2 * n.Lz, 1, &n.enc))) return rc;
    rc = mobody_wide_layout(a->S + n.Lz, a->hidden, a->A, 1, &n.dec);
  } else {
    n.Lz = 2 * a->S; n.D = a->S;
    if ((rc = mobody_wide_layout(2 * a->S + a->A, a->hidden, 2 * n.Lz, a->members, &n.enc))) return rc;
    rc = mobody_wide_layout(a->S + a->A + n.Lz, a->hidden, a->S, a->members, &n.dec);
  }
  return rc;
}

static void bosa_carve(const BosaNets& n, long long B, int ns, float* base, BosaWs& w) {
  const long long E = n.E, nB = (long long)ns * B, Hp = n.enc.Hp;
  Carver take{base};
  w.enc_x = take(B * n.enc.Kp1);
  w.enc_h1 = take(E * B * Hp); w.enc_h2 = take(E * B * Hp);
  w.enc_out = take(E * B * 2 * n.Lz);
  w.z = take(E * nB * n.Lz);
  w.dec_x = take(E * nB * n.dec.Kp1);
  w.dec_h1 = take(E * nB * Hp); w.dec_h2 = take(E * nB * Hp);
  w.u = take(E * nB * n.D);
  w.dz3_dec = take(E * B * n.D);
  w.dxz = take(E * B * n.Lz);
  w.denc = take(E * B * 2 * n.Lz);
  w.bwd = take(2 * E * B * Hp);
  w.klp = take(cdiv(E * B * n.Lz, 256));
  w.recp = take(cdiv(E * B * n.D, 256));
  w.pq = take(2 * E * nB);
  w.floats = take.off;
}

static int bosa_common(const char* who, const MobodyBosaVae* a, BosaNets& n) {
  MB_BLOCK(who, a, MobodyBosaVae);
  const int rc = bosa_nets(who, a, n);
  if (rc) return rc;
  MB_REQUIRE(a->precision == PREC_F32, "%s: precision %d: the wide nets run in exact fp32 (precision 0) only", who, a->precision);
  MB_REQUIRE(a->B >= 1 && a->B <= (1 << 21), "%s: B %lld outside [1, 2^21]", who, (long long)a->B);
  MB_REQUIRE(a->beta > 0.f, "%s: beta %g <= 0", who, (double)a->beta);
  return 0;
}

static MobodyWideFwd enc_forward(const MobodyBosaVae* a, const BosaNets& n, const BosaWs& w) {
  MobodyWideFwd f{};
  f.struct_bytes = (int32_t)sizeof(f); f.layout = n.enc; f.blob = a->blob;
  f.src0 = a->state; f.src_width0 = a->S; f.src1 = a->action; f.src_width1 = a->A;
  if (!n.policy) { f.src2 = a->next_state; f.src_width2 = a->S; }
  f.x_shared = 1; f.rows = a->B; f.out_mode = MOBODY_WIDE_OUT_RAW;
  f.out = w.enc_out; f.save_x = w.enc_x; f.save_h1 = w.enc_h1; f.save_h2 = w.enc_h2;
  return f;
}

// the decoder on `rows` = copies * B rows: the batch's own tensors repeat every B rows, the latent has one row per row
static MobodyWideFwd dec_forward(const MobodyBosaVae* a, const BosaNets& n, const BosaWs& w, long long rows) {
  MobodyWideFwd f{};
  f.struct_bytes = (int32_t)sizeof(f); f.layout = n.dec; f.blob = a->blob + n.enc.total_floats;
  f.src0 = a->state; f.src_width0 = a->S; f.src_rows0 = a->B;
  if (n.policy) {
    f.src1 = w.z; f.src_width1 = n.Lz;
    f.x_shared = 1; f.out_mode = MOBODY_WIDE_OUT_TANH; f.max_action = a->max_action;
  } else {
    f.src1 = a->action; f.src_width1 = a->A; f.src_rows1 = a->B;
    f.src2 = w.z; f.src_width2 = n.Lz; f.src_member_stride2 = rows * n.Lz;
    f.x_shared = 0; f.out_mode = MOBODY_WIDE_OUT_RAW;
  }
  f.rows = rows;
  f.out = w.u; f.save_x = w.dec_x; f.save_h1 = w.dec_h1; f.save_h2 = w.dec_h2;
  return f;
}

static EpsSrc eps_src(const MobodyBosaVae* a, uint32_t stream) {
  return EpsSrc{a->eps, a->seed, stream, a->call, (const long long*)a->call_dev};
}

}  // namespace mobody

using namespace mobody;

extern "C" int64_t mobody_bosa_workspace(const MobodyBosaVae* a) {
  BosaNets n;
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyBosaVae) || a->B < 1 || a->num_samples < 0 || a->num_samples > 64 ||
      bosa_nets("mobody_bosa_workspace", a, n))
    return -1;
  BosaWs w;
  bosa_carve(n, a->B, a->num_samples > 1 ? a->num_samples : 1, nullptr, w);
  return w.floats;
}

extern "C" int mobody_bosa_reparam(const float* enc, const float* eps, const float* dz, int64_t n, int32_t Lz, float beta, float* z,
                                   float* denc, float* lossp, float* kl_out, void* stream) {
  const char* who = "mobody_bosa_reparam";
  MB_REQUIRE(n >= 1 && Lz >= 1 && n * Lz <= (1ll << 31), "%s: n %lld, Lz %d", who, (long long)n, Lz);
  MB_REQUIRE(enc && eps && z && lossp && kl_out, "%s: null pointer", who);
  MB_REQUIRE((dz != nullptr) == (denc != nullptr), "%s: dz and denc come together", who);
  ReparamArgs r{};
  r.enc = enc; r.eps.p = eps; r.dz = dz; r.total = n * Lz; r.Lz = Lz; r.beta_over_n = (float)((double)beta / (double)(n * Lz));
  r.z = z; r.denc = denc; r.lossp = lossp;
  hipStream_t st = as_stream(stream);
  const int nb = (int)cdiv(r.total, 256);
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_reparam, dim3((unsigned)nb), dim3(256), 0, st, r);
  MB_LAUNCH_OK("k_bosa_reparam");
  hipLaunchKernelGGL(k_bosa_finish, dim3(1), dim3(256), 0, st, (const float*)lossp, nb, (const float*)nullptr, 0, (float)(1.0 / (double)r.total), 0.f,
                     beta, kl_out);
  MB_LAUNCH_OK("k_bosa_finish");
  return 0;
}

extern "C" int mobody_bosa_vae(const MobodyBosaVae* a, void* stream) {
  const char* who = "mobody_bosa_vae";
  BosaNets n;
  int rc = bosa_common(who, a, n);
  if (rc) return rc;
  MB_REQUIRE((a->m != nullptr) == (a->v != nullptr), "%s: one of m, v without the other", who);
  MB_REQUIRE(a->m == nullptr || a->t_dev != nullptr || a->t >= 1, "%s: step t must be >= 1", who);
  MB_REQUIRE(a->blob && a->state && a->action && (n.policy || a->next_state) && a->grad && a->loss_out && a->workspace, "%s: null pointer", who);
  BosaWs w;
  bosa_carve(n, a->B, 1, a->workspace, w);
  hipStream_t st = as_stream(stream);
  const long long B = a->B, E = n.E, nz = E * B * n.Lz, nd = E * B * n.D;
  const EpsSrc eps = eps_src(a, n.policy ? MOBODY_BOSA_STREAM_POLICY : MOBODY_BOSA_STREAM_DYNAMICS);
  const float beta_over_n = (float)((double)a->beta / (double)nz);

  const MobodyWideFwd fe = enc_forward(a, n, w);
  if ((rc = mobody_wide_mlp3_forward(&fe, stream))) return rc;
  ReparamArgs r{};
  r.enc = w.enc_out; r.eps = eps; r.total = nz; r.Lz = n.Lz; r.beta_over_n = beta_over_n; r.z = w.z; r.lossp = w.klp;
  {
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_reparam, dim3((unsigned)cdiv(nz, 256)), dim3(256), 0, st, r);
    MB_LAUNCH_OK("k_bosa_reparam");
  }
  const MobodyWideFwd fd = dec_forward(a, n, w, B);
  if ((rc = mobody_wide_mlp3_forward(&fd, stream))) return rc;
  {
    ReconArgs c{};
    c.u = w.u; c.target = n.policy ? a->action : a->next_state; c.total = nd; c.BD = B * n.D;
    c.two_over_n = (float)(2.0 / (double)nd); c.max_action = a->max_action; c.tanh_out = n.policy ? 1 : 0;
    c.dz3 = w.dz3_dec; c.lossp = w.recp;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_recon, dim3((unsigned)cdiv(nd, 256)), dim3(256), 0, st, c);
    MB_LAUNCH_OK("k_bosa_recon");
    hipLaunchKernelGGL(k_bosa_finish, dim3(1), dim3(256), 0, st, (const float*)w.klp, (int)cdiv(nz, 256), (const float*)w.recp, (int)cdiv(nd, 256),
                       (float)(1.0 / (double)nz), (float)(1.0 / (double)nd), a->beta, a->loss_out);
    MB_LAUNCH_OK("k_bosa_finish");
  }
  MobodyWideBwd bd{};
  bd.struct_bytes = (int32_t)sizeof(bd); bd.layout = n.dec; bd.blob = fd.blob; bd.dz3 = w.dz3_dec; bd.x = w.dec_x; bd.h1 = w.dec_h1; bd.h2 = w.dec_h2;
  bd.x_shared = fd.x_shared; bd.rows = B; bd.grad = a->grad + n.enc.total_floats;
  bd.dx = w.dxz; bd.dx_col0 = n.dec.in_dim - n.Lz; bd.dx_col1 = n.dec.in_dim; bd.workspace = w.bwd;
  if ((rc = mobody_wide_mlp3_backward(&bd, stream))) return rc;
  r.dz = w.dxz; r.z = nullptr; r.lossp = nullptr; r.denc = w.denc;
  {
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_reparam, dim3((unsigned)cdiv(nz, 256)), dim3(256), 0, st, r);
    MB_LAUNCH_OK("k_bosa_reparam");
  }
  MobodyWideBwd be{};
  be.struct_bytes = (int32_t)sizeof(be); be.layout = n.enc; be.blob = a->blob; be.dz3 = w.denc; be.x = w.enc_x; be.h1 = w.enc_h1; be.h2 = w.enc_h2;
  be.x_shared = 1; be.rows = B; be.grad = a->grad; be.workspace = w.bwd;
  if ((rc = mobody_wide_mlp3_backward(&be, stream))) return rc;
  if (a->m != nullptr) {
    MobodyWideAdam ad{};
    ad.struct_bytes = (int32_t)sizeof(ad); ad.blob = a->blob; ad.grad = a->grad; ad.m = a->m; ad.v = a->v;
    ad.n = n.enc.total_floats + n.dec.total_floats; ad.t = a->t; ad.t_dev = a->t_dev; ad.lr = a->lr;
    if ((rc = mobody_wide_adam(&ad, stream))) return rc;
  }
  return 0;
}

extern "C" int mobody_bosa_loglik(const MobodyBosaVae* a, void* stream) {
  const char* who = "mobody_bosa_loglik";
  BosaNets n;
  int rc = bosa_common(who, a, n);
  if (rc) return rc;
  MB_REQUIRE(a->num_samples >= 1 && a->num_samples <= 64, "%s: num_samples %d outside [1, 64]", who, a->num_samples);
  MB_REQUIRE(a->grad == nullptr && a->m == nullptr && a->v == nullptr, "%s: forward only: grad, m, v must be NULL", who);
  MB_REQUIRE(a->blob && a->state && a->action && (n.policy || a->next_state) && a->ll && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(a->mask_mean == nullptr || a->mask != nullptr, "%s: mask_mean needs mask", who);
  const int ns = a->num_samples;
  const long long B = a->B, rows = (long long)ns * B;
  MB_REQUIRE(rows <= (1 << 21), "%s: num_samples * B = %lld > 2^21", who, rows);
  BosaWs w;
  bosa_carve(n, B, ns, a->workspace, w);
  hipStream_t st = as_stream(stream);
  const MobodyWideFwd fe = enc_forward(a, n, w);
  if ((rc = mobody_wide_mlp3_forward(&fe, stream))) return rc;
  {
    LlSampleArgs s{};
    s.enc = w.enc_out; s.eps = eps_src(a, n.policy ? MOBODY_BOSA_STREAM_POLICY_LL : MOBODY_BOSA_STREAM_DYNAMICS_LL);
    s.B = B; s.E = n.E; s.n = ns; s.Lz = n.Lz; s.policy_layout = n.policy ? 1 : 0; s.z = w.z; s.pq = w.pq;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_ll_sample, dim3((unsigned)cdiv((long long)n.E * rows, 256)), dim3(256), 0, st, s);
    MB_LAUNCH_OK("k_bosa_ll_sample");
  }
  const MobodyWideFwd fd = dec_forward(a, n, w, rows);
  if ((rc = mobody_wide_mlp3_forward(&fd, stream))) return rc;
  LlReduceArgs q{};
  q.dec = w.u; q.x = n.policy ? a->action : a->next_state; q.pq = w.pq; q.B = B; q.E = n.E; q.n = ns; q.D = n.D;
  q.sd = (float)sqrt((double)a->beta / 4.0); q.log_n = (float)log((double)ns); q.log_eps = a->log_eps;
  q.ll = a->ll; q.min_ll = a->min_ll; q.mask = a->mask; q.w_out = a->w_out;
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_ll_reduce, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, q);
  MB_LAUNCH_OK("k_bosa_ll_reduce");
  if (a->mask_mean != nullptr) {
    hipLaunchKernelGGL(k_bosa_mask_mean, dim3(1), dim3(256), 0, st, (const float*)a->mask, B, a->mask_mean);
    MB_LAUNCH_OK("k_bosa_mask_mean");
  }
  return 0;
}

// the gradient's workspace: mobody_bosa_workspace's pieces first (the forward runs on them as it is), then the pieces on n B rows
struct BosaGradWs {
  float *seed, *dz, *bwd, *dxa, *direct;
  long long floats;
};
static void bosa_grad_carve(const BosaNets& n, long long B, int ns, float* base, BosaWs& w, BosaGradWs& g) {
  bosa_carve(n, B, ns, base, w);
  const long long nB = (long long)ns * B;
  Carver take{base, w.floats};
  g.seed = take(nB * n.D);
  g.dz = take(nB * n.Lz);
  g.bwd = take(2 * nB * n.dec.Hp);
  g.dxa = take(B * n.D);
  g.direct = take(B * n.D);
  g.floats = take.off;
}

extern "C" int64_t mobody_bosa_loglik_grad_workspace(const MobodyBosaVae* a) {
  BosaNets n;
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyBosaVae) || a->kind != MOBODY_BOSA_POLICY || a->B < 1 || a->num_samples < 1 ||
      a->num_samples > 64 || bosa_nets("mobody_bosa_loglik_grad_workspace", a, n))
    return -1;
  BosaWs w;
  BosaGradWs g;
  bosa_grad_carve(n, a->B, a->num_samples, nullptr, w, g);
  return g.floats;
}

extern "C" int mobody_bosa_loglik_grad(const MobodyBosaVae* a, float* dll_da, void* stream) {
  const char* who = "mobody_bosa_loglik_grad";
  MB_BLOCK(who, a, MobodyBosaVae);
  MB_REQUIRE(a->kind == MOBODY_BOSA_POLICY, "%s: kind %d: the gradient is the policy VAE's (kind 0); the dynamics estimator is only used without one", who,
             a->kind);
  BosaNets n;
  int rc = bosa_common(who, a, n);
  if (rc) return rc;
  MB_REQUIRE(a->num_samples >= 1 && a->num_samples <= 64, "%s: num_samples %d outside [1, 64]", who, a->num_samples);
  MB_REQUIRE(a->grad == nullptr && a->m == nullptr && a->v == nullptr, "%s: grad, m, v must be NULL: the VAE's parameters are held fixed", who);
  MB_REQUIRE(a->blob && a->state && a->action && a->ll && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(dll_da != nullptr, "%s: dll_da is NULL", who);
  MB_REQUIRE(a->mask_mean == nullptr || a->mask != nullptr, "%s: mask_mean needs mask", who);
  const int ns = a->num_samples;
  const long long B = a->B, rows = (long long)ns * B;
  MB_REQUIRE(rows <= (1 << 21), "%s: num_samples * B = %lld > 2^21", who, rows);
  // grids: B, B A and B Lz threads in 256s.  The layouts bound A by 64 (4 A <= 256) and B <= 2^21, so at most 2^20 workgroups: the
  // check below cannot fail under the bounds above and states the limit the launches rely on.
  MB_REQUIRE(cdiv(B * n.Lz, 256) <= 0x7fffffffLL, "%s: B %lld: grid of %lld workgroups", who, B, (long long)cdiv(B * n.Lz, 256));
  BosaWs w;
  BosaGradWs g;
  bosa_grad_carve(n, B, ns, a->workspace, w, g);
  if ((rc = mobody_bosa_loglik(a, stream))) return rc;      // ll, w_out; leaves x, h1, h2 of both nets, enc_out, z, u and w in the workspace
  hipStream_t st = as_stream(stream);
  {
    LlgSeedArgs s{};
    s.u = w.u; s.action = a->action; s.pq = w.pq; s.B = B; s.n = ns; s.A = n.D;
    s.sd = (float)sqrt((double)a->beta / 4.0); s.max_action = a->max_action; s.direct = g.direct; s.seed = g.seed;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_llg_seed, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, st, s);
    MB_LAUNCH_OK("k_bosa_llg_seed");
  }
  MobodyWideBwd bd{};
  bd.struct_bytes = (int32_t)sizeof(bd); bd.layout = n.dec; bd.blob = a->blob + n.enc.total_floats; bd.dz3 = g.seed;
  bd.x = w.dec_x; bd.h1 = w.dec_h1; bd.h2 = w.dec_h2; bd.x_shared = 1; bd.rows = rows;
  bd.dx = g.dz; bd.dx_col0 = n.dec.in_dim - n.Lz; bd.dx_col1 = n.dec.in_dim; bd.workspace = g.bwd;
  if ((rc = mobody_wide_mlp3_input_grad(&bd, stream))) return rc;
  {
    LlgEncArgs e{};
    e.enc = w.enc_out; e.z = w.z; e.dz = g.dz; e.pq = w.pq; e.eps = eps_src(a, MOBODY_BOSA_STREAM_POLICY_LL);
    e.B = B; e.n = ns; e.Lz = n.Lz; e.denc = w.denc;
    ProfScope scope(PROF_ROWWISE, st);
    hipLaunchKernelGGL(k_bosa_llg_enc, dim3((unsigned)cdiv(B * n.Lz, 256)), dim3(256), 0, st, e);
    MB_LAUNCH_OK("k_bosa_llg_enc");
  }
  MobodyWideBwd be{};
  be.struct_bytes = (int32_t)sizeof(be); be.layout = n.enc; be.blob = a->blob; be.dz3 = w.denc;
  be.x = w.enc_x; be.h1 = w.enc_h1; be.h2 = w.enc_h2; be.x_shared = 1; be.rows = B;
  be.dx = g.dxa; be.dx_col0 = a->S; be.dx_col1 = a->S + a->A; be.workspace = w.bwd;
  if ((rc = mobody_wide_mlp3_input_grad(&be, stream))) return rc;
  ProfScope scope(PROF_ROWWISE, st);
  hipLaunchKernelGGL(k_bosa_llg_sum, dim3((unsigned)cdiv(B * n.D, 256)), dim3(256), 0, st, (const float*)g.direct, (const float*)g.dxa, B * n.D, dll_da);
  MB_LAUNCH_OK("k_bosa_llg_sum");
  return 0;
}
