// MOBODY gradient step: critic (twin-Q TD regression) and actor (Q-scaled policy gradient +
// Q-weighted behaviour cloning), assembled from the fused MLP forward/backward kernels (which also form the row-wise
// quantities in their prologues, mlp_bwd.hip) plus the few row-wise kernels below.  Reference: algo/offline_offline/mobody.py:189-208 (critic),
// :246-276 (bc_loss), :314-345 (update_policy), :540-578 (order of updates), :183-187 (Polyak).
//
// Row-wise kernels are HBM-streaming (a few floats per row); the scalar reductions are
// single-workgroup and deterministic (no atomics), so N-GPU == 1-GPU to rounding.
#include <math.h>

#include "common.h"
#include "dara.h"
#include "igdf.h"
#include "layers.h"
#include "train.h"

namespace mobody {

// ------------------------------------------------------------------------------------------------
// workspace carving
// ------------------------------------------------------------------------------------------------
struct TrainWs {
  uint32_t *mq1, *mq2, *ma1, *ma2;      // ReLU sign words of the twin-Q / actor hidden layers
  int *eh1q, *eh1a, *edz2;              // f16 mode: scale exponents of the 32-row tiles of the h1 / dz2 planes
  float *pin;            // pi(s') of the critic phase (pi holds pi(s) for the actor phase)
  float *pi, *qt, *q, *qb, *xq, *h1q, *h2q, *xa, *h1a, *h2a, *dz3q, *dz2, *dz1, *dz3a, *dxa, *bcw, *dbp, *slabs, *lossp;
  float *lossp_pairs;      // seed mode 9: a pair of partial sums per (row tile, member)
  float *bc;               // Adam bias corrections of a device step count: two floats per net (critic, actor), mlp3_weight_grads
  int *tickets;            // one per row tile: arrivals of the tile's two frozen-Q workgroups in k_actor_bwd_chain (zeroed by k_actor_stats)
  int *ctickets;           // two per row tile: arrivals of (tile, member)'s two producers in k_critic_chain_bf (any contents on entry)
  long long total;
  int nsplit_q, nsplit_a, ntiles;
  MobodyMlpLayout Lq, La;
};

static int carve(const MobodyTrainDims& d, float* base, TrainWs& w) {
  int rc = mobody_mlp_layout(d.S + d.A, 1, 2, &w.Lq);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S, d.A, 1, &w.La);
  if (rc) return rc;
  const long long N = d.N, Nt = d.Nt;
  const long long N32 = (N + 31) & ~31LL;             // h1 / dz2 hold fp16 planes of whole 32-row tiles in the f16 mode (same bytes)
  Carver take{base};
  w.pi = take(N * d.A);
  w.pin = take(N * d.A);
  w.qt = take(2 * N);
  w.q = take(2 * N);
  w.qb = take(2 * Nt);
  w.xq = take(N * w.Lq.Kp1);
  w.h1q = take(2 * N32 * HID);
  w.h2q = take(2 * N * HID);
  w.xa = take(N * w.La.Kp1);
  w.h1a = take(N32 * HID);
  w.h2a = take(N * HID);
  const long long mw = cdiv(N, 32) * HID;
  w.mq1 = (uint32_t*)take(2 * mw); w.mq2 = (uint32_t*)take(2 * mw);
  w.ma1 = (uint32_t*)take(mw); w.ma2 = (uint32_t*)take(mw);
  w.eh1q = (int*)take(2 * (N32 / 32)); w.eh1a = (int*)take(N32 / 32); w.edz2 = (int*)take(2 * (N32 / 32));
  w.dz3q = take(2 * N * w.Lq.Np3);
  w.dz2 = take(2 * N32 * HID);
  w.dz1 = take(2 * N * HID);
  w.dz3a = take(N * w.La.Np3);
  w.dxa = take(2 * N * d.A);
  w.bcw = take(Nt > 0 ? Nt : 1);
  w.lossp = take(2 * cdiv(N, 32));                // per (row tile, member) / per-tile pairs, tiles of >= 32 rows
  w.ntiles = (int)cdiv(N, MLP_TILE_ROWS);         // the bias partials are per row tile
  w.nsplit_q = wgrad_nsplit(N, 2);
  w.nsplit_a = wgrad_nsplit(N, 1);
  const long long per_q = 2 * HID + w.Lq.Np3, per_a = 2 * HID + w.La.Np3;
  w.dbp = take((long long)w.ntiles * (2 * per_q > per_a ? 2 * per_q : per_a));
  {                                               // one slab area, used by the critic's and then the actor's gradients
    const long long sq = ((w.Lq.total_floats + 3) & ~3LL) * w.nsplit_q, sa = ((w.La.total_floats + 3) & ~3LL) * w.nsplit_a;
    w.slabs = take(sq > sa ? sq : sa);
  }
  w.bc = take(4);
  w.tickets = (int*)take(w.ntiles);
  w.lossp_pairs = take(4LL * w.ntiles);           // behind everything else: no other piece moves
  // The chained critic launch's tickets share the first half of these words: mode 9 (BOSA, always the separate backward launch)
  // writes every pair before the reduction reads it, and a ticket may hold anything on entry (critic_fwd_bf.hip), so neither
  // user minds what the other left.  The workspace keeps its size.
  w.ctickets = (int*)w.lossp_pairs;
  w.total = take.off;
  return 0;
}

static int check_dims(const MobodyTrainDims* d, const char* who) {
  MB_REQUIRE(d != nullptr, "%s: dims is null", who);
  MB_REQUIRE(d->N >= 1 && d->Nt >= 0 && d->Nt <= d->N, "%s: need 1 <= N and 0 <= Nt <= N (N=%lld Nt=%lld)", who,
             (long long)d->N, (long long)d->Nt);
  MB_REQUIRE(d->N_global >= d->N && d->Nt_global >= d->Nt, "%s: global row counts smaller than local", who);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// row-wise kernels
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* sm) {      // blockDim.x multiple of 64, <= 1024
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float s = 0.f;
  for (int k = 0; k < nw; ++k) s += sm[k];       // same order in every thread: deterministic
  return s;
}

// stats[0] = sum_rows |min(Q1,Q2)(s,pi(s))|, stats[1] = sum_{rows<Nt} |min(Q1,Q2)(s_t,a_t)|   (:318, :259)
// Also zeroes the tile tickets of the backward launch that follows it in every caller (k_actor_bwd_chain).
__global__ __launch_bounds__(1024) void k_actor_stats(const float* qp, const float* qb, long long N, long long Nt,
                                                      float* stats, int* tickets, int ntickets) {
  __shared__ float sm[16];
  for (int k = threadIdx.x; k < ntickets; k += 1024) tickets[k] = 0;
  constexpr int U = 4;                            // 2U independent loads in flight; each thread still adds its rows in
  float s0 = 0.f, s1 = 0.f;                       // increasing order, so the sums do not depend on U
  for (long long base = threadIdx.x; base < N; base += U * 1024) {
    float a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const long long r = base + u * 1024; const long long rc = r < N ? r : 0; a[u] = qp[rc]; b[u] = qp[N + rc]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * 1024 < N) s0 += fabsf(fminf(a[u], b[u]));
  }
  for (long long base = threadIdx.x; base < Nt; base += U * 1024) {
    float a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const long long r = base + u * 1024; const long long rc = r < Nt ? r : 0; a[u] = qb[rc]; b[u] = qb[Nt + rc]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (base + u * 1024 < Nt) s1 += fabsf(fminf(a[u], b[u]));
  }
  s0 = block_sum(s0, sm);
  s1 = block_sum(s1, sm);
  if (threadIdx.x == 0) { stats[0] = s0; stats[1] = s1; }
}

// BOSA's actor phase (bosa.py:612-629): Q is critic_1 alone.  stats[0] = sum_rows |q_0|, stats[1] = sum_rows q_0, each
// thread adding its rows in increasing order.
__global__ __launch_bounds__(1024) void k_bosa_actor_stats(const float* q0, long long N, float* stats) {
  __shared__ float sm[16];
  float s0 = 0.f, s1 = 0.f;
  for (long long r = threadIdx.x; r < N; r += 1024) { const float q = q0[r]; s0 += fabsf(q); s1 += q; }
  s0 = block_sum(s0, sm);
  s1 = block_sum(s1, sm);
  if (threadIdx.x == 0) { stats[0] = s0; stats[1] = s1; }
}
// the frozen critic_1's seed: dz3[row][0] = -(1 / m) / N_global, m = stats[0] / N_global (norm_q, detached, :614); padding 0
__global__ __launch_bounds__(256) void k_bosa_q_seed(const float* stats, long long N, float ng, int Np3, float* dz3) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * Np3) return;
  dz3[i] = i % Np3 == 0 ? -(1.f / (stats[0] / ng)) / ng : 0.f;
}
// the actor's seed: d(pre-tanh)[row][j] = (dq/da + dpi_extra) * max_action (1 - (pi / max_action)^2), padding 0; thread 0 also leaves
// the pair (sum -q_0, 0) that LossFinal kind 2 turns into -(1 / m) stats[1] / N_global
__global__ __launch_bounds__(256) void k_bosa_actor_seed(const float* dxa, const float* extra, const float* pi, const float* stats,
                                                         long long N, int A, int Np3, float max_action, float* dz3, float* lossp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) { lossp[0] = -stats[1]; lossp[1] = 0.f; }
  if (i >= N * Np3) return;
  const long long row = i / Np3;
  const int j = (int)(i - row * Np3);
  float v = 0.f;
  if (j < A) {
    const float y = pi[row * A + j] / max_action;
    v = (dxa[row * A + j] + extra[row * A + j]) * max_action * (1.f - y * y);
  }
  dz3[i] = v;
}

// expectile regression of V towards min target-Q (update_v_function, mobody.py:231-242; asymmetric_l2_loss :85-86):
// adv = min(Qt1,Qt2)(s,a) - V(s); L_V = mean(|0.7 - 1[adv<0]| * adv^2); dz3[row][0] = dL/dV
__global__ __launch_bounds__(256) void k_v_loss(const float* qt, const float* v, long long N, float invNg, int Np3,
                                                float* dz3, float* lossp) {
  __shared__ float sm[4];
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float l = 0.f;
  if (row < N) {
    const float adv = fminf(qt[row], qt[N + row]) - v[row];
    const float w = fabsf(0.7f - (adv < 0.f ? 1.f : 0.f));
    l = w * adv * adv;
    float* o = dz3 + row * Np3;
    o[0] = -2.f * w * adv * invNg;
    for (int c = 1; c < Np3; ++c) o[c] = 0.f;
  }
  l = block_sum(l, sm);
  if (threadIdx.x == 0) lossp[blockIdx.x] = l;
}
__global__ __launch_bounds__(256) void k_sum_scale(const float* parts, int n, float scale, float* out) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int k = threadIdx.x; k < n; k += blockDim.x) s += parts[k];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) out[0] = s * scale;
}

// ------------------------------------------------------------------------------------------------
// Adam + Polyak, transposes
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_adam(AdamTarget a, const float* g, long long n, MobodyMlpLayout L) {
  __shared__ float adam_sm[2];
  adam_block_consts(a, adam_sm);
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  // (tested on entry here, not in front of the stores as in the fused kernels: this launch is off the step's critical chain,
  //  and the early form keeps the kernel at 8 waves per SIMD -- 97 scalar registers against 103)
  if (j >= n || (health_mask(a) != 0 && health_foreign(a))) return;
  adam_element(a, L, j, g[j], adam_sm);
}

int launch_adam(const AdamTarget& a, const float* g, const MobodyMlpLayout& L, hipStream_t st) {
  hipLaunchKernelGGL(k_adam, dim3((unsigned)cdiv(L.total_floats, 256)), dim3(256), 0, st, a, g, (long long)L.total_floats, L);
  MB_LAUNCH_OK("k_adam");
  return 0;
}

// W1 and W2 (and W3T, W2T of the T blob) are 256 columns wide and stored K-interleaved (tile.h wide_idx);
// W3 and W1T are narrow and row major.
__global__ __launch_bounds__(256) void k_mlp_transpose(MobodyMlpLayout L, const float* blob, float* bt, int precision, int* health) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= L.t_total_floats) return;
  const int m = (int)(j / L.t_member_floats);
  const long long o = j - (long long)m * L.t_member_floats;
  const float* src = blob + (long long)m * L.member_floats;
  if (o >= L.w2p) {                                // bf16 planes of W2 / W2^T: one thread per float slot writes nothing here;
    if (o >= L.w2p + HID * HID) return;            // the first 65536 threads of the region each split one weight
    const int e = (int)(o - L.w2p), k = e / HID, n = e % HID;
    const float w = src[L.w2 + wide_idx(k, n)];
    write_w2_planes(bt + (long long)m * L.t_member_floats, L, k, n, w, precision);
    if (precision == 4) {                          // the unused third plane slot: defined contents (a rebuilt T blob compares equal)
      short* tm = reinterpret_cast<short*>(bt + (long long)m * L.t_member_floats);
      tm[2 * L.w2p + bf_plane_idx(2, k, n)] = 0; tm[2 * L.w2tp + bf_plane_idx(2, n, k)] = 0;
      health_check_f16(health, w);
    }
    return;
  }
  float val;
  if (o < L.w1t) {                               // wide regions of the T blob: decode (row kk, column c) of storage slot o
    const bool is3 = o < L.w2t;
    const long long oo = is3 ? o : o - L.w2t;
    const long long g = oo >> 2;
    const int kk = (int)(g / HID) * 4 + (int)(oo & 3), c = (int)(g % HID);
    // W3T[n3 = kk][k = c] = W3[k][n3] (narrow, row major);  W2T[n = kk][k = c] = W2[k][n] (wide)
    val = is3 ? src[L.w3 + (long long)c * L.Np3 + kk] : src[L.w2 + wide_idx(c, kk)];
  } else {                                       // W1T[n][k] = W1[k][n] (narrow [256][Np1t]), zero for k >= Kp1
    const long long oo = o - L.w1t;
    const int n = (int)(oo / L.Np1t), k = (int)(oo % L.Np1t);
    val = k < L.Kp1 ? src[L.w1 + wide_idx(k, n)] : 0.f;
  }
  bt[j] = val;
}

// ------------------------------------------------------------------------------------------------
// helpers to launch the fused MLP pieces on a packed blob
// ------------------------------------------------------------------------------------------------
// blob_T != null: the split-precision modes stream W2's planes from the T blob.  e1 != null (f16 mode): sh1 receives the
// layer-1 activations as fp16 planes + tile exponents instead of fp32 rows.  s1 == null: one input.
static Mlp3FwdArgs fwd_args(const float* blob, const MobodyMlpLayout& L, const float* s0, int n0, const float* s1, int n1,
                            long long rows, float* out, int out_mode, float max_action, float* sx, float* sh1,
                            float* sh2, uint32_t* m1 = nullptr, uint32_t* m2 = nullptr, const float* blob_T = nullptr,
                            int* e1 = nullptr) {
  Mlp3FwdArgs a = fwd_net(blob, L, rows);
  if (blob_T != nullptr) fwd_set_planes(a, blob_T, L);
  fwd_set_src(a, 0, s0, n0, n0);
  fwd_set_src(a, 1, s1, n1, s1 ? n1 : 0);
  fwd_set_out(a, out, out_mode, max_action);
  fwd_set_saves(a, sx, 0, sh1, e1, sh2, m1, m2);
  return a;
}

// weight gradients of one packed MLP: one merged split-K launch + the deterministic reduction.  The critic (two members) and the
// actor (one) take turns on the same dz2 / dz1 / dbp / slabs.
static int weight_grads(const MobodyMlpLayout& L, const float* x, const float* h1, const float* h2, const int* e_h1, const float* dz3,
                        long long rows, const TrainWs& w, float* grad, const LossFinal& loss, const AdamTarget& adam, int prec,
                        hipStream_t st) {
  const bool actor = L.members == 1;
  Mlp3WgradArgs g = wgrad_net(L, rows, actor ? w.nsplit_a : w.nsplit_q);
  wgrad_set_saves(g, x, 0, h1, h2, e_h1);
  wgrad_set_grads(g, dz3, w.dz2, w.dz1, w.dbp, w.ntiles, w.edz2);
  wgrad_set_scratch(g, w.slabs, w.bc + (actor ? 2 : 0));
  wgrad_set_result(g, grad, loss, adam, prec);
  return mlp3_weight_grads(g, st);
}

// the train step's ReLU nets: always the W2^T planes and `prec`; e2 != null in the f16 mode: dz2 receives fp16 planes + tile
// exponents instead of fp32 rows
static Mlp3BwdArgs bwd_args(const MobodyMlpLayout& L, const float* blob_T, const float* dz3, const float* h1,
                            const float* h2, long long rows, float* dz2, float* dz1, float* dbp,
                            const uint32_t* m1 = nullptr, const uint32_t* m2 = nullptr, int prec = PREC_F32, int* e2 = nullptr) {
  Mlp3BwdArgs b = bwd_net(L, blob_T, rows);
  bwd_set_planes(b, L, prec);
  bwd_set_acts(b, h1, h2, m1, m2, 0);
  bwd_set_grads(b, dz3, dz2, dz1, dbp, prec == PREC_F16X2 ? e2 : nullptr);
  return b;
}

}  // namespace mobody

using namespace mobody;

// exponent scale of TD3_BC's BC weight exp(1 * q / mean|q|) (td3_bc.py:167; MOBODY's bc_weight has 3)
static constexpr float TD3BC_EXP_SCALE = 1.f;

extern "C" int64_t mobody_train_workspace(const MobodyTrainDims* d) {
  if (check_dims(d, "mobody_train_workspace")) return -1;
  TrainWs w;
  if (carve(*d, nullptr, w)) return -1;
  return w.total;
}

// extra (with q_next, or null): a one-member forward that shares the launch of Q(s, a) -- IQL's V(s'), which writes q_next.
// row_weight (or null): IGDF's per-row weights of the loss (seed mode 8, train.h)
// cons (or null; needs row_weight): BOSA's conservative term (seed mode 9): the per-row constants of the seed, and what turns the
// second partial sum into loss_out -- loss_out[0] = sum w (q_m - y)^2 / N_global + coef * loss_out[1], loss_out[1] = sum_{c != 0} q_m /
// rows.  The fused form then steps the critic without touching its target (BOSA's Polyak update waits for the delayed actor step).
struct ConsTerm { const float* c; float coef, rows; };
static int critic_impl(const MobodyCritic& a, const FwdGather* gather, void* stream, const char* who = "mobody_critic",
                       const Mlp3FwdArgs* extra = nullptr, const float* row_weight = nullptr, const ConsTerm* cons = nullptr) {
  // gather != null (phase 0, q_next == null): state .. not_done are not read by the first forward launch but WRITTEN by it --
  // its tiles draw and fetch the minibatch rows themselves (layers.h FwdGather; the block arrives with `g` filled)
  // phase: 0 the whole step; 1 only its forwards (nothing of them reads `reward`); 2 only the backward, weight gradients and
  // reduction / optimizer step -- the caller may let another stream finish rewriting `reward` (penalty_type 'par': an ensemble
  // step on the source rows) between the two
  const MobodyTrainDims* d = &a.d;
  const MobodyHyper* h = &a.h;
  const bool fused = a.m != nullptr;
  int rc = check_dims(d, who);
  if (rc) return rc;
  MB_REQUIRE(a.q_blob && a.q_blob_T && a.state && a.action && a.reward && a.not_done && a.loss_out && a.workspace, "%s: null pointer", who);
  MB_REQUIRE(a.q_next || (a.actor_blob && a.qtarg_blob && a.next_state), "%s: need q_next or actor/target/next_state", who);
  rc = check_precision(who, h->precision, a.q_next != nullptr || (a.actor_blob_T && a.qtarg_blob_T));
  if (rc) return rc;
  if (fused) {
    MB_REQUIRE(a.qtarg_blob || cons != nullptr, "%s: null pointer", who);
    MB_REQUIRE(a.t_dev != nullptr || a.t >= 1, "%s: step t must be >= 1", who);
    MB_REQUIRE(a.bump == nullptr || a.bump != a.t_dev, "%s: bump must not be the step word the launch reads", who);
  } else {
    MB_REQUIRE(a.bump == nullptr, "%s: bump is incremented by the optimizer launch: it needs m, v", who);
  }
  TrainWs w;
  rc = carve(*d, a.workspace, w);
  if (rc) return rc;
  AdamTarget adam{};
  if (fused) {
    if (cons != nullptr) {
      adam = adam_target(a.q_blob, a.q_blob_T, a.m, a.v, nullptr, a.t, a.t_dev, a.lr, -1.f, 1.f, h->precision);
    } else {
      adam = adam_target(a.q_blob, a.q_blob_T, a.m, a.v, a.qtarg_blob, a.t, a.t_dev, a.lr, h->tau, 1.f, h->precision);
      adam.target_T = a.qtarg_blob_T;
    }
    adam.bump = (long long*)a.bump;
  }
  const float *q_blob = a.q_blob, *state = a.state, *action = a.action, *next_state = a.next_state, *q_next = a.q_next;
  const int prec = h->precision;
  const float *aT = prec != PREC_F32 ? a.actor_blob_T : nullptr, *qT = prec != PREC_F32 ? a.q_blob_T : nullptr, *tT = prec != PREC_F32 ? a.qtarg_blob_T : nullptr;
  hipStream_t st = as_stream(stream);
  const long long N = d->N;
  const int S = d->S, A = d->A;
  // online twin-Q(s, a), activations kept for the backward (:196), together with a' = pi(s') (:191) in one launch
  const Mlp3FwdArgs fq = fwd_args(q_blob, w.Lq, state, S, action, A, N, w.q, 0, 1.f, w.xq, w.h1q, w.h2q, w.mq1, w.mq2, qT,
                                  prec == PREC_F16X2 ? w.eh1q : nullptr);
  const float invNg = 1.f / (float)d->N_global;
  // TD error -> dz3 in the backward's prologue (mobody.py:190-207), then dz2, dz1 and the bias partials
  Mlp3BwdArgs bq = bwd_args(w.Lq, a.q_blob_T, w.dz3q, w.h1q, w.h2q, N, w.dz2, w.dz1, w.dbp, w.mq1, w.mq2, prec, w.edz2);
  bq.seed.mode = 1; bq.seed.q = w.q; bq.seed.qt = w.qt; bq.seed.qnext = q_next; bq.seed.r = a.reward; bq.seed.nd = a.not_done;
  bq.seed.gamma = h->gamma; bq.seed.inv_ng = invNg; bq.seed.dz3_out = w.dz3q; bq.seed.lossp = w.lossp;
  // the plain seed (mode 1) of a whole step: the merged forward launch runs the backward tiles too where it can (critic_fwd_bf.hip)
  const bool may_chain = a.phase == 0 && row_weight == nullptr && cons == nullptr;
  bool chained = false;
  if (a.phase == 2) {
    // forwards already enqueued by the phase-1 call
  } else if (q_next == nullptr) {
    const Mlp3FwdArgs fpn = fwd_args(a.actor_blob, w.La, next_state, S, nullptr, 0, N, w.pin, 1, h->max_action, nullptr, nullptr, nullptr, nullptr, nullptr, aT);
    // target twin-Q(s', a') (:192) -- and, when the caller asks for it, pi(s) of the coming actor phase in the same
    // launch: the actor is not updated in between, and a twin-Q launch alone is 2.5 workgroups per CU where the
    // merged one is 3.75 (the actor phase then opens with Q(s_t,a_t) alone: exactly 2 per CU)
    const Mlp3FwdArgs ft = fwd_args(a.qtarg_blob, w.Lq, next_state, S, w.pin, A, N, w.qt, 0, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, tT);
    Mlp3FwdArgs fpi{};
    if (a.policy_forward)
      fpi = fwd_args(a.actor_blob, w.La, state, S, nullptr, 0, N, w.pi, 1, h->max_action, w.xa, w.h1a, w.h2a, w.ma1, w.ma2, aT,
                     prec == PREC_F16X2 ? w.eh1a : nullptr);
    if (gather != nullptr) {
      // all of them in one launch where target-Q's workgroups can evaluate pi(s') of their own rows (layers.h)
      FwdGather fg = *gather;
      fwd_set_gather(fg, 0, fq, 0);                // state | action open the ring row, next_state follows them
      fwd_set_gather(fg, 1, fpn, S + A);
      rc = launch_critic_forward_gather(fq, fpn, ft, a.policy_forward ? &fpi : nullptr, fg, prec, st, may_chain ? &bq : nullptr, w.ctickets, &chained);
    } else {
      rc = launch_mlp3_forward(fq, 2, fpn, 1, ACT_RELU, prec, st);
      if (!rc && a.policy_forward) rc = launch_mlp3_forward(ft, 2, fpi, 1, ACT_RELU, prec, st);
      else if (!rc) rc = launch_mlp3_forward(ft, 2, ACT_RELU, prec, st);
    }
  } else {
    // q_next = V(s') supplied by the caller (update_q_functions_1, :210-229), or evaluated beside Q(s, a) (`extra`)
    rc = extra != nullptr ? launch_mlp3_forward(fq, 2, *extra, 1, ACT_RELU, prec, st) : launch_mlp3_forward(fq, 2, ACT_RELU, prec, st);
  }
  if (rc || a.phase == 1) return rc;
  if (cons != nullptr) {                           // BOSA: weight and constant (mode 9); its partial sums are pairs, 4 per row tile
    bq.seed.mode = 9; bq.seed.cs.w = row_weight; bq.seed.cs.c = cons->c;
    bq.seed.lossp = w.lossp_pairs;
    rc = launch_mlp3_bwd_ccritic(bq, st);
    if (rc) return rc;
    LossFinal lc{};                                // kind 2 without the q scale: out[0] = s0 / ng + bc_coef * out[1], out[1] = s1 / ntg_a
    lc.kind = 2; lc.nparts = 2 * w.ntiles; lc.scale_q = 0; lc.bc_coef = cons->coef; lc.ng = (float)d->N_global; lc.ntg_a = cons->rows;
    lc.parts = w.lossp_pairs; lc.out = a.loss_out;
    return weight_grads(w.Lq, w.xq, w.h1q, w.h2q, w.eh1q, w.dz3q, N, w, a.grad_q, lc, adam, prec, st);
  } else if (row_weight != nullptr) {              // IGDF: the same seed with the row's weight, an instance of its own (mode 8)
    bq.seed.mode = 8; bq.seed.cw.w = row_weight;
    rc = launch_mlp3_bwd_wcritic(bq, st);
  } else if (!chained) {
    rc = launch_mlp3_bwd(bq, 2, false, st);
  }
  if (rc) return rc;
  LossFinal lf{};                                  // q_loss = mse(q1,y)+mse(q2,y), local share of the global mean
  lf.kind = 1; lf.nparts = 2 * w.ntiles; lf.scale = invNg; lf.parts = w.lossp; lf.out = a.loss_out;
  return weight_grads(w.Lq, w.xq, w.h1q, w.h2q, w.eh1q, w.dz3q, N, w, a.grad_q, lf, adam, prec, st);
}

extern "C" int mobody_critic(const MobodyCritic* a, void* stream) {
  const char* who = "mobody_critic";
  MB_BLOCK(who, a, MobodyCritic);
  MB_REQUIRE((a->grad_q != nullptr) != (a->m != nullptr || a->v != nullptr), "%s: exactly one of grad_q and the optimizer state m, v must be given", who);
  MB_REQUIRE(a->grad_q || (a->m && a->v), "%s: null pointer", who);
  MB_REQUIRE(a->phase >= 0 && a->phase <= 2, "%s: phase is 0 (the whole step), 1 (forwards) or 2 (backward + update)", who);
  if (a->gather == nullptr) return critic_impl(*a, nullptr, stream);
  const MobodyGatherRng* gr = a->gather;
  MB_REQUIRE(a->phase == 0, "%s: the step cannot be split (phase %d): the first forward launch writes the minibatch the backward reads", who, a->phase);
  MB_REQUIRE(a->q_next == nullptr, "%s: q_next given: the launch that gathers is the one that evaluates pi(s')", who);
  FwdGather fg{};
  long long N;
  int rc = gather_args_rng(who, fg.g, gr->bufs, gr->counts, gr->nbuf, a->d.S, a->d.A, gr->seeds, gr->call_offsets, gr->counter, gr->sizes,
                           a->state, a->action, a->next_state, a->reward, a->not_done, gr->bump, gr->nbump, N);
  if (rc) return rc;
  MB_REQUIRE(N == a->d.N, "%s: the counts add up to %lld rows, the step runs on %lld", who, N, (long long)a->d.N);
  for (int k = 0; k < gr->nbuf; ++k)
    MB_REQUIRE(gr->counts[k] == 0 || fg.g.packed[k], "%s: source %d is not a row-interleaved ring (mobody_ring_pitch)", who, k);
  return critic_impl(*a, &fg, stream);
}

// BOSA's critic update (bosa.py:580-607) on bootstrap values the caller supplies: Q(s, a) with saves, seed mode 9, the
// weight gradients with the optimizer step fused -- and no Polyak update
extern "C" int mobody_bosa_critic(const MobodyCritic* a, const float* row_weight, const float* row_const, float cons_coef,
                                  int64_t cons_rows_global, void* stream) {
  const char* who = "mobody_bosa_critic";
  MB_BLOCK(who, a, MobodyCritic);
  MB_REQUIRE((a->grad_q != nullptr) != (a->m != nullptr || a->v != nullptr), "%s: exactly one of grad_q and the optimizer state m, v must be given", who);
  MB_REQUIRE(a->grad_q || (a->m && a->v), "%s: null pointer", who);
  MB_REQUIRE(a->phase == 0 && a->gather == nullptr && a->policy_forward == 0, "%s: phase, gather and policy_forward must be 0 / NULL", who);
  MB_REQUIRE(a->q_next != nullptr, "%s: q_next is NULL: the caller supplies min target-Q(s', a') with its clipped target noise", who);
  MB_REQUIRE(row_weight != nullptr && row_const != nullptr, "%s: row_weight / row_const is NULL", who);
  MB_REQUIRE(cons_rows_global >= 1, "%s: cons_rows_global %lld < 1", who, (long long)cons_rows_global);
  const ConsTerm cons{row_const, cons_coef, (float)cons_rows_global};
  return critic_impl(*a, nullptr, stream, who, nullptr, row_weight, &cons);
}

// td3bc: the TD3_BC form (the entry point has checked Nt == N, no v_true, scale_q) -- no Q(s_t, a_t) forward and no second statistic
static int actor_forward_impl(const MobodyActor* a, void* stream, const char* who, bool td3bc) {
  const MobodyTrainDims* d = &a->d;
  const MobodyHyper* h = &a->h;
  int rc = check_dims(d, who);
  if (rc) return rc;
  MB_REQUIRE(a->actor_blob && a->q_blob && a->state && a->action && a->stats && a->workspace, "%s: null pointer", who);
  rc = check_precision(who, h->precision, a->actor_blob_T && a->q_blob_T);
  if (rc) return rc;
  const int prec = h->precision;
  const float *aT = prec != PREC_F32 ? a->actor_blob_T : nullptr, *qT = prec != PREC_F32 ? a->q_blob_T : nullptr;
  const float *q_blob = a->q_blob, *state = a->state;
  TrainWs w;
  rc = carve(*d, a->workspace, w);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const long long N = d->N, Nt = td3bc ? 0 : d->Nt;
  const int S = d->S, A = d->A;
  // Q(s_true, a_true) for the BC weights (:251) and pi(s) on the whole mixed batch (its first Nt rows are
  // pi(s_true), mobody.py:249,315) in one launch -- unless the critic call already left pi(s) in the workspace
  const Mlp3FwdArgs fb = fwd_args(q_blob, w.Lq, state, S, a->action, A, Nt, w.qb, 0, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, qT);
  // Q(s, pi(s)) with the freshly updated critic (:316); dQ/da through the frozen net needs only the ReLU signs
  const Mlp3FwdArgs fp = fwd_args(q_blob, w.Lq, state, S, w.pi, A, N, w.q, 0, 1.f, nullptr, nullptr, nullptr, w.mq1, w.mq2, qT);
  const auto policy = [&] {
    return fwd_args(a->actor_blob, w.La, state, S, nullptr, 0, N, w.pi, 1, h->max_action, w.xa, w.h1a, w.h2a, w.ma1, w.ma2, aT,
                    prec == PREC_F16X2 ? w.eh1a : nullptr);
  };
  if (td3bc) {                                      // TD3_BC (td3_bc.py:161-163): pi(s), then Q(s, pi(s)) alone
    if (!a->policy_ready) rc = launch_mlp3_forward(policy(), 1, ACT_RELU, prec, st);
    if (!rc) rc = launch_mlp3_forward(fp, 2, ACT_RELU, prec, st);
  } else if (a->policy_ready) {
    rc = launch_mlp3_forward(fb, 2, fp, 2, ACT_RELU, prec, st);                 // both on the same critic: one launch of N + Nt rows (0.384 -> 0.380 ms/step)
  } else {
    rc = launch_mlp3_forward(fb, 2, policy(), 1, ACT_RELU, prec, st);
    if (!rc) rc = launch_mlp3_forward(fp, 2, ACT_RELU, prec, st);
  }
  if (rc) return rc;
  // (Nt = 0: stats[1] = 0 and qb is not read)
  hipLaunchKernelGGL(k_actor_stats, dim3(1), dim3(1024), 0, st, w.q, w.qb, N, Nt, a->stats, w.tickets, w.ntiles);
  MB_LAUNCH_OK("k_actor_stats");
  return 0;
}

extern "C" int mobody_actor_forward(const MobodyActor* a, void* stream) {
  const char* who = "mobody_actor_forward";
  MB_BLOCK(who, a, MobodyActor);
  return actor_forward_impl(a, stream, who, false);
}

// td3bc: the TD3_BC form (seed mode 4 in the frozen-Q tile; the entry point has checked Nt == N, no v_true, scale_q)
static int actor_backward_impl(const MobodyActor& a, void* stream, const char* who = "mobody_actor_backward", bool td3bc = false) {
  const MobodyTrainDims* d = &a.d;
  const MobodyHyper* h = &a.h;
  const bool fused = a.m != nullptr;
  int rc = check_dims(d, who);
  if (rc) return rc;
  MB_REQUIRE(a.actor_blob && a.actor_blob_T && a.q_blob && a.q_blob_T && a.state && a.action && a.stats && a.loss_out && a.workspace,
             "%s: null pointer", who);
  rc = check_precision(who, h->precision, true);
  if (rc) return rc;
  MB_REQUIRE(!fused || a.t_dev != nullptr || a.t >= 1, "%s: step t must be >= 1", who);
  TrainWs w;
  rc = carve(*d, a.workspace, w);
  if (rc) return rc;
  const AdamTarget adam = fused ? adam_target(a.actor_blob, a.actor_blob_T, a.m, a.v, nullptr, a.t, a.t_dev, a.lr, -1.f, 1.f, h->precision) : AdamTarget{};
  hipStream_t st = as_stream(stream);
  const long long N = d->N;
  ActorRowArgs ra{};
  ra.qp = w.q; ra.qb = w.qb; ra.stats = a.stats; ra.pi = w.pi; ra.act = a.action; ra.dxa = w.dxa; ra.v_true = a.v_true;
  ra.bcw = w.bcw; ra.N = N; ra.Nt = d->Nt; ra.Ng = d->N_global; ra.Ntg = d->Nt_global > 0 ? d->Nt_global : 1;
  ra.A = d->A; ra.h = *h;
  // dq -> d(action) through the frozen twin-Q (parameters get no gradient, mobody.py:555-556); the prologue forms
  // -p_w/N d min(q1,q2) and the BC weights
  Mlp3BwdArgs bq = bwd_args(w.Lq, a.q_blob_T, nullptr, nullptr, nullptr, N, nullptr, nullptr, w.dbp, w.mq1, w.mq2, h->precision);
  bq.seed.mode = td3bc ? 4 : 2; bq.seed.ar = ra;
  if (td3bc) bq.seed.exp_scale = TD3BC_EXP_SCALE;
  bq.dx = w.dxa; bq.dx_c0 = d->S; bq.dx_n = d->A;
  // actor: d(pre-tanh) from both members' dx and the BC term in the prologue, then the actor's own backward -- in the same
  // launch: a tile's actor backward runs in the second of the tile's two frozen-Q workgroups to finish
  Mlp3BwdArgs ba = bwd_args(w.La, a.actor_blob_T, w.dz3a, w.h1a, w.h2a, N, w.dz2, w.dz1, w.dbp, w.ma1, w.ma2, h->precision, w.edz2);
  ba.seed.mode = 3; ba.seed.ar = ra; ba.seed.dz3_out = w.dz3a; ba.seed.lossp = w.lossp;
  rc = launch_actor_bwd_chain(bq, ba, w.tickets, st);
  if (rc) return rc;
  LossFinal lf{};                                  // loss_out[0] = p_w*mean(-q) + bc_coef*L_BC, [1] = L_BC (local shares)
  lf.kind = 2; lf.nparts = w.ntiles; lf.scale_q = h->scale_q; lf.weight = h->weight; lf.bc_coef = h->bc_coef;
  lf.ng = (float)ra.Ng; lf.ntg_a = (float)ra.Ntg * (float)ra.A; lf.parts = w.lossp; lf.stats = a.stats; lf.out = a.loss_out;
  return weight_grads(w.La, w.xa, w.h1a, w.h2a, w.eh1a, w.dz3a, N, w, a.grad_actor, lf, adam, h->precision, st);
}

extern "C" int mobody_actor_backward(const MobodyActor* a, void* stream) {
  const char* who = "mobody_actor_backward";
  MB_BLOCK(who, a, MobodyActor);
  MB_REQUIRE((a->grad_actor != nullptr) != (a->m != nullptr || a->v != nullptr), "%s: exactly one of grad_actor and the optimizer state m, v must be given", who);
  MB_REQUIRE(a->grad_actor || (a->m && a->v), "%s: null pointer", who);
  return actor_backward_impl(*a, stream);
}

// ---- TD3_BC actor phase (td3_bc.py:160-176): BC on every row, weighted by min(exp(1 * q/mean|q|), 100) of the SAME Q the policy
// term uses, with the gradient through the weight.  One Q forward fewer than MOBODY's actor phase (no Q(s_t, a_t)). ----
static int td3bc_check(const MobodyActor* a, const char* who) {
  MB_BLOCK(who, a, MobodyActor);
  MB_REQUIRE(a->d.Nt == a->d.N, "%s: d.Nt %lld != d.N %lld (the BC term runs on every row)", who, (long long)a->d.Nt, (long long)a->d.N);
  MB_REQUIRE(a->d.Nt_global == a->d.N_global, "%s: d.Nt_global %lld != d.N_global %lld", who, (long long)a->d.Nt_global, (long long)a->d.N_global);
  MB_REQUIRE(a->v_true == nullptr, "%s: v_true given: the weight is exp(q/mean|q|) of Q(s, pi(s)), there is no V function", who);
  MB_REQUIRE(a->h.scale_q == 1, "%s: h.scale_q %d != 1 (the policy term is always weight / mean|Q|)", who, a->h.scale_q);
  MB_REQUIRE(a->d.A <= 24, "%s: d.A %d > 24", who, a->d.A);
  return 0;
}

extern "C" int mobody_td3bc_actor_forward(const MobodyActor* a, void* stream) {
  const char* who = "mobody_td3bc_actor_forward";
  int rc = td3bc_check(a, who);
  return rc ? rc : actor_forward_impl(a, stream, who, true);
}

extern "C" int mobody_td3bc_actor_backward(const MobodyActor* a, void* stream) {
  const char* who = "mobody_td3bc_actor_backward";
  int rc = td3bc_check(a, who);
  if (rc) return rc;
  MB_REQUIRE((a->grad_actor != nullptr) != (a->m != nullptr || a->v != nullptr), "%s: exactly one of grad_actor and the optimizer state m, v must be given", who);
  MB_REQUIRE(a->grad_actor || (a->m && a->v), "%s: null pointer", who);
  return actor_backward_impl(*a, stream, who, true);
}

// ---- BOSA's actor phase (bosa.py:612-629): Q = critic_1 (member 0) alone, and the estimator's term arrives as a
// per-element addend dpi_extra.  Existing launches in seed mode 0 -- dz3 read from memory -- between three row-wise kernels; each
// launch reads what the one before it on the stream wrote, nothing waits inside a kernel. ----
static constexpr unsigned BOSA_ACTOR_PREC = 1u << PREC_F32 | 1u << PREC_BF16X3 | 1u << PREC_F16X2;
static int bosa_actor_check(const MobodyActor* a, const char* who) {
  MB_BLOCK(who, a, MobodyActor);
  int rc = check_dims(&a->d, who);
  if (rc) return rc;
  MB_REQUIRE(a->d.N <= (1 << 21), "%s: d.N %lld > 2^21", who, (long long)a->d.N);
  MB_REQUIRE(a->v_true == nullptr, "%s: v_true given: there is no V function", who);
  MB_REQUIRE(a->policy_ready == 0, "%s: policy_ready %d: pi(s) is evaluated here", who, a->policy_ready);
  return check_precision(who, a->h.precision, a->actor_blob_T && a->q_blob_T, BOSA_ACTOR_PREC);
}

extern "C" int mobody_bosa_actor_forward(const MobodyActor* a, float* pi_out, void* stream) {
  const char* who = "mobody_bosa_actor_forward";
  int rc = bosa_actor_check(a, who);
  if (rc) return rc;
  MB_REQUIRE(a->actor_blob && a->q_blob && a->state && a->stats && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(pi_out != nullptr, "%s: pi_out is NULL", who);
  const MobodyTrainDims* d = &a->d;
  const MobodyHyper* h = &a->h;
  const int prec = h->precision;
  const float *aT = prec != PREC_F32 ? a->actor_blob_T : nullptr, *qT = prec != PREC_F32 ? a->q_blob_T : nullptr;
  TrainWs w;
  rc = carve(*d, a->workspace, w);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const long long N = d->N;
  const int S = d->S, A = d->A;
  const Mlp3FwdArgs fpi = fwd_args(a->actor_blob, w.La, a->state, S, nullptr, 0, N, w.pi, 1, h->max_action, w.xa, w.h1a, w.h2a, w.ma1, w.ma2, aT,
                                   prec == PREC_F16X2 ? w.eh1a : nullptr);
  // member 0 of the twin-Q blob: a one-member launch; dQ/da through the frozen net needs only the ReLU signs
  const Mlp3FwdArgs fq = fwd_args(a->q_blob, w.Lq, a->state, S, w.pi, A, N, w.q, 0, 1.f, nullptr, nullptr, nullptr, w.mq1, w.mq2, qT);
  rc = launch_mlp3_forward(fpi, 1, ACT_RELU, prec, st);
  if (!rc) rc = launch_mlp3_forward(fq, 1, ACT_RELU, prec, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bosa_actor_stats, dim3(1), dim3(1024), 0, st, (const float*)w.q, N, a->stats);
  MB_LAUNCH_OK("k_bosa_actor_stats");
  const hipError_t e = hipMemcpyAsync(pi_out, w.pi, sizeof(float) * N * A, hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return fail(MOBODY_E_LAUNCH, "%s: hipMemcpyAsync: %s", who, hipGetErrorString(e));
  return 0;
}

extern "C" int mobody_bosa_actor_backward(const MobodyActor* a, const float* dpi_extra, void* stream) {
  const char* who = "mobody_bosa_actor_backward";
  int rc = bosa_actor_check(a, who);
  if (rc) return rc;
  MB_REQUIRE((a->grad_actor != nullptr) != (a->m != nullptr || a->v != nullptr), "%s: exactly one of grad_actor and the optimizer state m, v must be given", who);
  MB_REQUIRE(a->grad_actor || (a->m && a->v), "%s: null pointer", who);
  MB_REQUIRE(a->actor_blob && a->actor_blob_T && a->q_blob && a->q_blob_T && a->state && a->stats && a->loss_out && a->workspace, "%s: null pointer", who);
  MB_REQUIRE(dpi_extra != nullptr, "%s: dpi_extra is NULL", who);
  const bool fused = a->m != nullptr;
  MB_REQUIRE(!fused || a->t_dev != nullptr || a->t >= 1, "%s: step t must be >= 1", who);
  const MobodyTrainDims* d = &a->d;
  const MobodyHyper* h = &a->h;
  const int prec = h->precision;
  TrainWs w;
  rc = carve(*d, a->workspace, w);
  if (rc) return rc;
  const AdamTarget adam = fused ? adam_target(a->actor_blob, a->actor_blob_T, a->m, a->v, nullptr, a->t, a->t_dev, a->lr, -1.f, 1.f, prec) : AdamTarget{};
  hipStream_t st = as_stream(stream);
  const long long N = d->N;
  const float ng = (float)d->N_global;
  hipLaunchKernelGGL(k_bosa_q_seed, dim3((unsigned)cdiv(N * w.Lq.Np3, 256)), dim3(256), 0, st, (const float*)a->stats, N, ng, w.Lq.Np3, w.dz3q);
  MB_LAUNCH_OK("k_bosa_q_seed");
  // dq_0/da through the frozen critic_1 (its parameters take no gradient): member 0 alone, sign words, no dz2 / dz1
  Mlp3BwdArgs bq = bwd_args(w.Lq, a->q_blob_T, w.dz3q, nullptr, nullptr, N, nullptr, nullptr, w.dbp, w.mq1, w.mq2, prec);
  bq.dx = w.dxa; bq.dx_c0 = d->S; bq.dx_n = d->A;
  if ((rc = launch_mlp3_bwd(bq, 1, true, st))) return rc;
  hipLaunchKernelGGL(k_bosa_actor_seed, dim3((unsigned)cdiv(N * w.La.Np3, 256)), dim3(256), 0, st, (const float*)w.dxa, dpi_extra, (const float*)w.pi,
                     (const float*)a->stats, N, d->A, w.La.Np3, h->max_action, w.dz3a, w.lossp);
  MB_LAUNCH_OK("k_bosa_actor_seed");
  const Mlp3BwdArgs ba = bwd_args(w.La, a->actor_blob_T, w.dz3a, w.h1a, w.h2a, N, w.dz2, w.dz1, w.dbp, w.ma1, w.ma2, prec, w.edz2);
  if ((rc = launch_mlp3_bwd(ba, 1, false, st))) return rc;
  LossFinal lf{};                                  // kind 2 on one pair: loss_out[0] = (1 / m) (-stats[1]) / N_global, loss_out[1] = 0
  lf.kind = 2; lf.nparts = 1; lf.scale_q = 1; lf.weight = 1.f; lf.bc_coef = 0.f; lf.ng = ng; lf.ntg_a = 1.f;
  lf.parts = w.lossp; lf.stats = a->stats; lf.out = a->loss_out;
  return weight_grads(w.La, w.xa, w.h1a, w.h2a, w.eh1a, w.dz3a, N, w, a->grad_actor, lf, adam, prec, st);
}

// ---- IQL (the reference's algo/offline_offline/iql.py): V with the expectile seed, twin-Q against V(s') through critic_impl, the
// policy with the advantage-weighted regression seed and a cosine learning rate.  DESIGN 5r. ----
namespace mobody {
// training scratch of one single-member net on `rows` rows: IQL's V and policy, DARA's heads, IGDF's encoders
struct OneNetScratch {
  float *out, *x, *h1, *h2, *dz3, *dz2, *dz1, *dbp, *slabs, *lossp, *bc;
  uint32_t *m1, *m2;
  int *e_h1, *e_dz2;
  int nsplit, ntiles;
};

// where one net's gradient goes: into `grad` (the gradient form), or through Adam on m, v at step t / t_dev[0] and rate lr (fused)
struct NetOpt { float *grad, *m, *v; int64_t t; const int64_t* t_dev; float lr; };

// One trained net: its layout, scratch, rows, weights and MFMA mode, bound once.  The three steps every net of the family takes
// are written here and nowhere else; what differs between the algorithms -- sources, loss seed, loss wiring -- stays with the caller.
struct TrainedNet {
  const MobodyMlpLayout& L; const OneNetScratch& s; long long rows; float *blob, *blob_T; int prec;
  // the forward on one or two sources, linear outputs to s.out, with the saves of the backward
  Mlp3FwdArgs forward(const float* s0, int n0, const float* s1 = nullptr, int n1 = 0) const {
    return fwd_args(blob, L, s0, n0, s1, n1, rows, s.out, 0, 1.f, s.x, s.h1, s.h2, s.m1, s.m2, prec != PREC_F32 ? blob_T : nullptr,
                    prec == PREC_F16X2 ? s.e_h1 : nullptr);
  }
  // the backward from dz3 in memory; dz3 == null: from a loss seed in the prologue, which leaves dz3 and the loss partials in the
  // scratch -- the caller sets the seed's mode and the fields of that mode
  Mlp3BwdArgs backward(const float* dz3 = nullptr) const {
    Mlp3BwdArgs b = bwd_args(L, blob_T, dz3, s.h1, s.h2, rows, s.dz2, s.dz1, s.dbp, s.m1, s.m2, prec, s.e_dz2);
    if (dz3 == nullptr) { b.seed.dz3_out = s.dz3; b.seed.lossp = s.lossp; }
    return b;
  }
  // dW, db from what the forward and the backward left, the loss scalar out[0] = scale * sum(parts[0..nparts)) (out == null: none)
  // and, fused, the Adam step; bc_ready: the backward's seed has written the bias corrections; bump: AdamTarget::bump
  int finish(const NetOpt& o, const float* parts, int nparts, float scale, float* out, bool bc_ready, hipStream_t st,
             int64_t* bump = nullptr) const {
    AdamTarget adam = o.m ? adam_target(blob, blob_T, o.m, o.v, nullptr, o.t, o.t_dev, o.lr, -1.f, 1.f, prec) : AdamTarget{};
    if (o.m) adam.bump = (long long*)bump;
    LossFinal lf{};
    if (out != nullptr) { lf.kind = 1; lf.nparts = nparts; lf.scale = scale; lf.parts = parts; lf.out = out; }
    Mlp3WgradArgs g = wgrad_net(L, rows, s.nsplit);
    wgrad_set_saves(g, s.x, 0, s.h1, s.h2, s.e_h1);
    wgrad_set_grads(g, s.dz3, s.dz2, s.dz1, s.dbp, s.ntiles, s.e_dz2);
    wgrad_set_scratch(g, s.slabs, s.bc);
    wgrad_set_result(g, o.grad, lf, adam, prec);
    g.bc_ready = bc_ready ? 1 : 0;
    return mlp3_weight_grads(g, st);
  }
};

struct IqlWs {
  TrainWs tw;              // the critic's scratch, where mobody_critic carves it
  MobodyMlpLayout Lv, Lp;
  OneNetScratch v, p;
  float *qt, *vnext;       // target twin-Q(s, a) [2][N], V(s') [N]
  long long total;
};

// one net's scratch on N rows, nloss loss partials per row tile
static void carve_one_net(const MobodyMlpLayout& L, long long N, int nloss, OneNetScratch& n, Carver& take) {
  const long long N32 = (N + 31) & ~31LL, mw = cdiv(N, 32) * HID;
  n.ntiles = (int)cdiv(N, MLP_TILE_ROWS); n.nsplit = wgrad_nsplit(N, 1);
  n.out = take(N * L.out_dim); n.x = take(N * L.Kp1); n.h1 = take(N32 * HID); n.h2 = take(N * HID);
  n.m1 = (uint32_t*)take(mw); n.m2 = (uint32_t*)take(mw);
  n.e_h1 = (int*)take(N32 / 32); n.e_dz2 = (int*)take(N32 / 32);
  n.dz3 = take(N * L.Np3); n.dz2 = take(N32 * HID); n.dz1 = take(N * HID);
  n.dbp = take((long long)n.ntiles * (2 * HID + L.Np3));
  n.slabs = take(((L.total_floats + 3) & ~3LL) * n.nsplit);
  n.lossp = take((long long)nloss * n.ntiles); n.bc = take(4);
}

static int carve_iql(const MobodyTrainDims& d, float* base, IqlWs& w) {
  int rc = carve(d, base, w.tw);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S, 1, 1, &w.Lv);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S, 2 * d.A, 1, &w.Lp);
  if (rc) return rc;
  Carver take{base, w.tw.total};
  carve_one_net(w.Lv, d.N, 3, w.v, take);
  carve_one_net(w.Lp, d.N, 1, w.p, take);
  w.qt = take(2 * d.N); w.vnext = take(d.N);
  w.total = take.off;
  return 0;
}

// The size bounds the family's entry points and its *_workspace functions share.  s_in (1 or 2; 0: none): the algorithm's widest
// extra net reads s_in S + A input columns (IGDF's encoder_sa, DARA's sas head).
static int family_sizes(const char* who, const MobodyTrainDims* d, int s_in = 0) {
  int rc = check_dims(d, who);
  if (rc) return rc;
  MB_REQUIRE(d->S >= 1 && d->A >= 1 && 2 * d->A <= 128, "%s: d.A %d: the policy's 2 A outputs must fit 128 columns (2 A > 128)", who, d->A);
  MB_REQUIRE(s_in * d->S + d->A <= 256, "%s: %sS + A = %d > 256 (the widest input a packed MLP takes)", who, s_in == 2 ? "2 " : "",
             s_in * d->S + d->A);
  return 0;
}

// "exactly one of the gradient blobs and the optimizer state": one net, or two that one optimizer steps (one t, t_dev and lr).
// grads: the block's gradient field names; nets: " of both heads" and the like, or ""
static int check_opt(const char* who, const NetOpt* o, int n, const char* grads, const char* nets) {
  bool any_grad = false, all_grad = true, any_opt = false, all_opt = true;
  for (int k = 0; k < n; ++k) {
    any_grad |= o[k].grad != nullptr; all_grad &= o[k].grad != nullptr;
    any_opt |= o[k].m != nullptr || o[k].v != nullptr; all_opt &= o[k].m != nullptr && o[k].v != nullptr;
  }
  MB_REQUIRE(any_grad != any_opt, "%s: exactly one of %s and the optimizer state m, v%s must be given", who, grads, nets);
  MB_REQUIRE(all_grad || all_opt, "%s: null pointer", who);
  MB_REQUIRE(!any_opt || o[0].t_dev != nullptr || o[0].t >= 1, "%s: step t must be >= 1", who);
  return 0;
}

// what the three entry points check alike, before any runtime call
static int iql_check(const MobodyIql* a, const char* who) {
  MB_BLOCK(who, a, MobodyIql);
  int rc = family_sizes(who, &a->d);
  if (rc) return rc;
  MB_REQUIRE(a->lam > 0.f && a->lam < 1.f, "%s: lam %g outside (0, 1)", who, (double)a->lam);
  const NetOpt o{a->grad, a->m, a->v, a->t, a->t_dev, a->lr};
  rc = check_opt(who, &o, 1, "grad", "");
  if (rc) return rc;
  MB_REQUIRE(a->state && a->action && a->loss_out && a->workspace, "%s: null pointer", who);
  return check_precision(who, a->h.precision, true);
}
}  // namespace mobody

extern "C" int64_t mobody_iql_workspace(const MobodyTrainDims* d) {
  if (family_sizes("mobody_iql_workspace", d)) return -1;
  IqlWs w;
  if (carve_iql(*d, nullptr, w)) return -1;
  return w.total;
}

// iql.py:174-185 (update_v_function), :217-220
extern "C" int mobody_iql_value(const MobodyIql* a, void* stream) {
  const char* who = "mobody_iql_value";
  int rc = iql_check(a, who);
  if (rc) return rc;
  MB_REQUIRE(a->v_blob && a->v_blob_T && a->qtarg_blob && a->adv, "%s: null pointer", who);
  const int prec = a->h.precision;
  MB_REQUIRE(prec == PREC_F32 || a->qtarg_blob_T, "%s: the split-precision modes need qtarg_blob_T", who);
  IqlWs w;
  rc = carve_iql(a->d, a->workspace, w);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const long long N = a->d.N;
  const int S = a->d.S, A = a->d.A;
  const TrainedNet v{w.Lv, w.v, N, a->v_blob, a->v_blob_T, prec};
  // target twin-Q(s, a) (no grad, :175-177) and V(s) with its saves (:179) read the same rows: one launch
  const Mlp3FwdArgs ft = fwd_args(a->qtarg_blob, w.tw.Lq, a->state, S, a->action, A, N, w.qt, 0, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  prec != PREC_F32 ? a->qtarg_blob_T : nullptr);
  rc = launch_mlp3_forward(ft, 2, v.forward(a->state, S), 1, ACT_RELU, prec, st);
  if (rc) return rc;
  const float invNg = 1.f / (float)a->d.N_global;
  Mlp3BwdArgs b = v.backward();
  b.seed.mode = 5; b.seed.iq.qt = w.qt; b.seed.iq.v = w.v.out; b.seed.iq.adv_out = a->adv; b.seed.iq.lam = a->lam; b.seed.iq.inv = invNg;
  rc = launch_mlp3_bwd_seed(b, st);
  if (rc) return rc;
  rc = v.finish({a->grad, a->m, a->v, a->t, a->t_dev, a->lr}, w.v.lossp, w.v.ntiles, invNg, a->loss_out, false, st);
  if (rc || a->log_out == nullptr) return rc;
  // the logged scalars of a logging step (:181-183): two more partial sums of the seed prologue
  for (int k = 0; k < 2; ++k) {
    hipLaunchKernelGGL(k_sum_scale, dim3(1), dim3(256), 0, st, w.v.lossp + (long long)(k + 1) * w.v.ntiles, w.v.ntiles, invNg, a->log_out + k);
    MB_LAUNCH_OK("k_sum_scale");
  }
  return 0;
}

// iql.py:187-196 (update_q_functions), :222-228; row_weight: igdf.py:468-479
static int iql_critic_impl(const MobodyIql* a, const float* row_weight, void* stream, const char* who) {
  int rc = iql_check(a, who);
  if (rc) return rc;
  MB_REQUIRE(a->v_blob && a->v_blob_T && a->q_blob && a->q_blob_T && a->qtarg_blob && a->next_state && a->reward && a->not_done, "%s: null pointer", who);
  IqlWs w;
  rc = carve_iql(a->d, a->workspace, w);
  if (rc) return rc;
  const int prec = a->h.precision;
  MobodyCritic c{};
  c.struct_bytes = (int32_t)sizeof(MobodyCritic);
  c.d = a->d; c.h = a->h;
  c.q_blob = a->q_blob; c.q_blob_T = a->q_blob_T; c.qtarg_blob = a->qtarg_blob; c.qtarg_blob_T = a->qtarg_blob_T;
  c.state = const_cast<float*>(a->state); c.action = const_cast<float*>(a->action); c.next_state = const_cast<float*>(a->next_state);
  c.reward = const_cast<float*>(a->reward); c.not_done = const_cast<float*>(a->not_done);
  c.q_next = w.vnext; c.grad_q = a->grad; c.m = a->m; c.v = a->v; c.t = a->t; c.t_dev = a->t_dev; c.lr = a->lr;
  c.loss_out = a->loss_out; c.workspace = a->workspace; c.bump = a->bump;
  // V(s') with the V net mobody_iql_value has just updated (:189), beside Q(s, a)
  const Mlp3FwdArgs fvn = fwd_args(a->v_blob, w.Lv, a->next_state, a->d.S, nullptr, 0, a->d.N, w.vnext, 0, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   prec != PREC_F32 ? a->v_blob_T : nullptr);
  return critic_impl(c, nullptr, stream, who, &fvn, row_weight);
}

extern "C" int mobody_iql_critic(const MobodyIql* a, void* stream) { return iql_critic_impl(a, nullptr, stream, "mobody_iql_critic"); }

// iql.py:91-95 (bc_loss), :198-202 (update_policy), :233-237
extern "C" int mobody_iql_actor(const MobodyIql* a, void* stream) {
  const char* who = "mobody_iql_actor";
  int rc = iql_check(a, who);
  if (rc) return rc;
  MB_REQUIRE(a->T_max >= 1, "%s: T_max %lld < 1", who, (long long)a->T_max);
  MB_REQUIRE(a->pi_blob && a->pi_blob_T && a->adv, "%s: null pointer", who);
  IqlWs w;
  rc = carve_iql(a->d, a->workspace, w);
  if (rc) return rc;
  const int prec = a->h.precision;
  const bool fused = a->m != nullptr, dev = fused && a->t_dev != nullptr;
  // the step's learning rate: from the host count here, from the device count in the backward launch's first tile
  const float lr_k = dev || !fused ? a->lr : cosine_lr(a->lr, a->t, a->T_max);
  hipStream_t st = as_stream(stream);
  const int A = a->d.A;
  const TrainedNet pi{w.Lp, w.p, a->d.N, a->pi_blob, a->pi_blob_T, prec};
  // the linear 2 A outputs (mu | logstd, :92-93) with the saves of the backward
  rc = launch_mlp3_forward(pi.forward(a->state, a->d.S), 1, ACT_RELU, prec, st);
  if (rc) return rc;
  const float inv = 1.f / ((float)a->d.N_global * (float)A);
  Mlp3BwdArgs b = pi.backward();
  b.seed.mode = 6; b.seed.iq.z = w.p.out; b.seed.iq.ldz = 2 * A; b.seed.iq.act = a->action; b.seed.iq.adv = a->adv; b.seed.iq.A = A;
  b.seed.iq.temp = a->temp; b.seed.iq.inv = inv;
  if (dev) { b.seed.iq.bc_out = w.p.bc; b.seed.iq.t_dev = (const long long*)a->t_dev; b.seed.iq.T_max = a->T_max; b.seed.iq.lr0 = a->lr; }
  rc = launch_mlp3_bwd_seed(b, st);
  if (rc) return rc;
  return pi.finish({a->grad, a->m, a->v, a->t, a->t_dev, lr_k}, w.p.lossp, w.p.ntiles, inv, a->loss_out, dev, st);
}

// ---- DARA (the reference's algo/offline_offline/dara.py): IQL's step behind one domain-classifier update per step and a relabel
// of the source rewards with the classifier's log-ratio.  The two heads are one-member nets trained like V and the policy: paired
// forward, loss seed in the backward prologue (mode 7), weight gradients with the reduce and Adam fused.  DESIGN 5s. ----
namespace mobody {
struct DaraWs {
  IqlWs iq;                // IQL's scratch, where its three entry points carve it
  MobodyMlpLayout Lsa, Lsas;
  OneNetScratch sa, sas;
  float *xin_sa, *xin_sas; // noisy input rows [N][S+A], [N][2S+A] (the forward's sources; its save_x is the padded copy)
  float* delta;            // [N] per-row penalty when the caller keeps none
  long long total;
};

static int carve_dara(const MobodyTrainDims& d, float* base, DaraWs& w) {
  int rc = carve_iql(d, base, w.iq);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S + d.A, 2, 1, &w.Lsa);
  if (rc) return rc;
  rc = mobody_mlp_layout(2 * d.S + d.A, 2, 1, &w.Lsas);
  if (rc) return rc;
  const long long N = d.N;
  Carver take{base, w.iq.total};
  carve_one_net(w.Lsa, N, 1, w.sa, take);
  carve_one_net(w.Lsas, N, 1, w.sas, take);
  w.xin_sa = take(N * (d.S + d.A)); w.xin_sas = take(N * (2 * d.S + d.A));
  w.delta = take(N);
  w.total = take.off;
  return 0;
}

// what the two entry points check alike, before any runtime call; n_src: the source rows (a->n_src, or N / 2)
static int dara_check(const MobodyDara* a, const char* who, long long& n_src) {
  MB_BLOCK(who, a, MobodyDara);
  int rc = family_sizes(who, &a->d, 2);
  if (rc) return rc;
  MB_REQUIRE(a->n_src >= 0 && a->n_src <= a->d.N, "%s: n_src %lld outside [0, N = %lld]", who, (long long)a->n_src, (long long)a->d.N);
  MB_REQUIRE(a->n_src != 0 || a->d.N % 2 == 0, "%s: N %lld is odd and n_src is not given (rows are [src | tar], n_src = N / 2)", who, (long long)a->d.N);
  n_src = a->n_src != 0 ? a->n_src : a->d.N / 2;
  MB_REQUIRE(a->sa_blob && a->sa_blob_T && a->sas_blob && a->sas_blob_T && a->state && a->action && a->next_state && a->workspace, "%s: null pointer", who);
  return check_precision(who, a->precision, true);
}
}  // namespace mobody

extern "C" int64_t mobody_dara_workspace(const MobodyTrainDims* d) {
  if (family_sizes("mobody_dara_workspace", d, 2)) return -1;
  DaraWs w;
  if (carve_dara(*d, nullptr, w)) return -1;
  return w.total;
}

// dara.py:131-144 (Classifier.forward, with_noise), :202-223 (update_classifier)
extern "C" int mobody_dara_classifier(const MobodyDara* a, void* stream) {
  const char* who = "mobody_dara_classifier";
  long long n_src = 0;
  int rc = dara_check(a, who, n_src);
  if (rc) return rc;
  // one optimizer over both heads = one step count and rate (:192); sas first, as the launches go
  const NetOpt opt[2] = {{a->grad_sas, a->m_sas, a->v_sas, a->t, a->t_dev, a->lr}, {a->grad_sa, a->m_sa, a->v_sa, a->t, a->t_dev, a->lr}};
  rc = check_opt(who, opt, 2, "grad_sa, grad_sas", " of both heads");
  if (rc) return rc;
  MB_REQUIRE(a->loss_out, "%s: null pointer", who);
  MB_REQUIRE(a->noise_std >= 0.f, "%s: noise_std %g < 0", who, (double)a->noise_std);
  DaraWs w;
  rc = carve_dara(a->d, a->workspace, w);
  if (rc) return rc;
  const int prec = a->precision;
  hipStream_t st = as_stream(stream);
  const long long N = a->d.N;
  const int S = a->d.S, A = a->d.A;
  // 1. the noisy rows [s | a | s'] and [s | a] (:132-141), one row-wise launch
  DaraInArgs in{a->state, a->action, a->next_state, a->noise_sas, a->noise_sa, N, S, A, a->noise_std, a->seed, a->call, w.xin_sas, w.xin_sa};
  rc = launch_dara_inputs(in, (const long long*)a->call_dev, a->call_offset, st);
  if (rc) return rc;
  // 2. both heads' forwards with the saves of their backwards (:136, :142): one launch
  const TrainedNet heads[2] = {{w.Lsas, w.sas, N, a->sas_blob, a->sas_blob_T, prec}, {w.Lsa, w.sa, N, a->sa_blob, a->sa_blob_T, prec}};
  rc = launch_mlp3_forward(heads[0].forward(w.xin_sas, 2 * S + A), 1, heads[1].forward(w.xin_sa, S + A), 1, ACT_RELU, prec, st);
  if (rc) return rc;
  // 3., 4. per head: the backward with the double-softmax cross-entropy seed in its prologue (:217-219), then the weight
  // gradients with the loss scalar (loss_out = (loss_sa, loss_sas)) and (fused) the Adam step
  const float invNg = 1.f / (float)a->d.N_global;
  for (int k = 0; k < 2; ++k) {
    const TrainedNet& h = heads[k];
    Mlp3BwdArgs b = h.backward();
    b.seed.mode = 7; b.seed.da.z = h.s.out; b.seed.da.ldz = 2; b.seed.da.n_src = n_src; b.seed.da.inv = invNg;
    rc = launch_mlp3_bwd_seed(b, st);
    if (rc) return rc;
    rc = h.finish(opt[k], h.s.lossp, h.s.ntiles, invNg, a->loss_out + (1 - k), false, st);
    if (rc) return rc;
  }
  return 0;
}

// dara.py:281-292 (the reward modification of train())
extern "C" int mobody_dara_relabel(const MobodyDara* a, void* stream) {
  const char* who = "mobody_dara_relabel";
  long long n_src = 0;
  int rc = dara_check(a, who, n_src);
  if (rc) return rc;
  MB_REQUIRE(a->reward || a->delta_out || a->log_out, "%s: null pointer (reward, delta_out and log_out)", who);
  MB_REQUIRE(n_src < (1LL << 31), "%s: n_src %lld does not fit the mean's launch", who, n_src);
  DaraWs w;
  rc = carve_dara(a->d, a->workspace, w);
  if (rc) return rc;
  const int prec = a->precision;
  hipStream_t st = as_stream(stream);
  const int S = a->d.S, A = a->d.A;
  // noise-free pass of both heads on the source rows (:282), state | action | next_state read in place: one launch, no saves
  Mlp3FwdArgs f_sas = fwd_net(a->sas_blob, w.Lsas, n_src), f_sa = fwd_net(a->sa_blob, w.Lsa, n_src);
  if (prec != PREC_F32) { fwd_set_planes(f_sas, a->sas_blob_T, w.Lsas); fwd_set_planes(f_sa, a->sa_blob_T, w.Lsa); }
  fwd_set_src(f_sas, 0, a->state, S, S); fwd_set_src(f_sas, 1, a->action, A, A); fwd_set_src(f_sas, 2, a->next_state, S, S);
  fwd_set_src(f_sa, 0, a->state, S, S); fwd_set_src(f_sa, 1, a->action, A, A);
  fwd_set_out(f_sas, w.sas.out, 0, 1.f); fwd_set_out(f_sa, w.sa.out, 0, 1.f);
  rc = launch_mlp3_forward(f_sas, 1, f_sa, 1, ACT_RELU, prec, st);
  if (rc) return rc;
  // reward[row] += eta * penalty (:283-292); eta == 0 leaves every reward's bits alone
  float* delta = a->delta_out ? a->delta_out : (a->log_out ? w.delta : nullptr);
  float* reward = a->eta != 0.f ? a->reward : nullptr;
  if (reward == nullptr && delta == nullptr) return 0;
  rc = launch_dara_penalty(w.sas.out, w.sa.out, n_src, a->eta, reward, delta, st);
  if (rc || a->log_out == nullptr) return rc;
  hipLaunchKernelGGL(k_sum_scale, dim3(1), dim3(256), 0, st, delta, (int)n_src, 1.f / (float)n_src, a->log_out);   // train/reward penalty (:290)
  MB_LAUNCH_OK("k_sum_scale");
  return 0;
}

// ---- IGDF (the reference's algo/offline_offline/igdf.py): IQL's step behind a data filter -- two contrastive encoders score the
// source rows, the k best are kept -- with a row-weighted critic loss.  The encoders are one-member nets trained like DARA's heads,
// except that their loss couples the rows: its gradient is formed by k_igdf_contrast and read from memory (seed mode 0).
// DESIGN 5t. ----
namespace mobody {
struct IgdfWs {
  IqlWs iq;                // IQL's scratch, where its three entry points carve it
  MobodyMlpLayout Lsa, Lss;
  OneNetScratch sa, ss;       // on n and 2n-1 rows
  float* score;            // [n]
  int32_t* kept;           // [n]
  long long total;
};

static int carve_igdf(const MobodyTrainDims& d, long long n, int Z, float* base, IgdfWs& w) {
  int rc = carve_iql(d, base, w.iq);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S + d.A, Z, 1, &w.Lsa);
  if (rc) return rc;
  rc = mobody_mlp_layout(d.S, Z, 1, &w.Lss);
  if (rc) return rc;
  Carver take{base, w.iq.total};
  carve_one_net(w.Lsa, n, 1, w.sa, take);
  carve_one_net(w.Lss, 2 * n - 1, 1, w.ss, take);
  w.score = take(n); w.kept = (int32_t*)take(n);
  w.total = take.off;
  return 0;
}

static int igdf_check_sizes(const char* who, const MobodyTrainDims* d, long long n, int Z) {
  int rc = family_sizes(who, d, 1);
  if (rc) return rc;
  MB_REQUIRE(n >= 2 && n <= IGDF_MAX_N, "%s: n %lld outside [2, %d]", who, n, IGDF_MAX_N);
  MB_REQUIRE(Z >= 1 && Z <= IGDF_MAX_Z, "%s: Z %d outside [1, %d]", who, Z, IGDF_MAX_Z);
  return 0;
}

// what the two entry points check alike, before any runtime call
static int igdf_check(const MobodyIgdf* a, const char* who) {
  MB_BLOCK(who, a, MobodyIgdf);
  int rc = igdf_check_sizes(who, &a->d, a->n, a->Z);
  if (rc) return rc;
  MB_REQUIRE(a->sa_blob && a->sa_blob_T && a->ss_blob && a->ss_blob_T && a->state && a->action && a->next_state && a->workspace, "%s: null pointer", who);
  return check_precision(who, a->precision, true);
}
}  // namespace mobody

extern "C" int64_t mobody_igdf_workspace(const MobodyTrainDims* d, int64_t n, int32_t Z) {
  if (igdf_check_sizes("mobody_igdf_workspace", d, n, Z)) return -1;
  IgdfWs w;
  if (carve_igdf(*d, n, Z, nullptr, w)) return -1;
  return w.total;
}

// igdf.py:418-447 (update_info, one step)
extern "C" int mobody_igdf_info(const MobodyIgdf* a, void* stream) {
  const char* who = "mobody_igdf_info";
  int rc = igdf_check(a, who);
  if (rc) return rc;
  // one optimizer over both encoders = one step count and rate (:407)
  const NetOpt opt[2] = {{a->grad_sa, a->m_sa, a->v_sa, a->t, a->t_dev, a->lr}, {a->grad_ss, a->m_ss, a->v_ss, a->t, a->t_dev, a->lr}};
  rc = check_opt(who, opt, 2, "grad_sa, grad_ss", " of both encoders");
  if (rc) return rc;
  MB_REQUIRE(a->bump == nullptr || (a->m_sa != nullptr && a->bump != a->t_dev), "%s: bump is incremented by the optimizer launch: it needs m, v and must not be the step word", who);
  MB_REQUIRE(a->loss_out, "%s: null pointer", who);
  IgdfWs w;
  rc = carve_igdf(a->d, a->n, a->Z, a->workspace, w);
  if (rc) return rc;
  const int prec = a->precision;
  hipStream_t st = as_stream(stream);
  const long long n = a->n, n2 = 2 * n - 1;
  const int S = a->d.S, A = a->d.A, Z = a->Z;
  // 1. phi = encoder_sa([s | a]) on the n target rows, psi = encoder_ss(s') on [tar s' | src s'] (:424-434): one launch, with the
  // saves of the backwards.  (The reference encodes n^2 next states of which 2n-1 are distinct.)
  const TrainedNet encs[2] = {{w.Lsa, w.sa, n, a->sa_blob, a->sa_blob_T, prec}, {w.Lss, w.ss, n2, a->ss_blob, a->ss_blob_T, prec}};
  rc = launch_mlp3_forward(encs[1].forward(a->next_state, S), 1, encs[0].forward(a->state, S, a->action, A), 1, ACT_RELU, prec, st);
  if (rc) return rc;
  // 2. the loss partials and dL/dphi, dL/dpsi (:434-440)
  rc = launch_igdf_contrast(w.sa.out, w.ss.out, w.ss.out + n * Z, n, Z, Z, w.Lsa.Np3, w.sa.dz3, w.ss.dz3, w.sa.lossp, st);
  if (rc) return rc;
  // 3., 4. per encoder: the backward from dz3 in memory, then the weight gradients with (sa) the loss scalar and (fused) the Adam
  // step (the last one advances `bump`)
  for (int e = 0; e < 2; ++e) {
    const TrainedNet& h = encs[e];
    rc = launch_mlp3_bwd(h.backward(h.s.dz3), 1, false, st);
    if (rc) return rc;
    rc = h.finish(opt[e], w.sa.lossp, (int)cdiv(n, IGDF_TILE), 1.f / ((float)n * (float)n), e == 0 ? a->loss_out : nullptr, false, st,
                  e == 1 ? a->bump : nullptr);
    if (rc) return rc;
  }
  return 0;
}

// igdf.py:494-524 (the data filter of train())
extern "C" int mobody_igdf_filter(const MobodyIgdf* a, void* stream) {
  const char* who = "mobody_igdf_filter";
  int rc = igdf_check(a, who);
  if (rc) return rc;
  MB_REQUIRE(a->k >= 1 && a->k <= a->n, "%s: k %lld outside [1, n = %lld]", who, (long long)a->k, (long long)a->n);
  MB_REQUIRE(a->d.N >= a->k, "%s: d.N %lld < k %lld (the training batch is the k kept rows and the target rows)", who, (long long)a->d.N, (long long)a->k);
  MB_REQUIRE(a->reward && a->not_done && a->out_state && a->out_action && a->out_next_state && a->out_reward && a->out_not_done && a->row_weight,
             "%s: null pointer", who);
  IgdfWs w;
  rc = carve_igdf(a->d, a->n, a->Z, a->workspace, w);
  if (rc) return rc;
  const int prec = a->precision;
  hipStream_t st = as_stream(stream);
  const long long n = a->n;
  const int S = a->d.S, A = a->d.A, Z = a->Z;
  // both encoders on the source rows (:500), state | action and next_state read in place: one launch, no saves
  Mlp3FwdArgs f_sa = fwd_net(a->sa_blob, w.Lsa, n), f_ss = fwd_net(a->ss_blob, w.Lss, n);
  if (prec != PREC_F32) { fwd_set_planes(f_sa, a->sa_blob_T, w.Lsa); fwd_set_planes(f_ss, a->ss_blob_T, w.Lss); }
  fwd_set_src(f_sa, 0, a->state, S, S); fwd_set_src(f_sa, 1, a->action, A, A);
  fwd_set_src(f_ss, 0, a->next_state, S, S);
  fwd_set_out(f_sa, w.sa.out, 0, 1.f); fwd_set_out(f_ss, w.ss.out, 0, 1.f);
  rc = launch_mlp3_forward(f_sa, 1, f_ss, 1, ACT_RELU, prec, st);
  if (rc) return rc;
  float* score = a->score_out ? a->score_out : w.score;
  rc = launch_igdf_score(w.sa.out, w.ss.out, n, Z, Z, score, st);
  if (rc) return rc;
  IgdfBatch b{a->state, a->action, a->next_state, a->reward, a->not_done, a->out_state, a->out_action, a->out_next_state, a->out_reward,
              a->out_not_done, a->row_weight, a->d.N - a->k, S, A};
  return launch_igdf_select(score, n, a->k, a->importance_weight, a->kept_out ? a->kept_out : w.kept, nullptr, b, st);
}

extern "C" int mobody_igdf_critic(const MobodyIql* a, const float* row_weight, void* stream) {
  return iql_critic_impl(a, row_weight, stream, "mobody_igdf_critic");
}

extern "C" int mobody_mlp_transpose(int in_dim, int out_dim, int members, const float* blob, float* blob_T, int precision,
                                    void* stream) {
  MobodyMlpLayout L;
  int rc = mobody_mlp_layout(in_dim, out_dim, members, &L);
  if (rc) return rc;
  MB_REQUIRE(blob && blob_T, "mobody_mlp_transpose: null pointer");
  rc = check_precision("mobody_mlp_transpose", precision, true);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mlp_transpose, dim3((unsigned)cdiv(L.t_total_floats, 256)), dim3(256), 0, as_stream(stream), L, blob, blob_T,
                     precision, health_words());
  MB_LAUNCH_OK("k_mlp_transpose");
  return 0;
}

static int adam_impl(const MobodyAdam& a, void* stream) {
  const char* who = "mobody_adam_polyak";
  MobodyMlpLayout L;
  int rc = mobody_mlp_layout(a.in_dim, a.out_dim, a.members, &L);
  if (rc) return rc;
  MB_REQUIRE(a.blob && a.grad && a.m && a.v, "%s: null pointer", who);
  MB_REQUIRE(a.t_dev != nullptr || a.t >= 1, "%s: step t must be >= 1", who);
  rc = check_precision(who, a.precision, true);
  if (rc) return rc;
  AdamTarget at = adam_target(a.blob, a.blob_T, a.m, a.v, a.target, a.t, a.t_dev, a.lr, a.tau, a.grad_scale, a.precision);
  at.target_T = at.target ? a.target_T : nullptr;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)cdiv(L.total_floats, 256)), dim3(256), 0, st, at, a.grad, (long long)L.total_floats, L);
  MB_LAUNCH_OK("k_adam");
  return 0;       // (W1T's zero padding columns k >= Kp1 are written once by mobody_mlp_transpose and never change)
}

extern "C" int mobody_adam_polyak(const MobodyAdam* a, void* stream) {
  MB_BLOCK("mobody_adam_polyak", a, MobodyAdam);
  return adam_impl(*a, stream);
}

// ---- PAR reward penalty: r -= coef * mean_d (s'_true - s'_model)^2   (mobody.py:428-434) ----
namespace mobody {
__global__ __launch_bounds__(256) void k_par_penalty(const float* ns_true, const float* ns_model, float* reward, float coef,
                                                     long long n, int S) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  // In double, rounded once: in fp32 the differences alone cost 2 u of the mean (u = 2^-24) before its S products and adds, and a
  // row at S = 1 missed the (S + 2) u tests/test_hip_aux_rowwise.py holds it to.  The kernel streams 2 S floats per row: free.
  double s = 0.0;
  for (int d = 0; d < S; ++d) { const double e = (double)ns_true[row * S + d] - (double)ns_model[row * S + d]; s += e * e; }
  reward[row] = (float)((double)reward[row] - (double)coef * (s / (double)S));
}
}  // namespace mobody

extern "C" int mobody_par_penalty(const float* next_state_true, const float* next_state_model, float* reward, float coef,
                                  int64_t n, int S, void* stream) {
  MB_REQUIRE(n >= 0 && S >= 1, "mobody_par_penalty: bad sizes");
  if (n == 0) return 0;
  MB_REQUIRE(next_state_true && next_state_model && reward, "mobody_par_penalty: null pointer");
  hipLaunchKernelGGL(k_par_penalty, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), next_state_true,
                     next_state_model, reward, coef, (long long)n, S);
  MB_LAUNCH_OK("k_par_penalty");
  return 0;
}


// ---- V-function expectile loss (advantage variant): dz3[N][16] and loss_out[0] = local share of L_V ----
extern "C" int mobody_value_loss_grad(const float* qt, const float* v, int64_t N, int64_t N_global, float* dz3,
                                      float* loss_out, float* lossp_ws, void* stream) {
  MB_REQUIRE(N >= 1 && N_global >= N, "mobody_value_loss_grad: bad sizes");
  MB_REQUIRE(qt && v && dz3 && loss_out && lossp_ws, "mobody_value_loss_grad: null pointer");
  const int nb = (int)cdiv(N, 256);
  const float invNg = 1.f / (float)N_global;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_v_loss, dim3(nb), dim3(256), 0, st, qt, v, (long long)N, invNg, 16, dz3, lossp_ws);
  MB_LAUNCH_OK("k_v_loss");
  hipLaunchKernelGGL(k_sum_scale, dim3(1), dim3(256), 0, st, lossp_ws, nb, invNg, loss_out);
  MB_LAUNCH_OK("k_sum_scale");
  return 0;
}
