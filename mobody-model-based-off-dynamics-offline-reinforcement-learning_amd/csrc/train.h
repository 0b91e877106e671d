// Argument blocks shared by the training translation units (mlp_bwd.hip, train.hip).
#pragma once
#include <math.h>
#include <stdlib.h>

#include "common.h"
#include "layers.h"
#include "tile.h"
#include "tile_bf.h"
#include "health.h"

namespace mobody {

// Row-wise quantities of the actor update (mobody.py:246-276, 314-345) shared by the two seed prologues of k_actor_bwd_chain.
struct ActorRowArgs {
  const float *qp, *qb, *stats, *pi, *act, *dxa;
  const float* v_true;       // [Nt] V(s_true) when config['advantage'] (else null)
  float* bcw;                // [Nt] BC weights (written by the frozen-Q backward, read by the actor backward)
  long long N, Nt, Ng, Ntg;
  int A;
  MobodyHyper h;
};
__device__ __forceinline__ float policy_weight(const ActorRowArgs& a) {       // p_w, mobody.py:318 / :283
  return a.h.scale_q ? a.h.weight / (a.stats[0] / (float)a.Ng) : 1.f;
}
__device__ __forceinline__ float bc_weight(const ActorRowArgs& a, long long row) {   // exp_adv, :257-267
  if (!a.h.q_weighted) return 1.f;
  const float qb = fminf(a.qb[row], a.qb[a.Nt + row]);
  const float adv = a.v_true ? qb - a.v_true[row]                      // advantage variant, mobody.py:255-256
                             : qb / (a.stats[1] / (float)a.Ntg);
  return fminf(expf(3.f * adv), 100.f);
}

// Where the output-layer gradient dz3 of a backward launch comes from.  Modes 1-3 compute it in the kernel's
// prologue from the row-wise inputs (no separate row-wise launch, no dz3 round trip through HBM before the first GEMM):
//   0  dz3 read from memory
//   1  critic: y = r + nd*gamma*min(Qt1,Qt2) (or q_next); dz3[m][row][0] = 2 (q_m - y) / N_global   (mobody.py:190-207)
//      lossp[tile*2 + m] = sum_rows (q_m - y)^2
//   2  frozen twin-Q of the actor update: dz3[m][row][0] = -p_w/N_global * d min(q0,q1)/dq_m (ties split 1/2, as
//      torch.min's backward); member 0 also writes the BC weights bcw[row < Nt].  The net takes no parameter gradient:
//      this mode stores no bias-gradient partials (`dbp` is not written).
//   3  actor: d(pre-tanh) = (dxa[0]+dxa[1] + bc_coef*2*w*(pi-a)/(Ntg*A)) * max_action*(1-tanh^2);
//      lossp[2*tile] = sum -min q, lossp[2*tile+1] = sum w*(pi-a)^2
//   4  frozen twin-Q of the TD3_BC actor update (td3_bc.py:160-176), in mode 2's place: every row is a BC row (Nt == N) and the
//      BC weight w = min(e, 100), e = exp(k q/m), q = min(q0,q1), m = stats[0]/N_global (detached), carries a gradient through q:
//        dq = -(weight/m)/N_global + (q_weighted && e <= 100 ? bc_coef * (k e/m) * sum_j (pi-a)^2 / (N_global*A) : 0)
//        dz3[m][row][0] = dq * d min(q0,q1)/dq_m (ties as mode 2);  member 0 writes bcw[row] = q_weighted ? w : 1
//      k = `exp_scale`.  The clamp's gradient is a select (e overflows to inf past q/m = 88).  The actor tile behind it is mode 3.
// Modes 1 and 3 also store dz3 to `dz3_out` (the weight-gradient GEMM reads it).  Modes 1 and 2 seed column 0 of a
// one-output net only: the kernel forms dz3 W3^T as the rank-1 product it is instead of running the K = Np3 GEMM.
// Where each runs: launch_mlp3_bwd (k_mlp3_bwd) takes modes 0 and 1 and chooses between them at run time; modes 2 and 3 exist
// only as the two tiles of launch_actor_bwd_chain (k_actor_bwd_chain), compiled in, with mode 2's dx / bcw handed to mode 3 in
// agent-scope stores and loads; mode 4 is mode 2's alternative as the first tile (the chain's third template argument).  Mode 1
// also runs, compiled in (bwd_tile.h SEED_CRITIC_CHAIN), as the tiles chained onto the merged critic forward (critic_fwd_bf.hip).
//   5  IQL's V net (iql.py:174-185, asymmetric_l2_loss :117-118), one output: adv = min(qt[0], qt[1]) - v,
//        dz3[row][0] = -2 |lam - 1[adv < 0]| adv / N_global; adv_out[row] = adv (the policy phase's weights come from it);
//        lossp[tile] = sum |lam - 1[adv<0]| adv^2, lossp[T + tile] = sum adv, lossp[2 T + tile] = sum v (T row tiles)
//   6  IQL's policy net (update_policy + bc_loss, iql.py:91-95, :198-202), Np3 = pad16(2 A) outputs of which the first A are mu:
//        w = min(exp(temp * adv[row]), 100), th = tanh(z[row][j]);  j < A: dz3 = 2 w (th - a)(1 - th^2) / (N_global A), j >= A: 0
//        (the logstd half takes no gradient); lossp[tile] = sum w (th - a)^2.  Its first tile also forms, from the device step
//        count, the Adam constants of the policy's cosine learning rate for the k_grad_reduce launch behind it (bc_out).
//   7  DARA's classifier heads (dara.py:131-144, :217-219), two real outputs of an Np3 = 16 net: z = z[row][0..1], label = 0 for
//        row < n_src, else 1; dz3[row][0..1] = d/dz of cross_entropy(softmax(z), label) / N_global -- the loss applies its own
//        log_softmax to the head's probabilities (ce_on_probs, dara.h: the one copy of that arithmetic) --, columns >= 2: 0;
//        lossp[tile] = sum -log q[label].  Rides mode 6's general K = Np3 path for dz3 W3^T.
//   8  IGDF's row-weighted critic (igdf.py:468-479): mode 1 with a per-row weight w = cw.w[row], dz3[m][row][0] = 2 w (q_m - y) /
//        N_global, lossp[tile*2 + m] = sum w (q_m - y)^2; runs in launch_mlp3_bwd_wcritic (k_mlp3_bwd_wcritic), compiled in, so the
//        kernels of mode 1 keep their code.  Its weight pointer rides in the bytes of `ar`, which modes 1 and 8 do not read.
//   9  BOSA's masked conservative critic (bosa.py:596-598): mode 8 plus a per-row constant c = cs.c[row],
//        dz3[m][row][0] = 2 w (q_m - y) / N_global + c  (c == 0: exactly mode 8's value); the partial sums are PAIRS,
//        lossp[2 (tile*2 + m)] = sum w (q_m - y)^2 and lossp[2 (tile*2 + m) + 1] = sum_{c != 0} q_m (LossFinal kind 2's layout); runs in
//        launch_mlp3_bwd_ccritic (k_mlp3_bwd_ccritic), compiled in, so the kernels of modes 1 and 8 keep their code.
// Modes 5, 6 and 7 run in launch_mlp3_bwd_seed (k_mlp3_bwd_seed), compiled in; their row-wise arguments are `iq` (5, 6) or `da`
// (7), which share the bytes of `ar`.
struct IqlSeed {
  const float *qt, *v;         // mode 5: [2][rows] target twin-Q(s, a), [rows] V(s)
  const float *z, *act, *adv;  // mode 6: [rows][ldz] linear policy outputs, [rows][A] actions, [rows] adv of mode 5
  float* adv_out;              // mode 5
  float* bc_out;               // mode 6, or null: {lr_k / (1 - 0.9^k), sqrt(1 - 0.999^k)}, k = t_dev[0]
  const long long* t_dev;
  long long T_max;
  float lam, temp, inv, lr0;   // inv: 1 / N_global (mode 5), 1 / (N_global A) (mode 6)
  int A, ldz;
};
struct DaraSeed {
  const float* z;              // [rows][ldz] the head's two logits
  long long n_src;             // rows < n_src carry label 0, the rest label 1
  float inv;                   // 1 / N_global
  int ldz;
};
struct CriticSeed {
  const float* w;              // [rows] row weights of the critic loss (mode 8 reads nothing else of the union)
};
struct ConsSeed {
  const float* w;              // [rows] row weights, as CriticSeed's
  const float* c;              // [rows] additive constants of the seed; rows with c != 0 enter the second partial sum
};
struct BwdSeed {
  int mode;
  const float *q, *qt, *qnext, *r, *nd;      // mode 1 ([2][rows] q and qt, [rows] the rest)
  union { float gamma; float exp_scale; };   // mode 1: the discount; mode 4: the exponent scale k of the BC weight
  float inv_ng;
  union {
    ActorRowArgs ar;                         // modes 2, 3, 4
    IqlSeed iq;                              // modes 5, 6
    DaraSeed da;                             // mode 7
    CriticSeed cw;                           // mode 8
    ConsSeed cs;                             // mode 9
  };
  float* dz3_out;
  float* lossp;
};
static_assert(sizeof(IqlSeed) <= sizeof(ActorRowArgs) && alignof(IqlSeed) == alignof(ActorRowArgs),
              "IqlSeed rides in ActorRowArgs' bytes: the argument block of every backward kernel keeps its layout");
static_assert(sizeof(DaraSeed) <= sizeof(ActorRowArgs) && alignof(DaraSeed) == alignof(ActorRowArgs),
              "DaraSeed rides in ActorRowArgs' bytes: the argument block of every backward kernel keeps its layout");

static_assert(sizeof(CriticSeed) <= sizeof(ActorRowArgs) && alignof(CriticSeed) == alignof(ActorRowArgs),
              "CriticSeed rides in ActorRowArgs' bytes: the argument block of every backward kernel keeps its layout");

static_assert(sizeof(ConsSeed) <= sizeof(ActorRowArgs) && alignof(ConsSeed) == alignof(ActorRowArgs),
              "ConsSeed rides in ActorRowArgs' bytes: the argument block of every backward kernel keeps its layout");

struct Mlp3BwdArgs {
  BwdSeed seed;
  const float* dz3;        // [members][rows][Np3] (zero in padded columns); seed.mode 0 only
  const float* h1;         // [members][rows][256] post-ReLU hidden activations saved by the forward
  const float* h2;         // (swish != 0: the Swish derivatives save_d1 / save_d2 of k_mlp3_fwd_train instead)
  int swish;
  const uint32_t* m1;      // [members][ceil(rows/32)][256] sign bits of h1 / h2 written by the forward; when both are
  const uint32_t* m2;      // given they replace h1 / h2 (which may then be null)
  const float* wt;         // transposed blob (member 0)
  const unsigned short* w2t_planes;   // bf16 planes of W2^T (member 0; wt + L.w2tp) and the precision (0 = exact fp32 MFMA)
  long long planes_ms;
  int prec;
  long long t_mstride, w3t, w2t, w1t;
  int Np3, Np1t;
  long long rows;
  float* dz2;              // [members][rows][256] or null (not needed when only dx is wanted)
  float* dz1;
  unsigned short* dz2p;    // f16 mode, instead of dz2: its two fp16 planes in the weight-gradient GEMM's fragment layout
  long long dz2p_ms;       // ([member][2][rows32 / 8][256][8]; member / plane strides in 16-bit elements, layers_bf.h PlaneSave)
  long long dz2p_plane;
  int* e2_out;             // [members][ceil(rows / 32)] the tiles' scale exponents of dz2p
  float* dbp;              // [tiles][members][512 + Np3] bias-gradient partials: db1 | db2 | db3
  float* dx;               // [members][rows][dx_n] input gradient columns [dx_c0, dx_c0 + dx_n)  (DX only)
  int dx_c0, dx_n;
};
int launch_mlp3_bwd(const Mlp3BwdArgs& a, int members, bool with_dx, hipStream_t st);
// the actor update's frozen-Q pass `q` (seed mode 2, 2 members, dx) and actor pass `pi` (seed mode 3) in one launch: the second of a
// tile's two member workgroups to finish runs that tile's actor backward (mlp_bwd.hip k_actor_bwd_chain).  tickets: one int per
// row tile, zero on entry and on exit.
int launch_actor_bwd_chain(const Mlp3BwdArgs& q, const Mlp3BwdArgs& pi, int* tickets, hipStream_t st);
// one net (member 0), sign words, seed mode 5, 6 or 7 formed in the prologue; no dx
int launch_mlp3_bwd_seed(const Mlp3BwdArgs& a, hipStream_t st);
// the twin-Q net (two members), sign words, seed mode 8 (mode 1's fields + cw.w) formed in the prologue; no dx
int launch_mlp3_bwd_wcritic(const Mlp3BwdArgs& a, hipStream_t st);
// the twin-Q net (two members), sign words, seed mode 9 (mode 1's fields + cs.w, cs.c) formed in the prologue; no dx
int launch_mlp3_bwd_ccritic(const Mlp3BwdArgs& a, hipStream_t st);
// learning rate of 1-based gradient step k under CosineAnnealingLR(T_max), eta_min 0 (closed form, in double, rounded to fp32 once)
__host__ __device__ inline float cosine_lr(float lr0, long long k, long long T_max) {
  return (float)((double)lr0 * (1.0 + cos(3.14159265358979323846 * (double)(k - 1) / (double)T_max)) * 0.5);
}

// ---- host side: the one place an Mlp3BwdArgs is filled; each helper owns one group of fields (the seed and dx are the caller's).
// launch_mlp3_bwd picks its kernel from swish, prec + w2t_planes and m1 + m2, so every caller states those explicitly. ----
// transposed weights of a packed MLP (mobody_mlp_layout) on `rows` rows; everything else zero = exact fp32, ReLU, dz3 from memory
inline Mlp3BwdArgs bwd_net(const MobodyMlpLayout& L, const float* blob_T, long long rows) {
  Mlp3BwdArgs b{};
  b.wt = blob_T; b.t_mstride = L.t_member_floats;
  b.w3t = L.w3t; b.w2t = L.w2t; b.w1t = L.w1t; b.Np3 = L.Np3; b.Np1t = L.Np1t; b.rows = rows;
  return b;
}
// the precision id and W2^T's planes in the T blob (a launch without them runs the 256 x 256 GEMM on exact fp32 MFMA)
inline void bwd_set_planes(Mlp3BwdArgs& b, const MobodyMlpLayout& L, int prec) {
  b.prec = prec; b.w2t_planes = reinterpret_cast<const unsigned short*>(b.wt + L.w2tp); b.planes_ms = 2 * L.t_member_floats;
}
// what the forward saved: ReLU nets h1 / h2 or (replacing them) the sign words m1 / m2; swish = 1: the derivatives d1 / d2
inline void bwd_set_acts(Mlp3BwdArgs& b, const float* h1, const float* h2, const uint32_t* m1, const uint32_t* m2, int swish) {
  b.h1 = h1; b.h2 = h2; b.m1 = m1; b.m2 = m2; b.swish = swish;
}
// dz3 in (seed.mode 0) and dz2 / dz1 / the bias partials out.  e2 != null (f16x2, needs bwd_set_planes) and dz2: dz2 leaves as the
// two fp16 planes + tile exponents the weight-gradient GEMM reads, not as fp32 rows
inline void bwd_set_grads(Mlp3BwdArgs& b, const float* dz3, float* dz2, float* dz1, float* dbp, int* e2 = nullptr) {
  if (e2 != nullptr && dz2 != nullptr) {
    const long long r32 = (b.rows + 31) & ~31LL;
    b.dz2p = reinterpret_cast<unsigned short*>(dz2); b.dz2p_plane = r32 * HID; b.dz2p_ms = 2 * r32 * HID; b.e2_out = e2;
    dz2 = nullptr;
  }
  b.dz3 = dz3; b.dz2 = dz2; b.dz1 = dz1; b.dbp = dbp;
}

struct WgradJob {
  const float* A; long long a_mstride; int lda, ka;    // A[rows][lda], columns < ka contribute (output rows)
  const float* B; long long b_mstride; int ldb, nb;    // B[rows][ldb], columns < nb contribute (output cols)
  long long out_off; int out_ld, out_k, out_n;         // slab + out_off + m*out_mstride + k*out_ld + n  (k<out_k, n<out_n)
  int transposed;                                      // store [n][k] instead (used for dW3, computed as dz3^T h2)
  int wide;                                            // destination is a 256-wide matrix in wide_idx storage
  int tiles_n, ntiles;                                 // filled by launch_wgrad
};
struct WgradArgs {
  // prec 4 ("f16x2"): job 0's operands are NOT fp32 rows but the planes the forward / backward epilogues saved
  // (job[0].A = h1 planes, job[0].B = dz2 planes: [member][2][rows32 / 8][256][8] fp16, a_mstride / b_mstride in 16-bit
  // elements) together with the 32-row tiles' scale exponents eA / eB ([member][tiles])
  const int *eA, *eB;
  long long e_mstride, plane_stride;                   // tiles per member; 16-bit elements between the two planes
  WgradJob job[3];                                     // job 0: 64x64 wave tiles, jobs 1-2: 32x64
  long long rows, rows_per_wave;
  float* slabs; long long slab_stride, out_mstride;    // partial slab s = slabs + s*slab_stride (gradient-blob layout)
  int nsplit, members, tiles_total;
  // bc_out != null: the launch's last workgroup forms the Adam bias corrections of the device step count bc_t[0] at learning
  // rate bc_lr (adam_block_consts' expressions) for the k_grad_reduce launch that follows it on the stream
  float* bc_out; const long long* bc_t; float bc_lr;
  int prec;                                            // precision id (common.h): f32 exact; bf16 modes: the 256 x 256 job on the
                                                       // split-precision core; f16x2 with eA: job 0 on the saved fp16 planes
};
int launch_wgrad(WgradArgs a, hipStream_t st);

// Same op forms as torch's single-tensor Adam: exp_avg.lerp_(g, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
// denom = sqrt(v)/sqrt(bc2) + eps; p.addcdiv_(m, denom, -lr/bc1).  The scalar constants are formed in double
// on the host and rounded to fp32 once, as torch does when it multiplies a fp32 tensor by a Python float.
// beta1 = 0.9, beta2 = 0.999, eps = 1e-8 (torch's defaults, what every caller uses) are constants of the element functions.
struct AdamConsts { float step_size, bc2_sqrt, tau, one_minus_tau, gscale; };
constexpr float ADAM_W1 = (float)(1.0 - 0.9), ADAM_B2 = (float)0.999, ADAM_W2 = (float)(1.0 - 0.999), ADAM_EPS = 1e-8f;

// W2[k][n] = w -> its terms in the planes of W2 (as B[k][n]) and of W2^T (as B[n][k]) of a member's T blob: the three bf16
// terms (precision modes 0-3 share them), or -- precision 4, "f16x2" -- the two fp16 terms of w * 2^F16_WSHIFT in planes 0, 1
__device__ __forceinline__ void write_w2_planes(float* t_member, const MobodyMlpLayout& L, int k, int n, float w, int precision) {
  short* p2 = reinterpret_cast<short*>(t_member + L.w2p);
  short* p2t = reinterpret_cast<short*>(t_member + L.w2tp);
  if (precision == 4) {
    short t[2];
    split_terms<4>(w * exp2i(F16_WSHIFT), t);
#pragma unroll
    for (int p = 0; p < 2; ++p) { p2[bf_plane_idx(p, k, n)] = t[p]; p2t[bf_plane_idx(p, n, k)] = t[p]; }
  } else {
    short t[3];
    split_terms<3>(w, t);
#pragma unroll
    for (int p = 0; p < 3; ++p) { p2[bf_plane_idx(p, k, n)] = t[p]; p2t[bf_plane_idx(p, n, k)] = t[p]; }
  }
}

// Destination of parameter entry (member-local offset o) inside the member's T blob, or -1 (biases, padding rows).
__device__ __forceinline__ long long t_blob_index(const MobodyMlpLayout& L, long long o) {
  if (o < L.b1) {                                   // W1 (wide storage): W1T[n][k] row major, ld = Np1t
    const long long g = o >> 2;
    const int k = (int)(g / HID) * 4 + (int)(o & 3), n = (int)(g % HID);
    return L.w1t + (long long)n * L.Np1t + k;
  }
  if (o >= L.w2 && o < L.b2) {                      // W2 (wide): W2T[n][k] wide
    const long long oo = o - L.w2, g = oo >> 2;
    const int k = (int)(g / HID) * 4 + (int)(oo & 3), n = (int)(g % HID);
    return L.w2t + wide_idx(n, k);
  }
  if (o >= L.w3 && o < L.b3) {                      // W3 (narrow [256][Np3]): W3T[n3][k] wide
    const long long oo = o - L.w3;
    const int k = (int)(oo / L.Np3), n3 = (int)(oo % L.Np3);
    return L.w3t + wide_idx(n3, k);
  }
  return -1;
}

// Parameter blobs an optimizer step works on.  Used by k_adam (gradient read from a blob) and by k_grad_reduce (the
// single-GPU fused form: the element's gradient is the slab / partial sum it has just formed -- one launch and one
// gradient round trip through HBM fewer per network and step).
struct AdamTarget {
  float *p, *m, *v, *target, *blob_T;       // target / blob_T may be null
  float* target_T;                          // T blob of the target net (its W2 planes follow the Polyak update); may be null
  AdamConsts c;
  const long long* t_dev;                   // device step count (graph replay) or null
  float lr;
  int on;                                   // k_grad_reduce only: 0 = just write the gradient
  long long* bump;                          // k_grad_reduce only: device word incremented by one thread (not t_dev), or null
  int precision;                            // format of the W2 planes kept in blob_T / target_T (write_w2_planes); < 0: no planes
                                            // (dynamics pre-training runs exact fp32: six scattered 2-byte stores per W2 element saved)
  int* health;                              // health words of the device or null; this launch's tag and host step count
  int health_tag, t_host;
};
__device__ __forceinline__ int adam_step_count(const AdamTarget& a) { return a.t_dev != nullptr ? (int)a.t_dev[0] : a.t_host; }

// torch.optim.Adam scalar bookkeeping in double, as the reference's host code does; t_dev != null: the kernel forms the bias
// corrections itself from the device step count.  target == null or tau < 0: no Polyak update.  The caller sets target_T / bump.
inline AdamTarget adam_target(float* blob, float* blob_T, float* m, float* v, float* target, int64_t t, const int64_t* t_dev,
                              float lr, float tau, float grad_scale, int precision) {
  const double tt = t_dev ? 1.0 : (double)t;
  const double bc1 = 1.0 - pow(0.9, tt), bc2 = 1.0 - pow(0.999, tt);
  AdamTarget a{};
  a.p = blob; a.m = m; a.v = v; a.blob_T = blob_T;
  a.target = (target != nullptr && tau >= 0.f) ? target : nullptr;
  a.c.step_size = (float)((double)lr / bc1); a.c.bc2_sqrt = (float)sqrt(bc2);
  a.c.tau = tau; a.c.one_minus_tau = (float)(1.0 - (double)tau); a.c.gscale = grad_scale;
  a.t_dev = (const long long*)t_dev; a.lr = lr; a.on = 1; a.precision = precision;
  a.health = health_words(); a.health_tag = a.health ? health_next_tag() : 0; a.t_host = (int)t;
  return a;
}

// after an element's update: a non-finite parameter in any mode, an online / target W2 value past the fp16 planes' range
__device__ __forceinline__ void health_after_update(const AdamTarget& a, float pj, bool w2_plane, float tj, bool w2t_plane) {
  if (a.health == nullptr) return;
  int bits = 0;
  if (!(fabsf(pj) < INFINITY)) bits |= MOBODY_HEALTH_NONFINITE;
  if (a.precision == 4 && ((w2_plane && !(fabsf(pj) < F16_W_LIMIT)) || (w2t_plane && !(fabsf(tj) < F16_W_LIMIT)))) bits |= MOBODY_HEALTH_F16_RANGE;
  if (bits != 0) health_flag(a.health, bits, a.health_tag, adam_step_count(a));
}

// Bias corrections of a device-side step count (graph replay), formed ONCE per workgroup in double: thread 0 computes,
// everybody reads after the barrier.  (Every thread evaluating two double pow() per element made the fused
// reduce+Adam kernel 3x slower: 5.5 -> 17 us on the 0.5 M-parameter ensemble nets.)  Call before any early return.
// The same two values by one thread, for a launch that runs after this one (WgradArgs::bc_out).
__device__ __forceinline__ void adam_dev_consts(const long long* t_dev, float lr, float* out) {
  const double t = (double)t_dev[0];
  out[0] = (float)((double)lr / (1.0 - pow(0.9, t)));
  out[1] = (float)sqrt(1.0 - pow(0.999, t));
}
__device__ __forceinline__ void adam_block_consts(const AdamTarget& a, float* sm2) {
  if (a.on && a.t_dev != nullptr) {
    if (threadIdx.x == 0) {
      const double t = (double)a.t_dev[0];
      sm2[0] = (float)((double)a.lr / (1.0 - pow(0.9, t)));
      sm2[1] = (float)sqrt(1.0 - pow(0.999, t));
    }
    __syncthreads();
  }
}

// The health mask as an optimizer kernel reads it on entry: a uniform load (one scalar load per wave, no barrier, no LDS --
// a per-workgroup read behind a barrier put a memory round trip in front of every workgroup's first loads and cost 3 % of
// the c2 step and 27 % of the pre-training step).  The element functions test it only in front of their stores,
// so the load overlaps their own loads.  A stale 0 can only be seen inside the faulting launch, where 0 is the right answer.
__device__ __forceinline__ int health_mask(const AdamTarget& a) { return a.health != nullptr ? a.health[0] : 0; }
// mask != 0: was the fault raised by ANOTHER launch?  (slow path: acquire fence, then the key the faulting lane published)
__device__ __forceinline__ bool health_foreign(const AdamTarget& a) {
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  const unsigned long long key = __atomic_load_n(reinterpret_cast<const unsigned long long*>(a.health + 2), __ATOMIC_RELAXED);
  // (a host-count launch has a tag of its own; a captured one shares its tag with its replays and differs in the step count)
  return !((int)(key >> 32) == a.health_tag && (a.t_dev == nullptr || (int)(unsigned)key == (int)a.t_dev[0]));
}

// hmask: health_mask(a) of the launch; when an earlier launch has raised a fault nothing is stored
__device__ __forceinline__ void adam_element(const AdamTarget& a, const MobodyMlpLayout& L, long long j, float g,
                                             const float* sm2 = nullptr, int hmask = 0) {
  AdamConsts c = a.c;
  if (a.t_dev != nullptr) {                         // graph replay: the step count lives in device memory
    if (sm2 != nullptr) {
      c.step_size = sm2[0]; c.bc2_sqrt = sm2[1];
    } else {
      const double t = (double)a.t_dev[0];
      c.step_size = (float)((double)a.lr / (1.0 - pow(0.9, t)));
      c.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, t));
    }
  }
  const float gj = g * c.gscale;
  const float m0 = a.m[j];
  const float mj = m0 + ADAM_W1 * (gj - m0);
  const float vj = ADAM_B2 * a.v[j] + ADAM_W2 * (gj * gj);
  const float pj = a.p[j] - c.step_size * (mj / (sqrtf(vj) / c.bc2_sqrt + ADAM_EPS));
  if (hmask != 0 && health_foreign(a)) return;
  a.m[j] = mj; a.v[j] = vj;
  a.p[j] = pj;
  float tj = 0.f;
  if (a.target != nullptr) { tj = c.tau * pj + c.one_minus_tau * a.target[j]; a.target[j] = tj; }      // update_target :183-187
  if (a.blob_T != nullptr || a.target_T != nullptr) {   // keep the transposes / bf16 planes the kernels stream in sync
    const int mem = (int)(j / L.member_floats);
    const long long o = j - (long long)mem * L.member_floats;
    const long long ti = t_blob_index(L, o);
    if (ti >= 0 && a.blob_T != nullptr) a.blob_T[(long long)mem * L.t_member_floats + ti] = pj;
    if (o >= L.w2 && o < L.b2 && a.precision >= 0) {  // a W2 element (wide storage): its planes (precision < 0: nobody streams them)
      const long long oo = o - L.w2, g = oo >> 2;
      const int k = (int)(g / HID) * 4 + (int)(oo & 3), n = (int)(g % HID);
      if (a.blob_T != nullptr) write_w2_planes(a.blob_T + (long long)mem * L.t_member_floats, L, k, n, pj, a.precision);
      if (a.target_T != nullptr && a.target != nullptr) write_w2_planes(a.target_T + (long long)mem * L.t_member_floats, L, k, n, tj, a.precision);
      health_after_update(a, pj, a.blob_T != nullptr, tj, a.target_T != nullptr && a.target != nullptr);
      return;
    }
  }
  health_after_update(a, pj, false, 0.f, false);
}

int launch_adam(const AdamTarget& a, const float* g, const MobodyMlpLayout& L, hipStream_t st);      // k_adam over one packed MLP

// Final reduction of per-workgroup loss partials, done by one extra workgroup of k_grad_reduce (saves a launch).
//   kind 1 (critic): out[0] = scale * sum parts[k]
//   kind 2 (actor):  parts = pairs (sum -min q, sum w*(pi-a)^2);  bc = s1/ntg_a;
//                    out[0] = p_w * s0 / ng + bc_coef * bc, out[1] = bc,  p_w = scale_q ? weight/(stats[0]/ng) : 1
struct LossFinal {
  int kind, nparts, scale_q;
  float scale, weight, bc_coef, ng, ntg_a;
  const float* parts; const float* stats; float* out;
};

struct GradReduceArgs {
  MobodyMlpLayout L;
  const float* slabs; long long slab_stride; int nsplit;
  const float* dbp; int ntiles;
  float* grad;          // may be null when `adam.on` (nobody reads the gradient blob on one GPU)
  LossFinal loss;       // kind 0: none
  AdamTarget adam;      // on = 0: none
  const float* bc_dev;  // {step_size, bc2_sqrt} of adam.t_dev[0], formed by the weight-gradient launch in front, or null
};
int launch_grad_reduce(const GradReduceArgs& a, hipStream_t st);
// dW1, dW2, dW3 of one packed MLP (one merged split-K launch) + the deterministic slab / bias-partial reduction, optionally with
// the optimizer step fused.
struct Mlp3WgradArgs {
  MobodyMlpLayout L;
  long long rows;
  int nsplit;              // split-K factor the slabs were sized for (wgrad_nsplit)
  const float* x;          // what the forward saved: [.][rows][Kp1] input rows; x_mstride 0 = shared by the members, rows * Kp1 = per member
  long long x_mstride;
  const float *h1, *h2;    // [members][rows][256]
  const int* e_h1;         // f16x2: h1 holds the saved fp16 planes, e_h1 their 32-row tiles' exponents (read in that mode only)
  const float *dz3, *dz2, *dz1;    // what the backward left (Mlp3BwdArgs); f16x2: dz2 holds planes, e_dz2 their exponents
  const float* dbp;
  int ntiles;              // row tiles of dbp
  const int* e_dz2;
  float* slabs;            // scratch: [nsplit] partial slabs in the gradient-blob layout
  float* bc_ws;            // two floats of workspace (or null).  With a fused optimizer step on a device step count, the weight-gradient
                           // launch leaves the bias corrections there and k_grad_reduce takes them as a uniform load instead of forming
                           // them behind a barrier.
  float* grad;             // result: the gradient blob (may be null when adam.on), the loss scalars (kind 0: none), the fused step
  LossFinal loss;
  AdamTarget adam;
  int prec;
  int bc_ready;            // bc_ws already holds the constants of adam.t_dev[0] (an earlier launch formed them): the weight-gradient
                           // launch does not
};
int mlp3_weight_grads(const Mlp3WgradArgs& a, hipStream_t st);

// ---- host side: the one place an Mlp3WgradArgs is filled, one helper per group of fields (as for Mlp3BwdArgs above) ----
inline Mlp3WgradArgs wgrad_net(const MobodyMlpLayout& L, long long rows, int nsplit) {
  Mlp3WgradArgs g{};
  g.L = L; g.rows = rows; g.nsplit = nsplit;
  return g;
}
// e_h1 / e_dz2 (below): the exponent arrays of the f16x2 mode.  Callers pass them whatever the precision: mlp3_weight_grads reads
// them in the f16x2 mode alone, every other mode takes h1 / dz2 as fp32 rows.
inline void wgrad_set_saves(Mlp3WgradArgs& g, const float* x, long long x_mstride, const float* h1, const float* h2, const int* e_h1 = nullptr) {
  g.x = x; g.x_mstride = x_mstride; g.h1 = h1; g.h2 = h2; g.e_h1 = e_h1;
}
inline void wgrad_set_grads(Mlp3WgradArgs& g, const float* dz3, const float* dz2, const float* dz1, const float* dbp, int ntiles,
                            const int* e_dz2 = nullptr) {
  g.dz3 = dz3; g.dz2 = dz2; g.dz1 = dz1; g.dbp = dbp; g.ntiles = ntiles; g.e_dz2 = e_dz2;
}
inline void wgrad_set_scratch(Mlp3WgradArgs& g, float* slabs, float* bc_ws) { g.slabs = slabs; g.bc_ws = bc_ws; }
inline void wgrad_set_result(Mlp3WgradArgs& g, float* grad, const LossFinal& loss, const AdamTarget& adam, int prec) {
  g.grad = grad; g.loss = loss; g.adam = adam; g.prec = prec;
}

// split-K factor (workgroups along the row dimension) used for a batch of `rows`: 24 output tiles x nsplit x members
// workgroups should reach ~3 per CU (768), so a one-member net splits twice as fine as a twin net
inline int wgrad_nsplit(long long rows, int members) {
  const int cap = members == 1 ? 32 : members == 2 ? 16 : (32 / members > 1 ? 32 / members : 1);   // 7 members: 4
  long long s = rows / (members == 1 ? 128 : 256);
  if (s < 1) s = 1;
  if (s > cap) s = cap;
  while (rows > 2048LL * 4 * s) s *= 2;             // a wave's row slice spans at most 64 tiles of 32 rows (wgrad_tile_f16)
  return (int)s;
}

// The training scratch of one net: what its forward saves (x .. d2, e_h1: only in a record carved with them -- the pre-training
// nets; Swish derivatives d1 / d2), what its backward leaves and what its weight-gradient launch needs.  h1 and dz2 of a record with
// saves span rows32 rows: in the f16x2 mode they hold fp16 planes of whole 32-row tiles (same bytes) and e_h1 / e_dz2 the tiles'
// exponents.
struct NetScratch {
  float *x, *h1, *h2, *d1, *d2;
  float *dz2, *dz1, *dbp, *slabs;
  int *e_h1, *e_dz2;
  long long rows, rows32;
  int nsplit, ntiles;
};
// take(n) hands out n floats of the workspace (or null while it is only being sized).  dbp_np3: the output width the bias partials
// are sized for (>= L.Np3).
template <class Take>
inline NetScratch carve_net(const MobodyMlpLayout& L, long long rows, bool saves, int dbp_np3, Take&& take) {
  NetScratch s{};
  const long long M = L.members;
  s.rows = rows; s.rows32 = (rows + 31) & ~31LL;
  s.ntiles = (int)cdiv(rows, MLP_TILE_ROWS); s.nsplit = wgrad_nsplit(rows, L.members);
  if (saves) {
    s.x = take(M * rows * L.Kp1);
    s.h1 = take(M * s.rows32 * HID); s.h2 = take(M * rows * HID); s.d1 = take(M * rows * HID); s.d2 = take(M * rows * HID);
    s.e_h1 = reinterpret_cast<int*>(take(M * s.ntiles)); s.e_dz2 = reinterpret_cast<int*>(take(M * s.ntiles));
  }
  s.dz2 = take(M * (saves ? s.rows32 : rows) * HID); s.dz1 = take(M * rows * HID);
  s.dbp = take((long long)s.ntiles * M * (2 * HID + dbp_np3));
  s.slabs = take(((L.total_floats + 3) & ~3LL) * s.nsplit);
  return s;
}

}  // namespace mobody
