// Fused 3-layer MLP forward: one workgroup = one 32-row tile (MLP_TILE_ROWS, layers.h) x one member, all three
// GEMMs on fp32 MFMA with the activations resident in LDS (written to HBM only when the backward pass asks for
// them: x / h1 / h2 for the weight gradients, 32 B/row of ReLU sign words for the masks).  k_mlp3_fwd2 runs two
// independent networks in one launch.  Roofline: MFMA f32 (2*(Kp1+256+Np3)*256 FLOP per row against (in+out)*4
// bytes per row -> AI > 1000 F/B); weights (<= 340 KB per member) stream from L2.
#include <stdlib.h>

#include "common.h"
#include "layers.h"

namespace mobody {

constexpr int TB = MLP_TILE_ROWS;               // rows of a workgroup's tile

// Output layer of the forward (256 -> nout <= 16*NT) through the K-split narrow layer; NT = 0: generic row-split path.
template <int ACT, int NT>
__device__ __forceinline__ void mlp3_fwd_tail(const Mlp3FwdArgs& a, int m, float* Xs, WideRing& ring, float* h2,
                                              uint32_t* mask2, float* out, long long row0, int rows_here) {
  const float* w3 = a.w3 + m * a.sw3;
  const float* b3 = a.b3 + m * a.sb3;
  const bool full = rows_here == TB;
  auto save_h2 = [=](auto guarded, int row, int col, float y) {
    if (h2 != nullptr && (!decltype(guarded)::value || row < rows_here)) h2[row * HID + col] = y;
  };
  auto emit = [&](int row, int col, float v, float bias) { fwd_emit(a, out, row0, rows_here, row, col, v, bias); };
  if constexpr (NT > 0) {
    NarrowRegs<NT> br;
    // b3 of this thread's output columns: element e = threadIdx.x + 256 k has column e % (16 NT), the same for all k
    const int mycol = threadIdx.x % (16 * NT);
    float bias;
    const bool one = fwd_rank1<NT>(a);             // a one-output net: the fma chain of tile.h narrow_run_one (as fwd_bf_tile.h)
    wide_layer<ACT, MLP_MT>(Xs, a.w2 + m * a.sw2, a.b2 + m * a.sb2, HID, ring, save_h2, [&] {
      if (one) br.b[0][0] = narrow_prefetch_one(w3, 16 * NT);
      else narrow_prefetch<NT>(w3, 16 * NT, br);
      bias = b3[mycol < a.nout ? mycol : 0];
    }, mask2, full, (rows_here + 31) / 32);
    TR(4);
    if (one) narrow_run_one<TB / 16>(Xs, br.b[0][0], [&](int row, int col, float v) { emit(row, col, v, bias); });
    else narrow_run<TB / 16, NT>(Xs, br, [&](int row, int col, float v) { emit(row, col, v, bias); });
  } else {
    wide_layer<ACT, MLP_MT>(Xs, a.w2 + m * a.sw2, a.b2 + m * a.sb2, HID, ring, save_h2, [] {}, mask2, full, (rows_here + 31) / 32);
    TR(4);
    narrow_layer(Xs, w3, HID, a.Np3, [&](int row, int col, float v) { emit(row, col, v, b3[col < a.nout ? col : 0]); }, TB);
  }
}

// NT: 16-column tiles of the output layer handled by the K-split narrow layer (Np3 == 16*NT), or 0 = any Np3.
// GATHER: the input tile comes straight from the replay rings (layers.h fwd_gather_tile); fg / second: the stage's arguments and
// which net of the pair this tile belongs to
template <int ACT, int NT, bool GATHER = false>
__device__ __forceinline__ void mlp3_fwd_tile(const Mlp3FwdArgs& a, int m, float* Xs, const FwdGather* fg = nullptr, bool second = false) {
  const long long row0 = (long long)blockIdx.x * TB;
  const int rows_here = (int)min((long long)TB, a.rows - row0);
  const float* w1 = a.w1 + m * a.sw1;
  const float* w2 = a.w2 + m * a.sw2;
  TR(0);
  WideRing ring;
  wide_prefetch(w1, a.Kp1, ring);                 // W1 fragments travel while the input tile is fetched
  if constexpr (GATHER) tile_zero_cols(Xs, fwd_gather_tile(*fg, second, Xs, row0, rows_here), a.Kp1, TB);
  else tile_zero_cols(Xs, fwd_load_sources(a, m, Xs, row0, rows_here), a.Kp1, TB);
  lds_barrier();
  TR(1);
  fwd_save_x(a, m, Xs, row0, rows_here);
  if constexpr (GATHER) fwd_gather_save(*fg, second, m, Xs, row0, rows_here);
  const FwdTileOut t = fwd_tile_out(a, m, row0);
  float* h1 = t.h1;
  wide_layer<ACT, MLP_MT>(Xs, w1, a.b1 + m * a.sb1, a.Kp1, ring,
                      [=](auto guarded, int row, int col, float y) {
                        if (h1 != nullptr && (!decltype(guarded)::value || row < rows_here)) h1[row * HID + col] = y;
                      },
                      [&] { wide_prefetch(w2, HID, ring); }, t.mask1, rows_here == TB, (rows_here + 31) / 32);
  TR(2);
  mlp3_fwd_tail<ACT, NT>(a, m, Xs, ring, t.h2, t.mask2, t.out, row0, rows_here);
  TR(5);
}

template <int ACT, int NT>
__global__ __launch_bounds__(NTHREADS, 2) void k_mlp3_fwd(Mlp3FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  mlp3_fwd_tile<ACT, NT>(a, blockIdx.y, Xs);
}

// Two independent networks in ONE launch (blockIdx.y < members_a -> net a, else net b): Q(s,a) with pi(s') in the
// critic phase, Q(s_t,a_t) with pi(s) in the actor phase.  A 1-member launch of 10 k rows is only 320 workgroups
// (1.25 per CU: half the chip idles through the second round); merged with the twin-Q launch the grid is ~3.5
// workgroups per CU and one generation shorter.  The argument block is SELECTED (scalar selects), not branched on:
// two inlined copies of the tile body in an if/else made hipcc keep both live (190 VGPRs, half the occupancy).
template <int ACT, int NT>
__global__ __launch_bounds__(NTHREADS, 2) void k_mlp3_fwd2(Mlp3FwdArgs a, Mlp3FwdArgs b, int members_a) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const bool second = (int)blockIdx.y >= members_a;
  const Mlp3FwdArgs s = second ? b : a;
  if ((long long)blockIdx.x * TB >= s.rows) return;              // the two nets may differ in rows (grid.x = max)
  mlp3_fwd_tile<ACT, NT>(s, second ? (int)blockIdx.y - members_a : (int)blockIdx.y, Xs);
}

// k_mlp3_fwd2 with the gathering input stage (a kernel of its own: the stage's arguments are a fourth kernel argument)
template <int NT>
__global__ __launch_bounds__(NTHREADS, 2) void k_mlp3_fwd2_gather(Mlp3FwdArgs a, Mlp3FwdArgs b, int members_a, FwdGather fg) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const bool second = (int)blockIdx.y >= members_a;
  const Mlp3FwdArgs s = second ? b : a;
  if ((long long)blockIdx.x * TB >= s.rows) return;
  mlp3_fwd_tile<ACT_RELU, NT, true>(s, second ? (int)blockIdx.y - members_a : (int)blockIdx.y, Xs, &fg, second);
}

template <int ACT, int NT>
static int launch_fwd_t(const Mlp3FwdArgs& a, int members, hipStream_t stream) {
  size_t lds = (size_t)TB * LDX * sizeof(float);
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_fwd<ACT, NT>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  dim3 grid((unsigned)cdiv(a.rows, TB), (unsigned)members);
  ProfScope prof(PROF_MLP_FWD, stream);
  hipLaunchKernelGGL((k_mlp3_fwd<ACT, NT>), grid, dim3(NTHREADS), lds, stream, a);
  MB_LAUNCH_OK("k_mlp3_fwd");
  return 0;
}

template <int NT>
static int launch_fwd2_t(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, hipStream_t stream) {
  size_t lds = (size_t)TB * LDX * sizeof(float);
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_fwd2<ACT_RELU, NT>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  const long long rows = a.rows > b.rows ? a.rows : b.rows;
  dim3 grid((unsigned)cdiv(rows, TB), (unsigned)(members_a + members_b));
  ProfScope prof(PROF_MLP_FWD, stream);
  hipLaunchKernelGGL((k_mlp3_fwd2<ACT_RELU, NT>), grid, dim3(NTHREADS), lds, stream, a, b, members_a);
  MB_LAUNCH_OK("k_mlp3_fwd2");
  return 0;
}

static int launch_fwd2_gather(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg, hipStream_t stream) {
  size_t lds = (size_t)TB * LDX * sizeof(float);
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_fwd2_gather<1>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  dim3 grid((unsigned)cdiv(a.rows, TB), (unsigned)(members_a + members_b));
  ProfScope prof(PROF_MLP_FWD, stream);
  hipLaunchKernelGGL(k_mlp3_fwd2_gather<1>, grid, dim3(NTHREADS), lds, stream, a, b, members_a, fg);
  MB_LAUNCH_OK("k_mlp3_fwd2_gather");
  return 0;
}

// ReLU nets a and b, both non-empty and of one output width, in one launch
static int launch_fwd_pair(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, hipStream_t stream) {
  return dispatch_out_width(a.Np3, [&](auto nt) { return launch_fwd2_t<decltype(nt)::value>(a, members_a, b, members_b, stream); });
}

template <int ACT>
static int launch_fwd_act(const Mlp3FwdArgs& a, int members, hipStream_t stream) {
  return dispatch_out_width(a.Np3, [&](auto nt) { return launch_fwd_t<ACT, decltype(nt)::value>(a, members, stream); });
}

static int launch_mlp3_fwd(const Mlp3FwdArgs& a, int members, int act, hipStream_t stream) {
  return act == ACT_SWISH ? launch_fwd_act<ACT_SWISH>(a, members, stream) : launch_fwd_act<ACT_RELU>(a, members, stream);
}

// the other two back ends: split precision (mlp_fwd_bf.hip: a non-empty with w2_planes; b a ReLU net that shares the launch, or
// members_b = 0) and the fp32 training forward of a Swish net, which also saves the derivatives (pretrain.hip)
int launch_mlp3_fwd_bf(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, int act, int prec, hipStream_t st);
int launch_fwd_train(const Mlp3FwdArgs& a, int members, hipStream_t st);

// Two nets share a launch when both are ReLU nets of one output-layer width (the merged kernels are specialised on it), or --
// f16x2 only, which has the two mixed instantiations -- of widths 16 and 32: a twin-Q next to an actor of more than 16 actions.
static bool nets_share_launch(const Mlp3FwdArgs& a, const Mlp3FwdArgs& b, int act, int prec) {
  if (act != ACT_RELU) return false;
  return a.Np3 == b.Np3 || (prec == PREC_F16X2 && ((a.Np3 == 16 && b.Np3 == 32) || (a.Np3 == 32 && b.Np3 == 16)));
}

int launch_mlp3_forward(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, int act, int prec, hipStream_t st) {
  auto one = [&](const Mlp3FwdArgs& x, int members) {
    if (prec != PREC_F32) return launch_mlp3_fwd_bf(x, members, Mlp3FwdArgs{}, 0, act, prec, st);
    return x.save_d1 != nullptr ? launch_fwd_train(x, members, st) : launch_mlp3_fwd(x, members, act, st);
  };
  const bool has_a = members_a > 0 && a.rows > 0, has_b = members_b > 0 && b.rows > 0;
  if (!has_a || !has_b) return has_a ? one(a, members_a) : has_b ? one(b, members_b) : 0;
  if (!nets_share_launch(a, b, act, prec)) {
    int rc = one(a, members_a);
    return rc ? rc : one(b, members_b);
  }
  return prec == PREC_F32 ? launch_fwd_pair(a, members_a, b, members_b, st) : launch_mlp3_fwd_bf(a, members_a, b, members_b, act, prec, st);
}

int launch_mlp3_forward_gather(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg,
                               int prec, hipStream_t st) {
  const GatherArgs& g = fg.g;
  const long long N = g.start[g.nbuf];
  if (N <= 0 || members_a <= 0 || members_b <= 0) return fail(MOBODY_E_ARG, "launch_mlp3_forward_gather: needs both nets and a non-empty minibatch");
  if (a.rows != N || b.rows != N) return fail(MOBODY_E_ARG, "launch_mlp3_forward_gather: the nets run on %lld / %lld rows, the minibatch has %lld", a.rows, b.rows, N);
  for (int k = 0; k < g.nbuf; ++k)
    if (!g.packed[k] && g.start[k + 1] > g.start[k]) return fail(MOBODY_E_ARG, "launch_mlp3_forward_gather: source %d is not a packed ring", k);
  if (fg.off[0] != 0 || fg.n[0] != g.S + g.A || fg.off[1] != g.S + g.A || fg.n[1] != g.S)
    return fail(MOBODY_E_ARG, "launch_mlp3_forward_gather: net a reads state | action, net b next_state");
  auto chunks = [](int off, int n) { return ((off + n + 3) >> 2) - (off >> 2); };
  // the instances that exist: a one-output twin-Q (NT = 1) next to an actor of the same output-layer width, or -- f16x2 -- of width 32
  const bool built = a.Np3 == 16 && (b.Np3 == 16 || (prec == PREC_F16X2 && b.Np3 == 32)) && nets_share_launch(a, b, ACT_RELU, prec) &&
                     chunks(fg.off[0], fg.n[0]) <= 16 * FWD_GATHER_NQ && chunks(fg.off[1], fg.n[1] + 2) <= 16 * FWD_GATHER_NQ;
  if (!built) {
    int rc = launch_gather(g, N, st);
    return rc ? rc : launch_mlp3_forward(a, members_a, b, members_b, ACT_RELU, prec, st);
  }
  return prec == PREC_F32 ? launch_fwd2_gather(a, members_a, b, members_b, fg, st) : launch_mlp3_fwd_bf_gather(a, members_a, b, members_b, fg, prec, st);
}

// The merged launch takes what the f16x2 gathering kernel takes (launch_mlp3_forward_gather, `built`) when target-Q reads
// exactly pi(s')'s rows and outputs and a tile's [s' | a'] rows fit behind the image at four workgroups per CU (S + A <= 59:
// ant, 111 + 8, and pen, 45 + 24, stay on two launches).
static bool critic_forward_merges(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi, const FwdGather& fg,
                                  int prec) {
#ifdef MOBODY_TWO_CRITIC_FWD
  return false;                                    // A/B aid (build.py MOBODY_EXTRA_FLAGS): the two launches this one replaces
#else
  const GatherArgs& g = fg.g;
  const long long N = g.start[g.nbuf];
  auto chunks = [](int off, int n) { return ((off + n + 3) >> 2) - (off >> 2); };
  if (prec != PREC_F16X2 || N <= 0 || q.rows != N || pn.rows != N || qt.rows != N || (pi != nullptr && pi->rows != N)) return false;
  for (int k = 0; k < g.nbuf; ++k)
    if (!g.packed[k] && g.start[k + 1] > g.start[k]) return false;
  if (fg.off[0] != 0 || fg.n[0] != g.S + g.A || fg.off[1] != g.S + g.A || fg.n[1] != g.S) return false;
  if (q.Np3 != 16 || qt.Np3 != 16 || (pn.Np3 != 16 && pn.Np3 != 32) || chunks(0, g.S + g.A) > 16 * FWD_GATHER_NQ ||
      chunks(g.S + g.A, g.S + 2) > 16 * FWD_GATHER_NQ)
    return false;
  // target-Q is the twin-Q of [next_state | pn's output], whole rows, no saves; pi(s') is a plain tanh actor
  if (qt.Kp1 != q.Kp1 || qt.n[0] != g.S || qt.n[1] != g.A || qt.n[2] != 0 || qt.src[1] != pn.out || pn.nout != g.A ||
      pn.out_ld != g.A || pn.resid != nullptr || qt.save_x || qt.save_h1 || qt.save_h1p || qt.save_h2 || qt.mask1 || qt.mask2)
    return false;
  if (pi != nullptr && (pi->Np3 != pn.Np3 || pi->Kp1 != pn.Kp1 || pi->n[0] != g.S || pi->n[1] + pi->n[2] != 0)) return false;
  return critic_fwd_bf_lds(g.S, g.A) <= CRITIC_FWD_LDS_MAX;
#endif
}

int launch_critic_forward_gather(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi,
                                 const FwdGather& fg, int prec, hipStream_t st, const Mlp3BwdArgs* bq, int* tickets, bool* chained) {
  if (chained != nullptr) *chained = false;
  if (critic_forward_merges(q, pn, qt, pi, fg, prec)) return launch_critic_fwd_bf(q, pn, qt, pi, fg, st, bq, tickets, chained);
  int rc = launch_mlp3_forward_gather(q, 2, pn, 1, fg, prec, st);
  if (rc) return rc;
  return pi != nullptr ? launch_mlp3_forward(qt, 2, *pi, 1, ACT_RELU, prec, st) : launch_mlp3_forward(qt, 2, ACT_RELU, prec, st);
}

}  // namespace mobody

using namespace mobody;

extern "C" int mobody_mlp3_forward(const float* blob, const float* blob_T, int precision, int in_dim, int out_dim,
                                   int members, const float* src0, int n0, const float* src1, int n1, int64_t rows,
                                   int out_mode, float max_action, float* out, float* save_x, float* save_h1,
                                   float* save_h2, void* stream) {
  MobodyMlpLayout L;
  int rc = mobody_mlp_layout(in_dim, out_dim, members, &L);
  if (rc) return rc;
  MB_REQUIRE(rows >= 0, "mobody_mlp3_forward: rows < 0");
  if (rows == 0) return 0;
  MB_REQUIRE(blob && src0 && out, "mobody_mlp3_forward: null pointer");
  MB_REQUIRE(n0 + n1 == in_dim && n0 > 0 && n1 >= 0 && (n1 == 0 || src1), "mobody_mlp3_forward: n0+n1=%d != in_dim=%d", n0 + n1, in_dim);
  rc = check_precision("mobody_mlp3_forward", precision, blob_T != nullptr);
  if (rc) return rc;
  Mlp3FwdArgs a = fwd_net(blob, L, rows);
  fwd_set_src(a, 0, src0, n0, n0);
  fwd_set_src(a, 1, src1, n1, n1);
  fwd_set_out(a, out, out_mode, max_action);
  fwd_set_saves(a, save_x, 0, save_h1, nullptr, save_h2);
  if (precision != PREC_F32) fwd_set_planes(a, blob_T, L);
  return launch_mlp3_forward(a, members, ACT_RELU, precision, as_stream(stream));
}
