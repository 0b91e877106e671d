// Layer-level device helpers built on tile.h, and the argument block of the generic fused
// 3-layer MLP forward kernel (in -> 256 -> 256 -> out) used for:
//   actor / twin-Q / target twin-Q / V     (ReLU;  mobody.py:35-83)
//   the ensemble reward head               (Swish; mobody_module.py:295-302)
//   the DARA classifier heads              (ReLU;  mobody.py:11-33)
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/mobody_hip.h"
#include "gather.h"
#include "tile.h"

namespace mobody {

// One hidden layer in place on the LDS image: X <- act(X[:, :Kp] * W + b); `extra(row, col, y)` sees every output.
// `ring` holds wide_prefetch(W, Kp); `between()` runs after the last MFMA and before the epilogue -- the place to
// request the NEXT layer's first weight fragments (the ring's registers are free again), so their L2/HBM round trip
// overlaps this layer's barrier + epilogue instead of stalling the next GEMM.
// `mask` (optional): this tile's [groups][256] words, `mask_groups` of them real; bit r of word (g, col) =
// [y(row 32 g + r, col) > 0].  The backward
// pass of a ReLU net needs only these signs, 32 B per row instead of the 1 KB activation row.
template <int ACT, int MT, class Extra, class Between>
__device__ __forceinline__ void wide_layer(float* Xs, const float* __restrict__ W, const float* __restrict__ b, int Kp,
                                           WideRing& ring, Extra&& extra, Between&& between, uint32_t* mask = nullptr,
                                           bool full = false, int mask_groups = 1 << 30) {
  // the wave's two bias values (columns 64w + 32nt + lane&31): requested before the GEMM, consumed after it
  const float bias0 = b[64 * wave_col() + (lane_id() & 31)], bias1 = b[64 * wave_col() + 32 + (lane_id() & 31)];
  f32x16 acc[MT][2];
  wide_zero<MT>(acc);
  wide_gemm<MT>(Xs, W, Kp, acc, ring);
  if (Kp == HID) TR(3);
  between();
  lds_barrier();                         // every wave has finished reading the old image
  // `full` (wave uniform): every row of the tile is a real row, so `extra` may skip its row guard -- a per-element
  // row < rows_here test costs a v_cmp plus exec-mask save/restore around each of the 32 stores of a lane
  if (full) {
    wide_foreach<MT>(acc, [&](int row, int col, float v) {
      const float y = activate<ACT>(v + ((col & 32) ? bias1 : bias0));
      Xs[row * LDX + col] = y;
      extra(std::false_type{}, row, col, y);
    });
  } else {
    wide_foreach<MT>(acc, [&](int row, int col, float v) {
      const float y = activate<ACT>(v + ((col & 32) ? bias1 : bias0));
      Xs[row * LDX + col] = y;
      extra(std::true_type{}, row, col, y);
    });
  }
  if (mask != nullptr) {
    const int i = lane_id() & 31, hh = lane_id() >> 5;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const float bias = nt ? bias1 : bias0;
        uint32_t word = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          word |= (uint32_t)(activate<ACT>(acc[mt][nt][r] + bias) > 0.f) << ((r & 3) + 8 * (r >> 2) + 4 * hh);
        word |= (uint32_t)__shfl_xor((int)word, 32);        // the other lane half holds the other 16 rows
        // 32-row groups past the end of the batch have no words (a taller tile's last groups would land in the next member)
        if (hh == 0 && mt < mask_groups) mask[mt * HID + 64 * wave_col() + 32 * nt + i] = word;
      }
  }
  lds_barrier();
}

template <int ACT, int MT, class Extra>
__device__ __forceinline__ void wide_layer(float* Xs, const float* __restrict__ W, const float* __restrict__ b, int Kp,
                                           Extra&& extra) {
  WideRing ring;
  wide_prefetch(W, Kp, ring);
  wide_layer<ACT, MT>(Xs, W, b, Kp, ring, extra, [] {});
}

// Training forward of a Swish layer: X <- y = z*sigmoid(z), z = X*W + b, and `extra(guard, row, col, y, d)` also sees
// d = dy/dz = sig*(1 + z*(1 - sig)) (saved for the backward pass: Swish is not invertible, so the sign words of the ReLU
// nets do not carry over; mobody_module.py:9-15).
template <int MT, class Extra, class Between>
__device__ __forceinline__ void wide_layer_swish_d(float* Xs, const float* __restrict__ W, const float* __restrict__ b,
                                                   int Kp, WideRing& ring, Extra&& extra, Between&& between, bool full) {
  const float bias0 = b[64 * wave_col() + (lane_id() & 31)], bias1 = b[64 * wave_col() + 32 + (lane_id() & 31)];
  f32x16 acc[MT][2];
  wide_zero<MT>(acc);
  wide_gemm<MT>(Xs, W, Kp, acc, ring);
  between();
  lds_barrier();
  auto body = [&](auto guarded) {
    wide_foreach<MT>(acc, [&](int row, int col, float v) {
      const float z = v + ((col & 32) ? bias1 : bias0);
      const float sig = fast_rcp(1.f + __expf(-z));
      const float y = z * sig;
      Xs[row * LDX + col] = y;
      extra(guarded, row, col, y, sig * (1.f + z * (1.f - sig)));
    });
  };
  if (full) body(std::false_type{});
  else body(std::true_type{});
  lds_barrier();
}

struct NoExtra {
  template <class Guard>
  __device__ __forceinline__ void operator()(Guard, int, int, float) const {}
};

struct Mlp3FwdArgs {
  const float* src[3];      // concatenated inputs, src[k] is [rows][n[k]] with leading dim ld[k]; unused: n = 0
  int ld[3], n[3];
  long long src_ms[3];      // member stride of src[k] in floats: 0 = one input shared by all members (the hot path),
                            // rows*ld = per-member rows (dynamics pre-training / validation: [E][rows][n])
  long long x_ms;           // member stride of save_x: 0 = written once by member 0, else every member saves its own
  const float *w1, *b1, *w2, *b2, *w3, *b3;   // member 0
  long long sw1, sb1, sw2, sb2, sw3, sb3;     // member strides (floats)
  int Kp1, Np3, nout;
  long long rows;
  float* out;               // out[m*out_mstride + row*out_ld + c], c < nout
  long long out_mstride;
  int out_ld;
  float* save_x;            // [rows][Kp1]           (optional, written by member 0)
  float* save_h1;           // [members][rows][256]  (optional)
  float* save_h2;
  uint32_t* mask1;          // [members][ceil(rows/32)][256] sign bits of h1 / h2 (optional, see wide_layer)
  uint32_t* mask2;
  const unsigned short* w2_planes;   // split-precision modes: bf16 planes of W2, member 0 ([3][32][256][8] bf16 per member, tile_bf.h)
  long long planes_ms;               // member stride of w2_planes in bf16 elements
  float* save_d1;           // [members][rows][256] Swish derivative at the pre-activations of layers 1 / 2 (training
  float* save_d2;           // forward of the ensemble nets only: k_mlp3_fwd_train)
  unsigned short* save_h1p; // f16 mode, instead of save_h1: the layer-1 activations as the two fp16 planes the weight-gradient GEMM
  long long h1p_ms;         // reads ([member][2 planes][rows32 / 8][256][8], layers_bf.h PlaneSave; member stride h1p_ms and plane
  long long h1p_plane;      // stride h1p_plane in 16-bit elements, rows32 = rows rounded up to 32) and
  int* save_e1;             // [members][ceil(rows / 32)] the tiles' scale exponents
  int out_mode;             // 0 raw, 1 max_action*tanh
  const float* resid;       // optional: out[m][row][c] += resid[row*resid_ld + c] (shared by the members; mopo dynamics: s + f(s,a))
  int resid_ld;
  float max_action;
};

// ---- host side: the one place an Mlp3FwdArgs is filled; each helper owns one group of fields ----
// 16-bit planes of the three 256 x 256 ensemble layers (mobody_dyn_planes): [layer 0..2 = zs2, transition2, reward_model2][member]
// [3 planes][65536]; elements per (layer, member) and the offset of one
constexpr long long DYN_PLANE_MEMBER = 3LL * HID * HID;
__host__ __device__ inline long long dyn_planes_off(int layer, int member) { return ((long long)layer * NENS + member) * DYN_PLANE_MEMBER; }

// weights, member strides and dims of a packed MLP (mobody_mlp_layout) on `rows` rows; everything else zero
inline Mlp3FwdArgs fwd_net(const float* blob, const MobodyMlpLayout& L, long long rows) {
  Mlp3FwdArgs a{};
  a.w1 = blob + L.w1; a.b1 = blob + L.b1; a.w2 = blob + L.w2; a.b2 = blob + L.b2; a.w3 = blob + L.w3; a.b3 = blob + L.b3;
  a.sw1 = a.sb1 = a.sw2 = a.sb2 = a.sw3 = a.sb3 = L.member_floats;
  a.Kp1 = L.Kp1; a.Np3 = L.Np3; a.nout = L.out_dim; a.rows = rows;
  return a;
}
// W2's planes in the net's T blob (what the split-precision forward streams)
inline void fwd_set_planes(Mlp3FwdArgs& a, const float* blob_T, const MobodyMlpLayout& L) {
  a.w2_planes = reinterpret_cast<const unsigned short*>(blob_T + L.w2p);
  a.planes_ms = 2 * L.t_member_floats;
}
// the ensemble's reward head (reward_model1-3 of the dynamics blob, one output); dyn_planes: the plane blob or null (exact fp32)
inline Mlp3FwdArgs fwd_reward_head(const float* dyn_blob, const MobodyDynLayout& L, const float* dyn_planes, long long rows) {
  Mlp3FwdArgs a{};
  const MobodyLayer &l1 = L.layer[MOBODY_DL_RW1], &l2 = L.layer[MOBODY_DL_RW2], &l3 = L.layer[MOBODY_DL_RW3];
  a.w1 = dyn_blob + l1.w_off; a.b1 = dyn_blob + l1.b_off; a.sw1 = (long long)l1.Kp * l1.Np; a.sb1 = l1.Np;
  a.w2 = dyn_blob + l2.w_off; a.b2 = dyn_blob + l2.b_off; a.sw2 = (long long)l2.Kp * l2.Np; a.sb2 = l2.Np;
  a.w3 = dyn_blob + l3.w_off; a.b3 = dyn_blob + l3.b_off; a.sw3 = (long long)l3.Kp * l3.Np; a.sb3 = l3.Np;
  a.Kp1 = l1.Kp; a.Np3 = l3.Np; a.nout = 1; a.rows = rows;
  if (dyn_planes != nullptr) {
    a.w2_planes = reinterpret_cast<const unsigned short*>(dyn_planes) + dyn_planes_off(2, 0);
    a.planes_ms = DYN_PLANE_MEMBER;
  }
  return a;
}
// input k: [rows][ld] of which n columns are read; ms = 0: shared by the members, else the member stride in floats
inline void fwd_set_src(Mlp3FwdArgs& a, int k, const float* src, int ld, int n, long long ms = 0) {
  a.src[k] = src; a.ld[k] = ld; a.n[k] = n; a.src_ms[k] = ms;
}
// dense output [members][rows][nout], optionally max_action * tanh (out_mode 1) and + resid[row][c]
inline void fwd_set_out(Mlp3FwdArgs& a, float* out, int out_mode, float max_action, const float* resid = nullptr, int resid_ld = 0) {
  a.out = out; a.out_mstride = a.rows * a.nout; a.out_ld = a.nout;
  a.out_mode = out_mode; a.max_action = max_action; a.resid = resid; a.resid_ld = resid_ld;
}
// what the backward pass wants kept.  x_ms: 0 = x saved once by member 0, else per member.  e1 != null (f16x2) and h1: h1 leaves
// as the two fp16 planes + tile exponents the weight-gradient GEMM reads, not as fp32 rows
inline void fwd_set_saves(Mlp3FwdArgs& a, float* x, long long x_ms, float* h1, int* e1, float* h2, uint32_t* m1 = nullptr,
                          uint32_t* m2 = nullptr, float* d1 = nullptr, float* d2 = nullptr) {
  if (e1 != nullptr && h1 != nullptr) {
    const long long r32 = (a.rows + 31) & ~31LL;
    a.save_h1p = reinterpret_cast<unsigned short*>(h1); a.h1p_plane = r32 * HID; a.h1p_ms = 2 * r32 * HID; a.save_e1 = e1;
    h1 = nullptr;
  }
  a.save_x = x; a.x_ms = x_ms; a.save_h1 = h1; a.save_h2 = h2; a.mask1 = m1; a.mask2 = m2; a.save_d1 = d1; a.save_d2 = d2;
}

// The gathering input stage of a paired launch (the train step's first forward, twin-Q(s,a) next to pi(s')): the tiles draw
// and fetch their own ring rows (gather.h) instead of reading a minibatch another launch assembled.  Net k's input tile is
// columns [off[k], off[k] + n[k]) of the packed ring row; `g` also names the minibatch arrays the launch still writes for the
// launches behind it.  Travels as a kernel argument of its own: Mlp3FwdArgs keeps its layout.
struct FwdGather {
  GatherArgs g;
  int off[2], n[2];
};
// net k (0 = a, 1 = b) of the paired launch reads the columns from `off` of the ring row where it read its sources
inline void fwd_set_gather(FwdGather& fg, int k, const Mlp3FwdArgs& a, int off) {
  fg.off[k] = off; fg.n[k] = a.n[0] + a.n[1] + a.n[2];
}
constexpr int FWD_GATHER_NQ = 2;                 // 16-byte chunks a lane holds per row: a tile's part of a ring row is <= 32 chunks

// Output-layer width -> the NT of the kernel instantiations (16-column tiles of the K-split narrow layer; 0 = any width):
// f(std::integral_constant<int, NT>)
template <class F>
inline int dispatch_out_width(int Np3, F&& f) {
  return Np3 == 16 ? f(std::integral_constant<int, 1>{}) : Np3 == 32 ? f(std::integral_constant<int, 2>{})
                                                                     : f(std::integral_constant<int, 0>{});
}

// THE forward launch: net a, optionally net b (members_b = 0: none; either may be empty, rows <= 0), activation `act`, precision id
// (common.h).  It alone decides which kernel runs -- exact fp32 (mlp_fwd.hip), split precision (mlp_fwd_bf.hip), or the fp32
// training forward of a Swish net with derivative saves (pretrain.hip) -- and whether two nets share a launch.
int launch_mlp3_forward(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, int act, int prec, hipStream_t st);
inline int launch_mlp3_forward(const Mlp3FwdArgs& a, int members, int act, int prec, hipStream_t st) {
  return launch_mlp3_forward(a, members, Mlp3FwdArgs{}, 0, act, prec, st);
}

// The same pair of ReLU nets with the gathering input stage: a = twin-Q on state | action, b = the actor on next_state, of
// one minibatch of fg.g (every source a packed ring).  Pairs the gathering kernels do not cover (nets that cannot share a
// launch, ring rows longer than the stage holds) run the stand-alone gather and then the plain launch: same results.
int launch_mlp3_forward_gather(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg,
                               int prec, hipStream_t st);
int launch_mlp3_fwd_bf_gather(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg,
                              int prec, hipStream_t st);

// All forwards of a gathering critic step: q = twin-Q(s,a) with saves, pn = pi(s'), qt = target twin-Q(s', pi(s')) reading pn's
// output, pi = pi(s) with saves or null.  One launch where the merged kernel exists (f16x2, the pairs the gathering kernels
// cover, [s' | a'] rows that fit behind the image: critic_fwd_bf.hip k_critic_fwd_bf); otherwise launch_mlp3_forward_gather(q, pn)
// and then launch_mlp3_forward(qt, pi): same results, bit for bit.
// bq (or null), tickets, chained: the critic backward of the same step (train.h; seed mode 1) and its 2 x row tiles ticket words
// -- where the one-chain form of the merged kernel runs, the backward tiles run inside it (k_critic_chain_bf) and *chained is set:
// the caller then skips launch_mlp3_bwd(bq).
struct Mlp3BwdArgs;
int launch_critic_forward_gather(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi,
                                 const FwdGather& fg, int prec, hipStream_t st, const Mlp3BwdArgs* bq = nullptr, int* tickets = nullptr,
                                 bool* chained = nullptr);
int launch_critic_fwd_bf(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi, const FwdGather& fg,
                         hipStream_t st, const Mlp3BwdArgs* bq = nullptr, int* tickets = nullptr, bool* chained = nullptr);
size_t critic_fwd_bf_lds(int S, int A);          // LDS bytes of a k_critic_fwd_bf workgroup
constexpr size_t CRITIC_FWD_LDS_MAX = 40 * 1024; // four workgroups per CU

// Row-tile height of the fused 3-layer MLP kernels (forward and backward; the callers size the bias partials and the sign
// words by it).  Measured on MI355X (bench.py, S=17/A=6): 32-row tiles (33 KB LDS, ~124 VGPRs -> 4 workgroups = 16 waves
// per CU) beat 64-row tiles (2 workgroups per CU) at every batch size from 2.5 k to 41 k rows (forward 84 vs 73 TFLOP/s at
// 41 k rows, 60 vs 51 at 10 k): occupancy hides the weight-fetch latency better than the 2x weight reuse of the taller tile.
constexpr int MLP_TILE_ROWS = 32;
constexpr int MLP_MT = MLP_TILE_ROWS / 32;       // 32 x 32 MFMA row tiles per wave (the MT of the tile helpers)

// ---- pieces the fp32 and the split-precision forward tiles share (mlp_fwd.hip, mlp_fwd_bf.hip) ----
// Input tile of member m: concat(src0, src1, src2) into columns [0, return value); the caller zero-pads up to Kp1.
__device__ __forceinline__ int fwd_load_sources(const Mlp3FwdArgs& a, int m, float* Xs, long long row0, int rows_here) {
  int c0 = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (a.n[k] > 0) {
      tile_load(Xs, c0, a.src[k] + m * a.src_ms[k] + row0 * a.ld[k], a.ld[k], a.n[k], 0, rows_here, MLP_TILE_ROWS);
      c0 += a.n[k];
    }
  }
  return c0;
}

// ---- gathering input stage (FwdGather): what replaces the tile load, and the minibatch arrays the tile owes ----
// The tile's 32 rows, two per 16-lane group as k_gather_rows<2, .> takes them: lanes 0 and 1 of a group form the source
// pointers of rows g and g + 16 (buffer by start[], then an explicit index or one Philox draw: gather_src) and hand them over
// by shuffle; every lane requests its 16-byte chunks of both rows -- unconditional, from a clamped row and chunk -- before
// the first LDS store.  Only the chunks that hold the tile's own columns travel: [off, off + n) for the twin-Q tiles,
// [off, off + n + 2) for the pi(s') tile, which also owes reward and not_done (they follow next_state in the ring row) and
// stores them straight from the registers.  Xs ends up as tile_load2 / tile_load leave it: rows past the batch are zero.
// The pi(s) tile of the merged critic forward (critic_fwd_bf.hip) reads the state columns alone (FWD_COLS_STATE: the first
// g.S columns of net a's part of the row) and owes no minibatch array; where that launch evaluates pi(s') of a row block twice,
// the second copy fetches the same chunks and leaves reward / not_done to the first (`owes` false).
// PUB: reward / not_done are read by another workgroup of the same launch (tile.h agent_store).
enum FwdGatherCols { FWD_COLS_NET = 0, FWD_COLS_STATE = 1 };
template <int NQ, int COLS = FWD_COLS_NET, bool PUB = false>
__device__ __forceinline__ void fwd_gather_rows(const FwdGather& fg, bool second, float* Xs, long long row0, int rows_here, bool owes = true) {
  const GatherArgs& g = fg.g;
  const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long N = g.start[g.nbuf];
  const float* mine = nullptr;
  if (lane < 2) {
    const long long r = min(row0 + 16 * lane + grp, N - 1);
    int k;
    const long long src = gather_src(g, r, k);
    mine = g.bufs[k].state + src * g.bufs[k].pitch;
  }
  const int off = second ? fg.off[1] : fg.off[0], n = COLS == FWD_COLS_STATE ? g.S : second ? fg.n[1] : fg.n[0];
  const int q0 = off >> 2, q1 = (off + n + (second ? 2 : 0) + 3) >> 2;      // this tile's chunks of the row
  v4f v[2][NQ];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const gather_ptr_t rp = gather_group_row(mine, p);
#pragma unroll
    for (int j = 0; j < NQ; ++j) v[p][j] = rp[min(q0 + lane + 16 * j, q1 - 1)];
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = 16 * p + grp;
    const bool ok = r < rows_here;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int q = q0 + lane + 16 * j;
      if (q >= q1) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e - off;
        if (c >= 0 && c < n) Xs[r * LDX + c] = ok ? v[p][j][e] : 0.f;
        if (second && ok && owes && c == n) {
          if constexpr (PUB) agent_store(g.reward + row0 + r, v[p][j][e]);
          else g.reward[row0 + r] = v[p][j][e];
        }
        if (second && ok && owes && c == n + 1) {
          if constexpr (PUB) agent_store(g.not_done + row0 + r, v[p][j][e]);
          else g.not_done[row0 + r] = v[p][j][e];
        }
      }
    }
  }
}

// Returns the width of the input tile, as fwd_load_sources.  One thread of the launch advances the bump words.
template <int COLS = FWD_COLS_NET, bool PUB = false>
__device__ __forceinline__ int fwd_gather_tile(const FwdGather& fg, bool second, float* Xs, long long row0, int rows_here, bool owes = true) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    for (int k = 0; k < fg.g.nbump; ++k) fg.g.bump[k][0] += 1;
  const int off = second ? fg.off[1] : fg.off[0], n = COLS == FWD_COLS_STATE ? fg.g.S : second ? fg.n[1] : fg.n[0];
  if (((off + n + (second ? 2 : 0) + 3) >> 2) - (off >> 2) <= 16) fwd_gather_rows<1, COLS, PUB>(fg, second, Xs, row0, rows_here, owes);
  else fwd_gather_rows<FWD_GATHER_NQ, COLS, PUB>(fg, second, Xs, row0, rows_here, owes);
  return n;
}

// After the input barrier: the contiguous minibatch arrays, every element written once per launch -- state and action by
// the member-0 twin-Q tile of a row block, next_state by the pi(s') tile (all 256 threads, consecutive addresses).
__device__ __forceinline__ void fwd_gather_save(const FwdGather& fg, bool second, int m, const float* Xs, long long row0, int rows_here) {
  const GatherArgs& g = fg.g;
  auto put = [&](float* out, int col0, int n) {
    const uint32_t magic = div_magic(n);
    for (int e = threadIdx.x; e < rows_here * n; e += NTHREADS) {
      const int r = fast_div(e, magic, n);
      out[row0 * n + e] = Xs[r * LDX + col0 + (e - r * n)];
    }
  };
  if (second) {
    put(g.next_state, 0, g.S);
  } else if (m == 0) {
    put(g.state, 0, g.S);
    put(g.action, g.S, g.A);
  }
}

// Optional copy of the padded input tile for the weight gradients: same thread <-> element map as tile_load (no division).
__device__ __forceinline__ void fwd_save_x(const Mlp3FwdArgs& a, int m, const float* Xs, long long row0, int rows_here) {
  if (a.save_x != nullptr && (m == 0 || a.x_ms != 0)) {
    const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    float* sx = a.save_x + m * a.x_ms;
    for (int col = c; col < a.Kp1; col += 32)
      for (int r = r0; r < rows_here; r += NTHREADS >> 5) sx[(row0 + r) * a.Kp1 + col] = Xs[r * LDX + col];
  }
}

// This tile's slices of the optional activation copies and sign words, and of the output.
struct FwdTileOut { float *h1, *h2; uint32_t *mask1, *mask2; float* out; };
__device__ __forceinline__ FwdTileOut fwd_tile_out(const Mlp3FwdArgs& a, int m, long long row0) {
  FwdTileOut t;
  t.h1 = a.save_h1 ? a.save_h1 + ((long long)m * a.rows + row0) * HID : nullptr;
  t.h2 = a.save_h2 ? a.save_h2 + ((long long)m * a.rows + row0) * HID : nullptr;
  const long long mtile = ((long long)m * ((a.rows + 31) / 32) + row0 / 32) * HID;      // this tile's first mask word
  t.mask1 = a.mask1 ? a.mask1 + mtile : nullptr;
  t.mask2 = a.mask2 ? a.mask2 + mtile : nullptr;
  t.out = a.out + m * a.out_mstride + row0 * a.out_ld;
  return t;
}

// Whether this net's output layer runs as tile.h narrow_run_one: one live column of a 16-column output layer (twin-Q).
// Uniform over the launch's member slice.  -DMOBODY_NO_FWD_RANK1 (build.py MOBODY_EXTRA_FLAGS) keeps the MFMA form everywhere: the
// A/B parent.
template <int NT>
__device__ __forceinline__ bool fwd_rank1(const Mlp3FwdArgs& a) {
#ifdef MOBODY_NO_FWD_RANK1
  return false;
#else
  return NT == 1 && a.nout == 1;
#endif
}

// One element of the output layer: bias, tanh * max_action, residual, guarded store.
__device__ __forceinline__ void fwd_emit(const Mlp3FwdArgs& a, float* out, long long row0, int rows_here, int row, int col,
                                         float v, float bias) {
  if (row < rows_here && col < a.nout) {
    float y = v + bias;
    if (a.out_mode == 1) y = a.max_action * tanhf(y);
    if (a.resid != nullptr) y += a.resid[(row0 + row) * a.resid_ld + col];
    out[row * a.out_ld + col] = y;
  }
}
// the same element where another workgroup of the launch reads it (tile.h agent_store)
__device__ __forceinline__ void fwd_emit_pub(const Mlp3FwdArgs& a, float* out, long long row0, int rows_here, int row, int col,
                                             float v, float bias) {
  if (row < rows_here && col < a.nout) {
    float y = v + bias;
    if (a.out_mode == 1) y = a.max_action * tanhf(y);
    if (a.resid != nullptr) y += a.resid[(row0 + row) * a.resid_ld + col];
    agent_store(out + row * a.out_ld + col, y);
  }
}

}  // namespace mobody
