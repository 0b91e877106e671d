// The tile body of the split-precision fused MLP forward, shared by its two translation units: mlp_fwd_bf.hip (the plain, paired
// and gathering launches) and critic_fwd_bf.hip (the critic step's forwards merged into one launch).
#pragma once
#include "common.h"
#include "layers_bf.h"

namespace mobody {

constexpr int TB = MLP_TILE_ROWS, MT = MLP_MT;  // rows of a workgroup's tile; 32 x 32 MFMA row tiles per wave
constexpr int FWD_L1_RING = 3;                  // layer 1 is K = 24 .. 120: a short ring keeps the kernel at 128 registers
constexpr int FWD_F16_WAVES = 4;                // waves per SIMD the f16x2 inference forward is compiled for (launch bounds)

// ---- the merged critic forward (critic_fwd_bf.hip): what its tiles do differently from a plain gathering tile ----
// CF_NEXT: pi(s') as the first tile of a chained workgroup -- the layers overwrite the image, so it keeps its s' tile and then
//          its output a' in the LDS behind the image: the rows [s' | a'] target-Q takes;
// CF_Q:    a twin-Q tile whose input is either gathered (Q(s,a), with every save) or, `chained`, copied from those rows:
//          target-Q of the same 32 rows, no saves;
// CF_PI:   pi(s) with its saves, the state columns gathered with the indices of the row block's Q(s,a) tiles.
enum CriticFwdRole { CF_NONE = 0, CF_NEXT = 1, CF_Q = 2, CF_PI = 3 };
struct CriticFwdTile {
  float* Sa;                // [TB][S + A]: the chained workgroup's [s' | a'] rows (rows past the batch zero, as a tile load leaves them)
  int S, A;
  bool chained;             // the workgroup runs pi(s') and then target-Q on the same rows
  bool owes;                // CF_NEXT: this copy of the row block's pi(s') writes next_state, reward, not_done and pin
};

// fwd_emit of the chained pi(s'): the value that goes to `pin` is also the value target-Q takes, bit for bit; rows past the
// batch are zero as tile_load2 leaves them (they count in the f16 tile maximum)
__device__ __forceinline__ void chain_emit(const Mlp3FwdArgs& a, float* out, int rows_here, int row, int col, float v, float bias,
                                           const CriticFwdTile& ch) {
  if (col >= a.nout) return;
  float y = 0.f;
  if (row < rows_here) {
    y = v + bias;
    if (a.out_mode == 1) y = a.max_action * tanhf(y);
    if (ch.owes) out[row * a.out_ld + col] = y;
  }
  ch.Sa[row * (ch.S + ch.A) + ch.S + col] = y;
}
// thread t owns columns (t & 31) + 32 j of rows (t >> 5) + 8 u, as tile_load2
__device__ __forceinline__ void chain_stash(const float* Xs, const CriticFwdTile& ch) {
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  for (int col = c; col < ch.S; col += 32)
#pragma unroll
    for (int u = 0; u < TB / 8; ++u) ch.Sa[(r0 + 8 * u) * (ch.S + ch.A) + col] = Xs[(r0 + 8 * u) * LDX + col];
}
__device__ __forceinline__ int chain_input(float* Xs, const CriticFwdTile& ch) {
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
  for (int col = c; col < ch.S + ch.A; col += 32)
#pragma unroll
    for (int u = 0; u < TB / 8; ++u) Xs[(r0 + 8 * u) * LDX + col] = ch.Sa[(r0 + 8 * u) * (ch.S + ch.A) + col];
  return ch.S + ch.A;
}

// DS: training forward of a Swish net -- save_d1 / save_d2 receive the derivatives next to h1 (planes or rows) / h2
// GATHER: the input tile comes straight from the replay rings (layers.h fwd_gather_tile); fg / second: the stage's arguments and
// which net of the pair this tile belongs to
// ROLE / ch: a tile of the merged critic forward (above)
// PUB: the launch goes on to the critic backward of the same rows in whichever workgroup finishes them last (critic_fwd_bf.hip):
// what that tile's seed and masks read -- q / qt and the sign words of a CF_Q tile, reward / not_done of the CF_NEXT tile -- leaves
// in write-through agent-scope stores (tile.h agent_store); every other save stays a plain store
template <int ACT, int PM, int NT, bool DS = false, bool GATHER = false, int ROLE = CF_NONE, bool PUB = false>
__device__ __forceinline__ void mlp3_fwd_bf_tile(const Mlp3FwdArgs& a, int m, float* Xs, const FwdGather* fg = nullptr, bool second = false,
                                                 const CriticFwdTile& ch = CriticFwdTile{}) {
  char* Ps = reinterpret_cast<char*>(Xs);
  float* scr = reinterpret_cast<float*>(Ps + split_scr_offset<PM, TB>());
  const long long row0 = (long long)blockIdx.x * TB;
  const int rows_here = (int)min((long long)TB, a.rows - row0);
  const bool full = rows_here == TB;
  const float* w1 = a.w1 + m * a.sw1;
  const s16x8* w2b = reinterpret_cast<const s16x8*>(a.w2_planes + m * a.planes_ms);
  const float* w3 = a.w3 + m * a.sw3;
  const float* b3 = a.b3 + m * a.sb3;
  TR(0);
  WideRingT<FWD_L1_RING> ring;
  wide_prefetch(w1, a.Kp1, ring);
  int c0;
  if constexpr (ROLE == CF_NEXT) {
    c0 = fwd_gather_tile<FWD_COLS_NET, PUB>(*fg, true, Xs, row0, rows_here, ch.owes);
  } else if constexpr (ROLE == CF_Q) {
    if (ch.chained) {
      lds_barrier();                               // the output stage before this tile has read its partial sums (and left a')
      c0 = chain_input(Xs, ch);
    } else {
      c0 = fwd_gather_tile(*fg, false, Xs, row0, rows_here);
    }
  } else if constexpr (ROLE == CF_PI) {
    c0 = fwd_gather_tile<FWD_COLS_STATE>(*fg, false, Xs, row0, rows_here);
  } else if constexpr (GATHER) {
    c0 = fwd_gather_tile(*fg, second, Xs, row0, rows_here);
  } else if (a.n[0] <= 32 && a.n[1] <= 32 && a.n[2] == 0) {       // state | action: both sources in one round trip
    tile_load2<TB>(Xs, a.src[0] + m * a.src_ms[0] + row0 * a.ld[0], a.ld[0], a.n[0],
                   a.n[1] > 0 ? a.src[1] + m * a.src_ms[1] + row0 * a.ld[1] : nullptr, a.ld[1], a.n[1], rows_here);
    c0 = a.n[0] + a.n[1];
  } else {
    c0 = fwd_load_sources(a, m, Xs, row0, rows_here);
  }
  tile_zero_cols(Xs, c0, a.Kp1, TB);
  lds_barrier();
  TR(1);
  fwd_save_x(a, m, Xs, row0, rows_here);
  if constexpr (ROLE == CF_NEXT) {
    if (ch.owes) fwd_gather_save(*fg, true, m, Xs, row0, rows_here);
    chain_stash(Xs, ch);
  } else if constexpr (ROLE == CF_Q) {
    if (!ch.chained) fwd_gather_save(*fg, false, m, Xs, row0, rows_here);
  } else if constexpr (ROLE == CF_NONE && GATHER) {
    fwd_gather_save(*fg, second, m, Xs, row0, rows_here);
  }
  const FwdTileOut t = fwd_tile_out(a, m, row0);
  float* d1 = DS ? a.save_d1 + ((long long)m * a.rows + row0) * HID : nullptr;
  float* d2 = DS ? a.save_d2 + ((long long)m * a.rows + row0) * HID : nullptr;
  const int mg = (rows_here + 31) / 32;
  BfRing<PM> bring;
  PlaneSave gs{nullptr, 0, nullptr};
  if (a.save_h1p != nullptr) {
    gs.base = reinterpret_cast<short*>(a.save_h1p) + m * a.h1p_ms + (row0 / 8) * (HID * 8);
    gs.plane_stride = a.h1p_plane;
    gs.e_out = a.save_e1 + (long long)m * cdiv(a.rows, 32) + row0 / 32;
  }
  constexpr bool PQ = PUB && ROLE == CF_Q;
  const int e1 = wide_layer_to_planes<ACT, MT, PM, TB, DS, PQ>(Xs, Ps, scr, w1, a.b1 + m * a.sb1, a.Kp1, ring,
                                                           [&] { bf_prefetch<PM>(w2b, bring); }, t.mask1, full, mg, rows_here, t.h1, gs, d1);
  TR(2);
  auto emit = [&](int row, int col, float v, float bias) {
    if constexpr (ROLE == CF_NEXT) chain_emit(a, t.out, rows_here, row, col, v, bias, ch);
    else if constexpr (PQ) fwd_emit_pub(a, t.out, row0, rows_here, row, col, v, bias);
    else fwd_emit(a, t.out, row0, rows_here, row, col, v, bias);
  };
  if constexpr (NT > 0) {
    NarrowRegs<NT> br;
    const int mycol = threadIdx.x % (16 * NT);
    float bias;
    // a one-output net (twin-Q) forms its output as an fma chain (tile.h narrow_run_one): a wave-uniform branch, and the one
    // weight a lane needs travels in the first register of the fragments it does not fetch
    const bool one = fwd_rank1<NT>(a);
    bf_layer<ACT, MT, PM, TB, DS, PQ>(Xs, Ps, e1, w2b, a.b2 + m * a.sb2, bring, [&] {
      if (one) br.b[0][0] = narrow_prefetch_one(w3, 16 * NT);
      else narrow_prefetch<NT>(w3, 16 * NT, br);
      bias = b3[mycol < a.nout ? mycol : 0];
    }, t.mask2, mg, rows_here, t.h2, d2);
    TR(4);
    if (one) narrow_run_one<TB / 16>(Xs, br.b[0][0], [&](int row, int col, float v) { emit(row, col, v, bias); });
    else narrow_run<TB / 16, NT>(Xs, br, [&](int row, int col, float v) { emit(row, col, v, bias); });
  } else {
    bf_layer<ACT, MT, PM, TB, DS, PQ>(Xs, Ps, e1, w2b, a.b2 + m * a.sb2, bring, [] {}, t.mask2, mg, rows_here, t.h2, d2);
    narrow_layer(Xs, w3, HID, a.Np3, [&](int row, int col, float v) { emit(row, col, v, b3[col < a.nout ? col : 0]); }, TB);
  }
  TR(5);
}

}  // namespace mobody
