// Backward kernels of the 3-layer ReLU MLP (actor / twin-Q), fp32 MFMA.
//
// (The tile body, its masked epilogues and its seed prologues live in bwd_tile.h: critic_fwd_bf.hip runs the same tile.)
//
//   k_mlp3_bwd   per (32-row tile, member): dz3 (seed mode 0: read; mode 1: formed in the prologue from the critic's TD
//                error) -> dz2 = (dz3 W3^T) * [h2>0] -> dz1 = (dz2 W2^T) * [h1>0] (-> dx = dz1 W1^T), plus the
//                bias-gradient and loss partial sums of the tile.  Masks come from the forward's sign words (or the saved
//                activations); W^T blobs are streamed as MFMA B operands exactly like the forward weights.
//                                                                    (autograd of mobody.py:35-48)
//   k_actor_bwd_chain  the actor update's two passes in one launch, the only place seed modes 2 and 3 run: a frozen-Q dX tile
//                (mode 2: -p_w dmin(Q)), then -- in the second of the tile's two member workgroups to finish -- the actor's
//                tile of the same rows (mode 3: d(pre-tanh); ticket per row tile, no waiting)
//   k_wgrad      dW[k][n] = sum_rows A[row][k] * dZ[row][n]: rows are the contraction index, both
//                operands are read straight from global memory in MFMA fragment order (a wave
//                instruction = two full 128-byte lines); split-K over row slices, the four waves of a
//                workgroup reduce through LDS and write one deterministic partial slab.
//   k_grad_reduce slabs + bias partials -> gradient blob (deterministic, no atomics); on one GPU it applies the
//                Adam / Polyak step to each element it has just reduced, and one extra workgroup finishes the losses.
//
// Roofline: k_mlp3_bwd and k_wgrad are MFMA-f32 bound (2*256*256 FLOP per row and layer against
// ~2 KB of activations per row); k_grad_reduce is HBM/L2 streaming.
#include <stdlib.h>

#include "bwd_tile.h"

namespace mobody {

template <bool DX, int NT, int MASK, int PM = 0>
// (three workgroups per CU only for the sign-word variants: the variants that hold 32 mask / derivative values per lane next to
//  the accumulators spilled ~26 VGPRs at the 168-register budget; they serve the small generic launches -- V function, DARA
//  classifier, dynamics pre-training -- where a third resident workgroup buys nothing)
__global__ __launch_bounds__(NTHREADS, MASK == 1 ? 3 : 2) void k_mlp3_bwd(Mlp3BwdArgs a) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  mlp3_bwd_tile<DX, NT, MASK, PM>(a, blockIdx.y, blockIdx.x, gridDim.y, Xs, red);
}

template <bool DX, int NT, int BITS, int NPL = 0>
static int launch_bwd_t(const Mlp3BwdArgs& a, int members, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(NPL > 0 ? NPL : 1), MLP_TILE_ROWS>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_bwd<DX, NT, BITS, NPL>, lds);
    if (rc) return rc;
    once = true;
  }
  dim3 grid((unsigned)cdiv(a.rows, MLP_TILE_ROWS), (unsigned)members);
  ProfScope prof(PROF_MLP_BWD, st);
  hipLaunchKernelGGL((k_mlp3_bwd<DX, NT, BITS, NPL>), grid, dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK("k_mlp3_bwd");
  return 0;
}

// (Np1t, with_dx) -> the <DX, NT> pair of a backward instance, handed to `f` as integral constants: no dx = <false, 0>; dx
// through the K-split narrow layer where Np1t == 16 * NT (NT = 1, 2), else <true, 0>, the row-split path
template <class F>
static int dispatch_dx_nt(int Np1t, bool with_dx, F&& f) {
  using std::integral_constant;
  if (!with_dx) return f(std::false_type{}, integral_constant<int, 0>{});
  return Np1t == 16 ? f(std::true_type{}, integral_constant<int, 1>{}) : Np1t == 32 ? f(std::true_type{}, integral_constant<int, 2>{})
                                                                                      : f(std::true_type{}, integral_constant<int, 0>{});
}

// MASK / NPL as in mlp3_bwd_tile (MASK, PM); the callers size `dbp` / the bias reduction by MLP_TILE_ROWS
template <int MASK, int NPL = 0>
static int launch_bwd_dx(const Mlp3BwdArgs& a, int members, bool with_dx, hipStream_t st) {
  return dispatch_dx_nt(a.Np1t, with_dx, [&](auto dx, auto nt) {
    return launch_bwd_t<decltype(dx)::value, decltype(nt)::value, MASK, NPL>(a, members, st);
  });
}

int launch_mlp3_bwd(const Mlp3BwdArgs& a, int members, bool with_dx, hipStream_t st) {
  MB_REQUIRE(a.seed.mode == 0 || a.seed.mode == 1, "launch_mlp3_bwd: seed mode %d runs in launch_actor_bwd_chain only", a.seed.mode);
  if (a.rows <= 0) return 0;
  // Swish nets (the ensemble dynamics, pre-training): derivative multipliers in h1 / h2; f16x2: the 256 x 256 GEMM on the split
  // core, dz2 as planes for the weight gradients
  if (a.swish)
    return a.prec == PREC_F16X2 && a.w2t_planes != nullptr ? launch_bwd_dx<2, 4>(a, members, with_dx, st) : launch_bwd_dx<2>(a, members, with_dx, st);
  // split-precision backward: sign-word masks (the train step's three backward launches)
  if (a.prec != PREC_F32 && a.w2t_planes != nullptr && a.m1 != nullptr && a.m2 != nullptr)
    return a.prec == PREC_BF16 ? launch_bwd_dx<1, 1>(a, members, with_dx, st) : a.prec == PREC_BF16X2 ? launch_bwd_dx<1, 2>(a, members, with_dx, st)
         : a.prec == PREC_BF16X3 ? launch_bwd_dx<1, 3>(a, members, with_dx, st) : launch_bwd_dx<1, 4>(a, members, with_dx, st);
  // fp32 ReLU backward: sign words, or the saved activations
  return a.m1 != nullptr && a.m2 != nullptr ? launch_bwd_dx<1>(a, members, with_dx, st) : launch_bwd_dx<0>(a, members, with_dx, st);
}

// ------------------------------------------------------------------------------------------------
// The actor update's two backward passes in ONE launch: the frozen twin-Q input-gradient pass (seed mode 2, grid = row tiles x
// 2 members, exactly the launch k_mlp3_bwd<true, NT, 1, PM> would be) and, chained onto it tile by tile, the actor's own backward
// (seed mode 3).  An actor tile reads, for its 32 rows only, dxa of both members and bcw -- all written by the two member
// workgroups of the same blockIdx.x -- so it can start the moment those two have finished: each workgroup publishes its rows at
// device scope and draws a ticket for its tile; the second arriver runs the actor tile in the same workgroup, on the same LDS.
// THERE IS NO WAIT LOOP: a workgroup that is not last exits, so nobody ever waits for another workgroup and the launch makes
// progress under any dispatch order or residency.  The two passes use disjoint scratch (mode 2 writes dx and bcw only; dz2, dz1,
// dz3a, dbp and lossp are mode 3's), so an actor tile running beside other tiles' dX workgroups conflicts with nothing.
// Publication (correct wherever the three parties sit -- with an odd tile count a tile's members land on different XCDs): the
// ~1 KB of dx / bcw leaves in write-through agent-scope stores -> every wave drains its vector-memory counter -> workgroup barrier ->
// one lane's relaxed agent-scope fetch_add on tickets[tile]; the workgroup that draws 1 re-arms the ticket (a second backward on the
// same forward finds 0 again; k_actor_stats zeroes the words in front of the first) and goes on, reading dxa / bcw -- every load
// of them -- at agent scope, past its CU's L1.  (The fence form -- plain stores, an agent-scope release in all 640 workgroups,
// an acquire in the 320 that go on -- is as correct and measured 10 us SLOWER per step than the two separate launches: each
// release writes back its XCD's L2, which is full of the actor tiles' dz2 / dz1.)  "I am last" travels through
// `red`, the one static LDS object the tile body has anyway.  Every fma and MFMA sequence per output element is the one of the two
// separate launches: the results are the same bits.
// ------------------------------------------------------------------------------------------------
// PARAMETER ORDER: `q` first, `pi` directly behind it -- the body reads `pi` at offset sizeof(Mlp3BwdArgs) of the kernel-argument
// segment (see there); a parameter put in front of `pi` moves it.
// SQ: the seed form of the frozen-Q tile -- 2 (MOBODY) or 4 (the TD3_BC actor update, train.h BwdSeed)
template <int NT, int PM, int SQ>
__global__ __launch_bounds__(NTHREADS, 3) void k_actor_bwd_chain(Mlp3BwdArgs q, Mlp3BwdArgs pi, int* tickets) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const int tile = blockIdx.x;
  mlp3_bwd_tile<true, NT, 1, PM, SQ>(q, blockIdx.y, tile, 2, Xs, red);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's write-through dx (and bcw) stores are done
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(tickets + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t == 1) __hip_atomic_store(tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // both members have published
    red[0] = __int_as_float(t);
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");         // (no instruction: the agent-scope loads below stay below the ticket)
  const int ticket = __float_as_int(red[0]);
  if (ticket != 1) return;                                       // (a word nobody zeroed never reads 1: the actor tile then does not run)
  lds_barrier();                                                 // everybody has read red[0] before the seed's loss partials overwrite it
  // `pi` is read through the kernel-argument segment behind an opaque copy of its address: read as the parameter, its fields
  // (invariant loads) were hoisted into the frozen-Q tile and held there, up to 14 scalar registers spilled and a scratch frame
  // in two instances.  Nothing of the first tile is live here but the tile index.
  static_assert(sizeof(Mlp3BwdArgs) % 8 == 0 && alignof(Mlp3BwdArgs) == 8, "`pi` follows `q` in the kernel-argument segment");
  using KernArg = const __attribute__((address_space(4))) Mlp3BwdArgs;
  KernArg* ka = (KernArg*)__builtin_amdgcn_kernarg_segment_ptr() + 1;
  asm volatile("" : "+s"(ka));
  mlp3_bwd_tile<false, 0, 1, PM, 3>(*(const Mlp3BwdArgs*)ka, 0, tile, 1, Xs, red);
}

template <int NT, int PM, int SQ>
static int launch_chain_t(const Mlp3BwdArgs& q, const Mlp3BwdArgs& pi, int* tickets, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(PM > 0 ? PM : 1), MLP_TILE_ROWS>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_actor_bwd_chain<NT, PM, SQ>, lds);
    if (rc) return rc;
    once = true;
  }
  dim3 grid((unsigned)cdiv(q.rows, MLP_TILE_ROWS), 2u);
  ProfScope prof(PROF_MLP_BWD, st);
  hipLaunchKernelGGL((k_actor_bwd_chain<NT, PM, SQ>), grid, dim3(NTHREADS), lds, st, q, pi, tickets);
  MB_LAUNCH_OK("k_actor_bwd_chain");
  return 0;
}
template <int PM>
static int launch_chain_nt(const Mlp3BwdArgs& q, const Mlp3BwdArgs& pi, int* tickets, hipStream_t st) {
  return dispatch_dx_nt(q.Np1t, true, [&](auto, auto nt) {
    // (mode 2 named first: the instances are emitted in the order they are named here, and with the mode-4 instance in front of
    //  its mode-2 sibling the SAME machine code of k_actor_bwd_chain<2, 4, 2> ran 1.9 us per launch slower at another address:
    //  the c2 step 0.1992 ms against 0.1966 ms this way round and 0.1978 ms before mode 4 existed)
    return q.seed.mode != 4 ? launch_chain_t<decltype(nt)::value, PM, 2>(q, pi, tickets, st)
                            : launch_chain_t<decltype(nt)::value, PM, 4>(q, pi, tickets, st);
  });
}

// q: the frozen twin-Q pass (seed mode 2, or 4 = TD3_BC; dx out), pi: the actor's pass (seed mode 3) on the same rows; both with sign words and
// the same precision.  tickets: one zeroed int per row tile.  The precision picks the instance as in launch_mlp3_bwd.
int launch_actor_bwd_chain(const Mlp3BwdArgs& q, const Mlp3BwdArgs& pi, int* tickets, hipStream_t st) {
  if (q.rows <= 0) return 0;
  MB_REQUIRE(q.seed.mode != 4 || (q.seed.ar.A <= 24 && q.seed.ar.Nt == q.seed.ar.N),
             "launch_actor_bwd_chain: seed mode 4 spreads A <= 24 action columns over eight lanes and weights every row (A=%d)", q.seed.ar.A);
  MB_REQUIRE((q.seed.mode == 2 || q.seed.mode == 4) && pi.seed.mode == 3 && q.rows == pi.rows && q.prec == pi.prec && tickets != nullptr &&
             q.m1 && q.m2 && pi.m1 && pi.m2 && !q.swish && !pi.swish && (q.w2t_planes != nullptr) == (pi.w2t_planes != nullptr),
             "launch_actor_bwd_chain: the two passes do not form an actor update");
  if (q.prec != PREC_F32 && q.w2t_planes != nullptr)
    return q.prec == PREC_BF16 ? launch_chain_nt<1>(q, pi, tickets, st) : q.prec == PREC_BF16X2 ? launch_chain_nt<2>(q, pi, tickets, st)
         : q.prec == PREC_BF16X3 ? launch_chain_nt<3>(q, pi, tickets, st) : launch_chain_nt<4>(q, pi, tickets, st);
  return launch_chain_nt<0>(q, pi, tickets, st);
}

// ------------------------------------------------------------------------------------------------
// weight gradient GEMM (all three layers of one packed MLP in ONE launch)
//
//   job 0: dW2  = h1^T dz2      256 x 256      wave tile 64 x 64  (MT = 2)
//   job 1: dW1  = x^T  dz1      Kp1 x 256      wave tile 32 x 64  (MT = 1)
//   job 2: dW3^T = dz3^T h2     Np3 x 256      wave tile 32 x 64  (MT = 1), stored transposed into W3's [256][Np3]
//
// Rows are the contraction index: lane (i = lane&31, h = lane>>5) reads A[row+h][k0+i] and B[row+h][n0+i], i.e.
// every wave instruction is two full 128-byte lines, no LDS staging.  Split-K: the 4 waves of a workgroup take
// 4 consecutive row slices of the same output tile and reduce through LDS; workgroups along the row dimension
// write separate slabs (deterministic, summed by k_grad_reduce).  Operands of the next 8 rows are prefetched
// into a second register set while the current 8 rows feed the MFMAs (see wgrad_tile for what makes that overlap real).
// Block -> work mapping is XCD aware (blocks b and b+8 share an XCD and its L2): every (row slice, member) lives on one
// XCD, so its activations are fetched from HBM/Infinity Cache once and re-read by its output tiles from that XCD's L2.
// Along the block index the output TILE varies slowest: the tiles of the heavy 256 x 256 job are dispatched first, all
// their slices side by side (the tiles resident on an XCD at one time share its few slices' activations), the narrow
// jobs last.  k_wgrad_f16 holds 153 registers, three waves a SIMD: all 768 workgroups of a train-step launch are resident at
// once, three per CU.  Which block computes what changes no slab value; what every form has to keep is the ORDER (tests/
// wgrad_order_ref.py): wave (slice, w) runs one fp32 fma chain per element over its rows in increasing order, the four waves
// of a slice meet as (w0 + w2) + (w1 + w3), k_grad_reduce adds the slabs in slab order.
// The narrow jobs are 14 % of the FLOPs and cost 4.5 us of a 17.4 us launch, but not through the matrix pipe: 32 x 32
// tiles (half the chain per wave), 16-row blocks (half the round trips) and a rank-1 fma form of a one-output net's dW3 (no
// MFMA at all) each kept every bit and each measured SLOWER -- the launch moves ~11 TB/s from L2 and whatever makes the narrow
// waves ask for more, or sooner, takes it from the 256 x 256 tiles.
// ------------------------------------------------------------------------------------------------
// Buffer descriptor over `nrows` rows of a row-major fp32 matrix (pitch ld floats) starting at the wave-uniform pointer p, and a
// dword load through it: the per-lane byte offset rides in voffset, the wave-uniform row offset in soffset (a scalar register).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t slice_rsrc(const float* p, int nrows, int ld) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)((unsigned)nrows * (unsigned)ld * 4u), 0x00020000);
}
__device__ __forceinline__ float buf_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}

// Reduce the four row slices of a workgroup through LDS and write one slab tile.  Two tile buffers (32 KB), not four:
// waves 0,1 store, waves 2,3 add onto them (same lane <-> element map, so no conflicts).  With four buffers (64 KB)
// only two workgroups fit a CU and a 768-workgroup launch needs two rounds.
template <int MT, int NT>
__device__ __forceinline__ void wgrad_store(const WgradJob& jb, const WgradArgs& a, f32x16 (&acc)[MT][NT], int k0, int n0,
                                            int slice, int m, float* red) {
  constexpr int TK = 32 * MT, TN = 32 * NT;
  const int lane = lane_id(), w = wave_id();
  const int i = lane & 31, h = lane >> 5;
  float* mine = red + (w & 1) * (TK * TN);
  auto sweep = [&](bool add) {
#pragma unroll
    for (int x = 0; x < MT; ++x)
#pragma unroll
      for (int y = 0; y < NT; ++y)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kk = 32 * x + (r & 3) + 8 * (r >> 2) + 4 * h;
          float* p = mine + kk * TN + 32 * y + i;
          *p = add ? *p + acc[x][y][r] : acc[x][y][r];
        }
  };
  if (w < 2) sweep(false);
  lds_barrier();
  if (w >= 2) sweep(true);
  lds_barrier();
  float* slab = a.slabs + (long long)slice * a.slab_stride + jb.out_off + m * a.out_mstride;
  // Wide storage and W3's transposed [n][Np3] rows keep four consecutive k adjacent: the tile leaves in 16-byte stores (a wave
  // instruction = 1 KB contiguous for the wide jobs instead of 64 dwords at a 16-byte stride); same sums, same destinations.
  if ((jb.wide || jb.transposed) && (jb.out_k & 3) == 0 && (!jb.transposed || (jb.out_ld & 3) == 0)) {
    for (int g = threadIdx.x; g < (TK / 4) * TN; g += NTHREADS) {
      const int kg = g / TN, nn = g - kg * TN;
      f32x4 s;
#pragma unroll
      for (int c = 0; c < 4; ++c) { const int idx = (4 * kg + c) * TN + nn; s[c] = red[idx] + red[TK * TN + idx]; }
      const int gk = k0 + 4 * kg, gn = n0 + nn;
      if (gk < jb.out_k && gn < jb.out_n)
        *reinterpret_cast<f32x4*>(slab + (jb.transposed ? (long long)gn * jb.out_ld + gk : wide_idx(gk, gn))) = s;
    }
    return;
  }
  for (int idx = threadIdx.x; idx < TK * TN; idx += NTHREADS) {
    const int kk = idx / TN, nn = idx - kk * TN;
    const float s = red[idx] + red[TK * TN + idx];
    const int gk = k0 + kk, gn = n0 + nn;
    if (gk < jb.out_k && gn < jb.out_n) {
      if (jb.transposed) slab[(long long)gn * jb.out_ld + gk] = s;
      else if (jb.wide) slab[wide_idx(gk, gn)] = s;
      else slab[(long long)gk * jb.out_ld + gn] = s;
    }
  }
}

// What the three tile functions open with: the tile's first output row k0 and column n0, the row range [r_begin, r_end) of this
// wave (wave w of slice `slice` takes the slice's w-th run of rows_per_wave rows), and zeroed accumulators.
struct WgradTile { int k0, n0; long long r_begin, r_end; };
template <int MT, int NT>
__device__ __forceinline__ WgradTile wgrad_tile_open(const WgradJob& jb, const WgradArgs& a, int tile, int slice, f32x16 (&acc)[MT][NT]) {
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int tk = tile / jb.tiles_n, tn = tile - tk * jb.tiles_n;
  WgradTile g;
  g.k0 = tk * 32 * MT; g.n0 = tn * 32 * NT;
  g.r_begin = ((long long)slice * 4 + w) * a.rows_per_wave;
  g.r_end = min(a.rows, g.r_begin + a.rows_per_wave);
#pragma unroll
  for (int x = 0; x < MT; ++x)
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;
  return g;
}

// The row loop runs on wave-uniform row-block pointers (scalar registers) plus one per-lane 32-bit offset per operand
// column block, so a load costs no vector arithmetic, and whole row blocks carry no masks: the loaded registers feed the
// MFMAs directly and the loads of block n+1 stay in flight under the MFMAs of block n.  (Multiplying every loaded
// value by a 0/1 mask, as the first version did, made the compiler wait for each block's loads BEFORE the previous
// block's MFMAs: nothing overlapped inside a wave.)  Columns past ka / nb read column 0 instead: their products land in
// output elements wgrad_store never writes.  Only the < RB rows left at the end of a wave's slice take masked loads.
// The double-buffered loop over a wave's nblk whole row blocks: load(block, buf) requests a block's operands, mma(buf) feeds
// them to the MFMAs, so the loads of block n + 1 travel under the MFMAs of block n.  Straight-line body (no branch between a
// block's loads and the previous block's MFMAs, or the compiler's vmcnt bookkeeping merges the two paths and waits for the NEW
// loads): the last pass re-loads block nblk - 1, unused if nblk is even.
template <class Buf, class Load, class Mma>
__device__ __forceinline__ void wgrad_row_loop(int nblk, Load&& load, Mma&& mma) {
  Buf b0, b1;
  if (nblk > 0) load(0, b0);
  for (int blk = 0; blk + 1 < nblk; blk += 2) {
    load(blk + 1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mma(b0);
    __builtin_amdgcn_sched_barrier(0);
    load(min(blk + 2, nblk - 1), b0);
    __builtin_amdgcn_sched_barrier(0);
    mma(b1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (nblk & 1) mma(b0);
}

template <int MT>
__device__ __forceinline__ void wgrad_tile(const WgradJob& jb, const WgradArgs& a, int tile, int slice, int m, float* red) {
  constexpr int NT = 2, U = 4, RB = 2 * U;
  f32x16 acc[MT][NT];
  const WgradTile g = wgrad_tile_open<MT, NT>(jb, a, tile, slice, acc);
  const int k0 = g.k0, n0 = g.n0;
  const long long r_begin = g.r_begin, r_end = g.r_end;
  const int lane = lane_id(), i = lane & 31, h = lane >> 5;
  const int lda = jb.lda, ldb = jb.ldb;

  unsigned oa[MT], ob[NT];                            // byte offsets; lane half h takes the odd row of each pair
#pragma unroll
  for (int x = 0; x < MT; ++x) { const int c = k0 + 32 * x + i; oa[x] = 4u * (unsigned)((c < jb.ka ? c : 0) + h * lda); }
#pragma unroll
  for (int y = 0; y < NT; ++y) { const int c = n0 + 32 * y + i; ob[y] = 4u * (unsigned)((c < jb.nb ? c : 0) + h * ldb); }

  struct Blk { float a[U][MT], b[U][NT]; };          // the operands of one RB-row block
  auto mma = [&](const Blk& k) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y)
          acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x2f32(k.a[u][x], k.b[u][y], acc[x][y], 0, 0, 0);
  };
  if (r_begin < r_end) {
    const int nrows = (int)(r_end - r_begin), nblk = nrows / RB, tail = nrows - nblk * RB;
    const auto ra = slice_rsrc(jb.A + m * jb.a_mstride + r_begin * lda, nrows, lda);
    const auto rb = slice_rsrc(jb.B + m * jb.b_mstride + r_begin * ldb, nrows, ldb);
    const unsigned sa = 4u * lda, sb = 4u * ldb;      // row pitch in bytes
    wgrad_row_loop<Blk>(nblk, [&](int blk, Blk& k) {
      const unsigned row = blk * RB;
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int x = 0; x < MT; ++x) k.a[u][x] = buf_ld(ra, oa[x], (row + 2 * u) * sa);
#pragma unroll
        for (int y = 0; y < NT; ++y) k.b[u][y] = buf_ld(rb, ob[y], (row + 2 * u) * sb);
      }
    }, mma);
    if (tail > 0) {                                   // rows [nblk * RB, nrows) of the slice: masked lanes re-read its first row
      Blk k;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool ok = 2 * u + h < tail;
#pragma unroll
        for (int x = 0; x < MT; ++x) { const float v = buf_ld(ra, ok ? oa[x] + 2 * u * sa : oa[x] - h * sa, nblk * RB * sa); k.a[u][x] = ok ? v : 0.f; }
#pragma unroll
        for (int y = 0; y < NT; ++y) { const float v = buf_ld(rb, ok ? ob[y] + 2 * u * sb : ob[y] - h * sb, nblk * RB * sb); k.b[u][y] = ok ? v : 0.f; }
      }
      mma(k);
    }
  }
  wgrad_store<MT, NT>(jb, a, acc, k0, n0, slice, m, red);
}

// Split-precision form of the 256 x 256 job (dW2 = h1^T dz2, 86 % of the weight-gradient FLOPs): the contraction runs over
// batch ROWS, so a lane's A / B fragment of v_mfma_f32_32x32x16_bf16 is eight consecutive rows of one column -- eight
// coalesced scalar loads (a wave instruction = 2 rows x 128 bytes), split into NPL bf16 terms in registers, then the
// (i + j < NPL) products.  Same work split, addressing, LDS reduction and slab output as wgrad_tile<2>; row blocks of 16.
template <int NPL>
__device__ __forceinline__ void wgrad_tile_bf(const WgradJob& jb, const WgradArgs& a, int tile, int slice, int m, float* red) {
  constexpr int MT = 2, NT = 2, RB = 16;
  f32x16 acc[MT][NT];
  const WgradTile g = wgrad_tile_open<MT, NT>(jb, a, tile, slice, acc);
  const int k0 = g.k0, n0 = g.n0;
  const long long r_begin = g.r_begin, r_end = g.r_end;
  const int lane = lane_id(), i = lane & 31, h = lane >> 5;
  const int lda = jb.lda, ldb = jb.ldb;
  unsigned oa[MT], ob[NT];                                       // byte offsets; job 0: every column is real (ka = nb = 256)
#pragma unroll
  for (int x = 0; x < MT; ++x) oa[x] = 4u * (unsigned)(k0 + 32 * x + i + 8 * h * lda);
#pragma unroll
  for (int y = 0; y < NT; ++y) ob[y] = 4u * (unsigned)(n0 + 32 * y + i + 8 * h * ldb);
  auto pack = [&](const float (&v)[8], bf16x8 (&f)[NPL]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __bf16 t[NPL];
      bf_split<NPL>(v[j], t);
#pragma unroll
      for (int p = 0; p < NPL; ++p) f[p][j] = t[p];
    }
  };
  struct Blk { float a[MT][8], b[NT][8]; };          // the operands of one RB-row block
  auto mma = [&](const Blk& k) {
    bf16x8 af[MT][NPL], bfr[NT][NPL];
#pragma unroll
    for (int x = 0; x < MT; ++x) pack(k.a[x], af[x]);
#pragma unroll
    for (int y = 0; y < NT; ++y) pack(k.b[y], bfr[y]);
#pragma unroll
    for (int x = 0; x < MT; ++x)
#pragma unroll
      for (int y = 0; y < NT; ++y)
#pragma unroll
        for (int d = NPL - 1; d >= 0; --d)
#pragma unroll
          for (int q = 0; q <= d; ++q)
            acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[x][q], bfr[y][d - q], acc[x][y], 0, 0, 0);
  };
  if (r_begin < r_end) {
    const int nrows = (int)(r_end - r_begin), nblk = nrows / RB, tail = nrows - nblk * RB;
    const auto ra = slice_rsrc(jb.A + m * jb.a_mstride + r_begin * lda, nrows, lda);
    const auto rb = slice_rsrc(jb.B + m * jb.b_mstride + r_begin * ldb, nrows, ldb);
    const unsigned sa = 4u * lda, sb = 4u * ldb;
    wgrad_row_loop<Blk>(nblk, [&](int blk, Blk& k) {
      const unsigned row = blk * RB;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int x = 0; x < MT; ++x) k.a[x][j] = buf_ld(ra, oa[x], (row + j) * sa);
#pragma unroll
        for (int y = 0; y < NT; ++y) k.b[y][j] = buf_ld(rb, ob[y], (row + j) * sb);
      }
    }, mma);
    if (tail > 0) {                                   // as in wgrad_tile
      Blk k;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = 8 * h + j < tail;
#pragma unroll
        for (int x = 0; x < MT; ++x) { const float v = buf_ld(ra, ok ? oa[x] + j * sa : oa[x] - 8 * h * sa, nblk * RB * sa); k.a[x][j] = ok ? v : 0.f; }
#pragma unroll
        for (int y = 0; y < NT; ++y) { const float v = buf_ld(rb, ok ? ob[y] + j * sb : ob[y] - 8 * h * sb, nblk * RB * sb); k.b[y][j] = ok ? v : 0.f; }
      }
      mma(k);
    }
  }
  wgrad_store<MT, NT>(jb, a, acc, k0, n0, slice, m, red);
}

// "f16x2" form of the 256 x 256 job: both operands arrive PRE-SPLIT -- the two fp16 planes the forward (h1) and backward
// (dz2) epilogues stored in fragment order, [row / 8][256][8] per plane -- so a lane's A / B fragment is ONE 16-byte load and
// the row loop has no conversion work at all: per 16-row block 8 loads and 12 MFMAs (three products on four 32 x 32 tiles).
// Every 32-row tile carries its own power-of-two scales (planes hold h1 * 2^eA[t], dz2 * 2^eB[t]); a wave brings its
// blocks to one common scale U = min_t (eA[t] + eB[t]) over its rows by multiplying the B fragments with the exact factor
// 2^(U - eA[t] - eB[t]) <= 1 (v_pk_mul_f16, exact down to 2^-24, the smallest fp16 subnormal) and un-scales its accumulators
// once at the end.  A tile more than 2^24 below the slice's dominant one (U - eA - eB < -24) is dropped -- its factor is
// 0: its terms are below 2^-24 of the dominant tile's and so below fp32 resolution of the sum (a factor clamped to
// 2^-24 instead would overweight it by 2^(-24 - sh), which is all there is of an element the dominant tiles do not reach).
__device__ __forceinline__ void wgrad_tile_f16(const WgradJob& jb, const WgradArgs& a, int tile, int slice, int m, float* red) {
  constexpr int MT = 2, NT = 2, RB = 16;
  f32x16 acc[MT][NT];
  const WgradTile g = wgrad_tile_open<MT, NT>(jb, a, tile, slice, acc);
  const int k0 = g.k0, n0 = g.n0;
  const long long r_begin = g.r_begin, r_end = g.r_end;
  const int lane = lane_id(), i = lane & 31, h = lane >> 5;      // r_begin: multiple of 16
  int U = 0;
  if (r_begin < r_end) {
    const int nblk = (int)((r_end - r_begin + RB - 1) / RB);                   // the planes are zero beyond the batch (rows32)
    const int* eA = a.eA + m * a.e_mstride;
    const int* eB = a.eB + m * a.e_mstride;
    // Lane l keeps the summed exponent of the slice's tile t0 + l (a slice has at most 64 tiles: launch_wgrad), so the row
    // loop takes a block's scale with v_readlane instead of a memory round trip in front of its MFMAs.
    const int t0 = (int)(r_begin >> 5), t1 = (int)((r_end - 1) >> 5);
    const int Ev = (t0 + lane <= t1) ? eA[t0 + lane] + eB[t0 + lane] : 0x7fffffff;
    U = Ev;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) U = min(U, __shfl_xor(U, o));
    U = __builtin_amdgcn_readfirstlane(U);
    // 16-byte units: plane p of a member starts at p * plane_stride / 8; fragment of block b, column c: ((r / 8 + h) * 256 + c)
    const s16x8* pa = reinterpret_cast<const s16x8*>(jb.A) + (m * jb.a_mstride) / 8 + ((r_begin >> 3) + h) * HID + k0 + i;
    const s16x8* pb = reinterpret_cast<const s16x8*>(jb.B) + (m * jb.b_mstride) / 8 + ((r_begin >> 3) + h) * HID + n0 + i;
    const long long ps = a.plane_stride / 8;
    struct Blk { s16x8 a[2][MT], b[2][NT]; int sh; };
    auto load = [&](int b, Blk& k) {
      const long long o = (long long)b * 2 * HID;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int x = 0; x < MT; ++x) k.a[p][x] = pa[p * ps + o + 32 * x];
#pragma unroll
        for (int y = 0; y < NT; ++y) k.b[p][y] = pb[p * ps + o + 32 * y];
      }
      const int t = (int)((r_begin + (long long)b * RB) >> 5);
      k.sh = U - __builtin_amdgcn_readlane(Ev, t - t0);                         // <= 0
    };
    auto mma = [&](const Blk& k) {
      // 2^sh as a packed fp16 pair, exact for -24 <= sh <= 0; 0 below (the tile is dropped, see above: a select rather than a
      // branch around the MFMAs, which would break the straight-line body the loop relies on)
      const _Float16 f = k.sh < -24 ? (_Float16)0.f : (_Float16)__int_as_float((max(k.sh, -24) + 127) << 23);
      s16x8 bs[2][NT];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int y = 0; y < NT; ++y) bs[p][y] = __builtin_bit_cast(s16x8, __builtin_bit_cast(f16x8, k.b[p][y]) * f);
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < NT; ++y) {
          acc[x][y] = split_mfma<4>(k.a[0][x], bs[1][y], acc[x][y]);          // smallest terms first
          acc[x][y] = split_mfma<4>(k.a[1][x], bs[0][y], acc[x][y]);
          acc[x][y] = split_mfma<4>(k.a[0][x], bs[0][y], acc[x][y]);
        }
    };
    wgrad_row_loop<Blk>(nblk, load, mma);
  }
#pragma unroll
  for (int x = 0; x < MT; ++x)
#pragma unroll
    for (int y = 0; y < NT; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = ldexpf(acc[x][y][r], -U);
  wgrad_store<MT, NT>(jb, a, acc, k0, n0, slice, m, red);
}

// The Adam bias corrections of a device step count for the k_grad_reduce launch behind this one: one thread of the LAST
// workgroup (a narrow tile, done long before the 256 x 256 tiles), so that no workgroup of k_grad_reduce opens with a load, two
// double pow() and a barrier in front of its slab loads.  The step word is final before this launch (the step's first launch
// advances it).
__device__ __forceinline__ void wgrad_bias_corrections(const WgradArgs& a) {
  if (a.bc_out != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) adam_dev_consts(a.bc_t, a.bc_lr, a.bc_out);
}

// The body of the three weight-gradient kernels, which differ in the tile function of job 0 (TILE0) alone.  red: the workgroup's
// dynamic LDS, [2][64][64] floats.
template <void (*TILE0)(const WgradJob&, const WgradArgs&, int, int, int, float*)>
__device__ __forceinline__ void wgrad_body(const WgradArgs& a, float* red) {
  wgrad_bias_corrections(a);
  // XCD-aware decode: blocks with equal (id % 8) share an XCD; the output tile varies slowest (block comment above)
  const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
  const int groups = (a.nsplit * a.members + 7) / 8;
  const int t = j / groups;
  const int sm = xcd + 8 * (j - t * groups);
  if (sm >= a.nsplit * a.members) return;
  const int slice = sm / a.members, m = sm - slice * a.members;
  if (t < a.job[0].ntiles) TILE0(a.job[0], a, t, slice, m, red);
  else if (t < a.job[0].ntiles + a.job[1].ntiles) wgrad_tile<1>(a.job[1], a, t - a.job[0].ntiles, slice, m, red);
  else wgrad_tile<1>(a.job[2], a, t - a.job[0].ntiles - a.job[1].ntiles, slice, m, red);
}

__global__ __launch_bounds__(NTHREADS, 2) void k_wgrad_f16(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  wgrad_body<wgrad_tile_f16>(a, red);
}

template <int NPL>
__global__ __launch_bounds__(NTHREADS, 2) void k_wgrad_bf(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  wgrad_body<wgrad_tile_bf<NPL>>(a, red);
}

__global__ __launch_bounds__(NTHREADS, 4) void k_wgrad(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];
  wgrad_body<wgrad_tile<2>>(a, red);
}

// one weight-gradient kernel: allow its 32 KB of dynamic LDS once, then launch
template <void (*K)(WgradArgs)>
static int launch_wgrad_k(const char* name, const WgradArgs& a, int blocks, hipStream_t st) {
  constexpr size_t lds = (size_t)2 * 64 * 64 * sizeof(float);
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(K, lds);
    if (rc) return rc;
    once = true;
  }
  hipLaunchKernelGGL(K, dim3(blocks), dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK(name);
  return 0;
}

int launch_wgrad(WgradArgs a, hipStream_t st) {
  if (a.rows <= 0) return 0;
  const bool planes = a.prec == PREC_F16X2 && a.eA != nullptr;     // "f16x2": job 0 on the pre-split fp16 planes
  long long rpw = cdiv(a.rows, (long long)4 * a.nsplit);
  a.rows_per_wave = (rpw + 15) & ~15LL;               // whole 8- / 16-row blocks for every wave but the last one with work
  for (int k = planes ? 1 : 0; k < 3; ++k)            // a wave addresses its row slice through 32-bit buffer offsets
    if (a.rows_per_wave * (long long)std::max(a.job[k].lda, a.job[k].ldb) * 4 >= (1LL << 31))
      return fail(MOBODY_E_ARG, "launch_wgrad: row slice too large for 32-bit offsets (raise nsplit)");
  if (planes && a.rows_per_wave > 2048) return fail(MOBODY_E_ARG, "launch_wgrad: more than 64 row tiles per wave slice (raise nsplit)");
  a.job[0].tiles_n = (a.job[0].nb + 63) / 64; a.job[0].ntiles = ((a.job[0].ka + 63) / 64) * a.job[0].tiles_n;
  for (int k = 1; k < 3; ++k) { a.job[k].tiles_n = (a.job[k].nb + 63) / 64; a.job[k].ntiles = ((a.job[k].ka + 31) / 32) * a.job[k].tiles_n; }
  a.tiles_total = a.job[0].ntiles + a.job[1].ntiles + a.job[2].ntiles;
  const int sm = a.nsplit * a.members;
  const int blocks = 8 * ((sm + 7) / 8) * a.tiles_total;
  ProfScope prof(PROF_WGRAD, st);
  if (planes) return launch_wgrad_k<k_wgrad_f16>("k_wgrad_f16", a, blocks, st);
  // Split-precision job 0 in every bf16 mode (the operand split costs ~6 VALU instructions per value and term; with the
  // unmasked scalar-addressed row loop that still leaves a gain: per step at c2 0.058 ms fp32 job -> 0.052 bf16x3,
  // 0.044 bf16x2).
  if (a.prec != PREC_F32 && a.job[0].ka == HID && a.job[0].nb == HID && a.job[0].wide)
    return a.prec == PREC_BF16 ? launch_wgrad_k<k_wgrad_bf<1>>("k_wgrad_bf", a, blocks, st)
         : a.prec == PREC_BF16X2 ? launch_wgrad_k<k_wgrad_bf<2>>("k_wgrad_bf", a, blocks, st) : launch_wgrad_k<k_wgrad_bf<3>>("k_wgrad_bf", a, blocks, st);
  return launch_wgrad_k<k_wgrad>("k_wgrad", a, blocks, st);
}

// ------------------------------------------------------------------------------------------------
// slabs + bias partials -> gradient blob
// ------------------------------------------------------------------------------------------------
// Weight entries: one thread per entry sums the split-K slabs (coalesced across threads).  Bias entries: one
// WAVE per entry strides over the row-tile partials and shuffle-reduces (a serial loop over ~160 dependent
// L2 reads per thread made the first version of this kernel latency bound: 41 us instead of ~5).
__global__ __launch_bounds__(256) void k_grad_reduce(GradReduceArgs a) {
  __shared__ float adam_sm[2];
  // bias corrections of a device step count: a uniform load of what the weight-gradient launch left (no pow, no barrier, no
  // LDS in front of the slab loads), else formed once per workgroup
  const float* bc = a.bc_dev;
  float c0 = 0.f, c1 = 0.f;
  if (bc != nullptr) { c0 = bc[0]; c1 = bc[1]; }
  else if (a.adam.on && a.adam.t_dev != nullptr) { adam_block_consts(a.adam, adam_sm); c0 = adam_sm[0]; c1 = adam_sm[1]; }
  const float adam_c[2] = {c0, c1};
  const int hmask = health_mask(a.adam);                         // an earlier fault: the gradient and the loss are still written
  const long long nW = a.L.total_floats;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid == 0 && a.adam.on && a.adam.bump != nullptr && !(hmask != 0 && health_foreign(a.adam))) a.adam.bump[0] += 1;      // graph replay: advance a counter no block of this launch reads
  if (gid < nW) {
    const long long j = gid;
    const long long o = j % a.L.member_floats;
    const bool is_bias = (o >= a.L.b1 && o < a.L.b1 + HID) || (o >= a.L.b2 && o < a.L.b2 + HID) || (o >= a.L.b3);
    if (is_bias) return;
    // (requesting all 16 slab entries and the Adam state in one round trip instead of groups of four + one measured neutral at
    //  c2 and -1 % on the pre-training step: not kept)
    float s = 0.f;
    int k = 0;
    for (; k + 4 <= a.nsplit; k += 4) {            // 4 independent loads in flight, summed in slab order
      const float* p = a.slabs + (long long)k * a.slab_stride + j;
      const float v0 = p[0], v1 = p[a.slab_stride], v2 = p[2 * a.slab_stride], v3 = p[3 * a.slab_stride];
      s += v0; s += v1; s += v2; s += v3;
    }
    for (; k < a.nsplit; ++k) s += a.slabs[(long long)k * a.slab_stride + j];
    if (a.grad != nullptr) a.grad[j] = s;
    if (a.adam.on) adam_element(a.adam, a.L, j, s, adam_c, hmask);
    return;
  }
  // ---- bias part: wave index -> (member, bias element) ----
  const int per = 2 * HID + a.L.Np3;
  const long long wv = (gid - ((nW + 255) / 256) * 256) >> 6;
  if (blockIdx.x == gridDim.x - 1 && a.loss.kind != 0) {      // the extra workgroup: loss partials -> scalars
    __shared__ float sm[8];
    const LossFinal& f = a.loss;
    const int stride = f.kind == 2 ? 2 : 1;
    float s0 = 0.f, s1 = 0.f;
    for (int k = threadIdx.x; k < f.nparts; k += 256) { s0 += f.parts[stride * k]; if (f.kind == 2) s1 += f.parts[2 * k + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = s0; sm[4 + (threadIdx.x >> 6)] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      s0 = sm[0] + sm[1] + sm[2] + sm[3];
      s1 = sm[4] + sm[5] + sm[6] + sm[7];
      if (f.kind == 1) {
        f.out[0] = s0 * f.scale;
      } else {
        const float pw = f.scale_q ? f.weight / (f.stats[0] / f.ng) : 1.f;
        const float bc = s1 / f.ntg_a;
        f.out[0] = pw * s0 / f.ng + f.bc_coef * bc;
        f.out[1] = bc;
      }
    }
    return;
  }
  if (wv < 0 || wv >= (long long)a.L.members * per) return;
  const int lane = threadIdx.x & 63;
  const int m = (int)(wv / per), off = (int)(wv % per);
  float s = 0.f;
  for (int t = lane; t < a.ntiles; t += 64) s += a.dbp[((long long)t * a.L.members + m) * per + off];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) {
    const long long dst = (long long)m * a.L.member_floats + (off < HID ? a.L.b1 + off : off < 2 * HID ? a.L.b2 + (off - HID) : a.L.b3 + (off - 2 * HID));
    if (a.grad != nullptr) a.grad[dst] = s;
    if (a.adam.on) adam_element(a.adam, a.L, dst, s, adam_c, hmask);
  }
}

// dW1, dW2, dW3 (one merged split-K launch) + the deterministic slab / bias-partial reduction (optionally with the
// optimizer step fused).
int mlp3_weight_grads(const Mlp3WgradArgs& a, hipStream_t st) {
  const MobodyMlpLayout& L = a.L;
  const long long rows = a.rows;
  const bool planes = a.prec == PREC_F16X2 && a.e_h1 != nullptr;     // the exponents are read in the f16x2 mode alone
  WgradArgs g{};
  g.prec = a.prec;
  const long long rows32 = (rows + 31) & ~31LL;
  g.eA = planes ? a.e_h1 : nullptr; g.eB = planes ? a.e_dz2 : nullptr; g.e_mstride = rows32 / 32; g.plane_stride = rows32 * HID;
  const long long slab_stride = (L.total_floats + 3) & ~3LL;
  g.rows = rows; g.slabs = a.slabs; g.slab_stride = slab_stride; g.out_mstride = L.member_floats;
  g.nsplit = a.nsplit; g.members = L.members;
  const long long hs = rows * HID;
  // dW2 = h1^T dz2
  g.job[0] = WgradJob{a.h1, hs, HID, HID, a.dz2, hs, HID, HID, L.w2, HID, HID, HID, 0, 1, 0, 0};
  if (planes) g.job[0].a_mstride = g.job[0].b_mstride = 2 * rows32 * HID;   // planes: 16-bit elements per member
  // dW1 = x^T dz1
  g.job[1] = WgradJob{a.x, a.x_mstride, L.Kp1, L.Kp1, a.dz1, hs, HID, HID, L.w1, HID, L.Kp1, HID, 0, 1, 0, 0};
  // dW3^T = dz3^T h2, stored transposed into W3[256][Np3]
  g.job[2] = WgradJob{a.dz3, rows * L.Np3, L.Np3, L.Np3, a.h2, hs, HID, HID, L.w3, L.Np3, L.Np3, HID, 1, 0, 0, 0};
  GradReduceArgs r{L, a.slabs, slab_stride, a.nsplit, a.dbp, a.ntiles, a.grad, a.loss, a.adam, nullptr};
  if (a.bc_ws != nullptr && a.adam.on && a.adam.t_dev != nullptr) {
    if (!a.bc_ready) { g.bc_out = a.bc_ws; g.bc_t = a.adam.t_dev; g.bc_lr = a.adam.lr; }
    r.bc_dev = a.bc_ws;
  }
  int rc = launch_wgrad(g, st);
  if (rc) return rc;
  return launch_grad_reduce(r, st);
}

int launch_grad_reduce(const GradReduceArgs& a, hipStream_t st) {
  const long long wblocks = cdiv(a.L.total_floats, 256);
  const long long bblocks = cdiv((long long)a.L.members * (2 * HID + a.L.Np3) * 64, 256);
  const long long lblocks = a.loss.kind != 0 ? 1 : 0;
  hipLaunchKernelGGL(k_grad_reduce, dim3((unsigned)(wblocks + bblocks + lblocks)), dim3(256), 0, st, a);
  MB_LAUNCH_OK("k_grad_reduce");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// IQL's two trained one-member nets: the backward of k_mlp3_bwd<false, 0, 1, PM> with the seed form compiled in --
// mode 5, the expectile seed of the V net (rank-1 output layer), or mode 6, the advantage-weighted regression seed of the
// policy net (K = Np3 GEMM).  Mode 7, the double-softmax cross-entropy seed of DARA's two classifier heads, rides
// mode 6's path.  Instances of their own: no kernel that existed before them changes.
// ------------------------------------------------------------------------------------------------
template <int PM, int SEED>
__global__ __launch_bounds__(NTHREADS, 3) void k_mlp3_bwd_seed(Mlp3BwdArgs a) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  mlp3_bwd_tile<false, 0, 1, PM, SEED>(a, 0, blockIdx.x, 1, Xs, red);
}

template <int PM, int SEED>
static int launch_bwd_seed_t(const Mlp3BwdArgs& a, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(PM > 0 ? PM : 1), MLP_TILE_ROWS>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_bwd_seed<PM, SEED>, lds);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_BWD, st);
  hipLaunchKernelGGL((k_mlp3_bwd_seed<PM, SEED>), dim3((unsigned)cdiv(a.rows, MLP_TILE_ROWS)), dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK("k_mlp3_bwd_seed");
  return 0;
}
template <int PM>
static int launch_bwd_seed_m(const Mlp3BwdArgs& a, hipStream_t st) {
  return a.seed.mode == 5 ? launch_bwd_seed_t<PM, 5>(a, st) : a.seed.mode == 6 ? launch_bwd_seed_t<PM, 6>(a, st) : launch_bwd_seed_t<PM, 7>(a, st);
}

int launch_mlp3_bwd_seed(const Mlp3BwdArgs& a, hipStream_t st) {
  MB_REQUIRE((a.seed.mode == 5 || a.seed.mode == 6 || a.seed.mode == 7) && a.m1 && a.m2 && !a.swish && a.seed.dz3_out && a.seed.lossp,
             "launch_mlp3_bwd_seed: seed mode %d: needs mode 5, 6 or 7 of a ReLU net with sign words", a.seed.mode);
  MB_REQUIRE(a.seed.mode != 5 || a.Np3 == 16, "launch_mlp3_bwd_seed: seed mode 5 seeds a one-output net (Np3=%d)", a.Np3);
  MB_REQUIRE(a.seed.mode != 7 || a.Np3 == 16, "launch_mlp3_bwd_seed: seed mode 7 seeds a two-output net (Np3=%d)", a.Np3);
  if (a.rows <= 0) return 0;
  if (a.prec != PREC_F32 && a.w2t_planes != nullptr)
    return a.prec == PREC_BF16 ? launch_bwd_seed_m<1>(a, st) : a.prec == PREC_BF16X2 ? launch_bwd_seed_m<2>(a, st)
         : a.prec == PREC_BF16X3 ? launch_bwd_seed_m<3>(a, st) : launch_bwd_seed_m<4>(a, st);
  return launch_bwd_seed_m<0>(a, st);
}

// ------------------------------------------------------------------------------------------------
// IGDF's row-weighted critic: the twin-Q backward of seed mode 1 with the weight compiled in as mode 8 -- an instance of
// its own, so that the kernels of the unweighted critic keep their code.
// ------------------------------------------------------------------------------------------------
template <int PM>
__global__ __launch_bounds__(NTHREADS, 3) void k_mlp3_bwd_wcritic(Mlp3BwdArgs a) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  mlp3_bwd_tile<false, 0, 1, PM, 8>(a, blockIdx.y, blockIdx.x, 2, Xs, red);
}

template <int PM>
static int launch_bwd_wcritic_t(const Mlp3BwdArgs& a, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(PM > 0 ? PM : 1), MLP_TILE_ROWS>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_bwd_wcritic<PM>, lds);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_BWD, st);
  hipLaunchKernelGGL((k_mlp3_bwd_wcritic<PM>), dim3((unsigned)cdiv(a.rows, MLP_TILE_ROWS), 2u), dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK("k_mlp3_bwd_wcritic");
  return 0;
}

int launch_mlp3_bwd_wcritic(const Mlp3BwdArgs& a, hipStream_t st) {
  MB_REQUIRE(a.seed.mode == 8 && a.seed.cw.w && a.m1 && a.m2 && !a.swish && a.seed.dz3_out && a.seed.lossp && a.Np3 == 16,
             "launch_mlp3_bwd_wcritic: needs seed mode 8 with its row weights on a one-output ReLU twin net with sign words");
  if (a.rows <= 0) return 0;
  if (a.prec != PREC_F32 && a.w2t_planes != nullptr)
    return a.prec == PREC_BF16 ? launch_bwd_wcritic_t<1>(a, st) : a.prec == PREC_BF16X2 ? launch_bwd_wcritic_t<2>(a, st)
         : a.prec == PREC_BF16X3 ? launch_bwd_wcritic_t<3>(a, st) : launch_bwd_wcritic_t<4>(a, st);
  return launch_bwd_wcritic_t<0>(a, st);
}

// ------------------------------------------------------------------------------------------------
// BOSA's masked conservative critic: mode 8 plus a per-row constant, compiled in as mode 9 -- again an instance of its
// own, so that the kernels of modes 1 and 8 keep their code.
// ------------------------------------------------------------------------------------------------
template <int PM>
__global__ __launch_bounds__(NTHREADS, 3) void k_mlp3_bwd_ccritic(Mlp3BwdArgs a) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  mlp3_bwd_tile<false, 0, 1, PM, 9>(a, blockIdx.y, blockIdx.x, 2, Xs, red);
}

template <int PM>
static int launch_bwd_ccritic_t(const Mlp3BwdArgs& a, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(PM > 0 ? PM : 1), MLP_TILE_ROWS>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_bwd_ccritic<PM>, lds);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_BWD, st);
  hipLaunchKernelGGL((k_mlp3_bwd_ccritic<PM>), dim3((unsigned)cdiv(a.rows, MLP_TILE_ROWS), 2u), dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK("k_mlp3_bwd_ccritic");
  return 0;
}

int launch_mlp3_bwd_ccritic(const Mlp3BwdArgs& a, hipStream_t st) {
  MB_REQUIRE(a.seed.mode == 9 && a.seed.cs.w && a.seed.cs.c && a.m1 && a.m2 && !a.swish && a.seed.dz3_out && a.seed.lossp && a.Np3 == 16,
             "launch_mlp3_bwd_ccritic: needs seed mode 9 with its row weights and constants on a one-output ReLU twin net with sign words");
  if (a.rows <= 0) return 0;
  if (a.prec != PREC_F32 && a.w2t_planes != nullptr)
    return a.prec == PREC_BF16 ? launch_bwd_ccritic_t<1>(a, st) : a.prec == PREC_BF16X2 ? launch_bwd_ccritic_t<2>(a, st)
         : a.prec == PREC_BF16X3 ? launch_bwd_ccritic_t<3>(a, st) : launch_bwd_ccritic_t<4>(a, st);
  return launch_bwd_ccritic_t<0>(a, st);
}

}  // namespace mobody
