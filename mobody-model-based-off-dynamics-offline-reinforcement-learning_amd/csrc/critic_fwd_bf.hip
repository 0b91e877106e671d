// The critic step's forwards in ONE launch (f16x2): twin-Q(s,a) with saves, pi(s'), target twin-Q(s', pi(s')) and, when the caller
// asks for it, pi(s) with saves.  Target-Q of a row tile needs pi(s') of the same 32 rows and nothing else of the launch, so a
// workgroup evaluates pi(s') itself and goes on to the twin-Q layers without leaving the CU: a tile generation less than the two
// launches it replaces (mlp_fwd_bf.hip k_mlp3_fwd_bf_gather, then k_mlp3_fwd_bf).  No workgroup waits for another.
// Two forms (DESIGN 5n has the measurements):
//   CHAINS = 1  one chained workgroup per row block: pi(s'), then target-Q of member 0, then of member 1.  No tile is evaluated
//               twice; the launch is as long as three tiles in a row.  The form of a launch that fills the machine.
//   CHAINS = 2  one chained workgroup per row block and member: pi(s'), then target-Q of its member.  pi(s') is evaluated twice
//               (member 0's copy writes it); the launch is as long as two tiles.  The form of a launch whose workgroups have
//               CUs to themselves, where the redundant tile is free and the third tile in a row is not.
// (A translation unit of its own: next to this kernel the gathering kernels of mlp_fwd_bf.hip compiled to different code.)
//
// k_critic_chain_bf is the one-chain form with the critic BACKWARD chained onto it, tile by tile: the backward of
// (row tile t, member m), seed mode 1, reads q_m and the sign words of the Q(s,a) workgroup of (m, t) and qt of both members,
// reward and not_done of the chained workgroup of t -- nothing of another row tile.  Each of those two producers publishes
// these words (write-through agent-scope stores, every wave drains its vector-memory counter, workgroup barrier) and arrives on
// the ticket of (t, m); the one that completes it runs that backward tile on the same LDS.  A chained workgroup arrives on both
// members' tickets and may owe two tiles.  THERE IS NO WAIT LOOP: a workgroup that is not last exits.
#include <stdlib.h>

#include "bwd_tile.h"
#include "fwd_bf_tile.h"

namespace mobody {

__device__ __forceinline__ bool opaque_true() {
  int one;
  asm volatile("s_mov_b32 %0, 1" : "=s"(one));
  return one != 0;
}

// blockIdx.y: [0, CHAINS) the chained workgroups (the longest are dispatched first), then Q(s,a) member 0 / 1, then pi(s).
// NT2: 16-column tiles of the actor's output layer; the twin-Q has one.
template <int PM, int NT2, int CHAINS>
__global__ __launch_bounds__(NTHREADS, PM == 4 ? FWD_F16_WAVES : 2) void k_critic_fwd_bf(Mlp3FwdArgs q, Mlp3FwdArgs pn, Mlp3FwdArgs qt, Mlp3FwdArgs pi,
                                                                                         FwdGather fg) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const int role = (int)blockIdx.y;
  CriticFwdTile ch;
  ch.Sa = Xs + split_lds_bytes<PM, TB>() / sizeof(float);
  ch.S = fg.g.S; ch.A = fg.g.A;
  ch.chained = role < CHAINS; ch.owes = role == 0;
  if (role < CHAINS) {
    // One call per tile, not a loop, and each behind a test the optimiser cannot see through (always true): in a loop, or in
    // straight-line code, it kept the tiles' common per-lane values (shuffle indices, LDS offsets) live from one tile into the
    // next -- 128 registers and a scratch frame of 60 to 250 bytes.  A tile's values now die with it.
    if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, NT2, false, true, CF_NEXT>(pn, 0, Xs, &fg, true, ch);
    if constexpr (CHAINS == 1) {
      if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q>(qt, 0, Xs, &fg, false, ch);
      if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q>(qt, 1, Xs, &fg, false, ch);
    } else {
      if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q>(qt, role, Xs, &fg, false, ch);
    }
  } else if (role < CHAINS + 2) {
    mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q>(q, role - CHAINS, Xs, &fg, false, ch);
  } else {
    mlp3_fwd_bf_tile<ACT_RELU, PM, NT2, false, true, CF_PI>(pi, 0, Xs, &fg, false, ch);
  }
}

// ---- the critic backward chained onto the one-chain form ----
// Ticket of (row tile, member): TICKET_IDLE, anything at all before the first launch on a workspace, or (epoch << 2) | 1 once the
// first of its two producers has arrived; epoch = the draw counter of the gather, which this launch reads and only a later launch
// advances.  An arrival is a compare-exchange: the word (epoch << 2) | 1 -- the other producer of THIS launch has arrived, its
// words are published -- becomes TICKET_IDLE and the arriver owes the tile; any other word -- idle, stale, arbitrary bytes, a word of
// a launch that was cut short -- becomes (epoch << 2) | 1.  TICKET_IDLE has 3 in the two low bits, so no epoch makes it read as
// "one arrived", and a launch leaves every ticket idle: the same call again, counter advanced or not, starts from idle words.  Two
// producers contend for a word and the first attempt is a guess, so a producer needs at most three attempts (guess wrong, lose
// the word to the other producer, complete); the loop is bounded all the same.
constexpr unsigned TICKET_IDLE = 0xffffffffu;
__device__ __forceinline__ bool ticket_arrive(unsigned* t, unsigned one) {
  unsigned old = one;                              // first guess "the other has arrived": the workgroup that goes on pays one round trip
  for (int k = 0; k < 4; ++k) {
    const bool last = old == one;
    if (__hip_atomic_compare_exchange_strong(t, &old, last ? TICKET_IDLE : one, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return last;
  }
  return false;
}

// The forward tile(s) of a workgroup, as k_critic_fwd_bf<PM, NT2, 1> runs them, with what the backward tiles read published.
template <int PM, int NT2>
__device__ __forceinline__ void critic_chain_fwd(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs& pi,
                                                 const FwdGather& fg, int role, float* Xs) {
  CriticFwdTile ch;
  ch.Sa = Xs + split_lds_bytes<PM, TB>() / sizeof(float);
  ch.S = fg.g.S; ch.A = fg.g.A;
  ch.chained = role == 0; ch.owes = role == 0;
  if (role == 0) {
    if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, NT2, false, true, CF_NEXT, true>(pn, 0, Xs, &fg, true, ch);
    if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q, true>(qt, 0, Xs, &fg, false, ch);
    if (opaque_true()) mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q, true>(qt, 1, Xs, &fg, false, ch);
  } else if (role < 3) {
    mlp3_fwd_bf_tile<ACT_RELU, PM, 1, false, true, CF_Q, true>(q, role - 1, Xs, &fg, false, ch);
  } else {
    mlp3_fwd_bf_tile<ACT_RELU, PM, NT2, false, true, CF_PI>(pi, 0, Xs, &fg, false, ch);
  }
}

// PARAMETER ORDER: `b` first -- the backward tiles read it at offset 0 of the kernel-argument segment behind an opaque copy of
// that address (as k_actor_bwd_chain reads its second block, mlp_bwd.hip: read as the parameter its invariant loads are hoisted
// into the forward tiles and held there).  blockIdx.y as k_critic_fwd_bf<., ., 1>: 0 the chained workgroup, 1 / 2 Q(s,a) of
// member 0 / 1, 3 pi(s).  tickets: [row tiles][2].
template <int PM, int NT2>
__global__ __launch_bounds__(NTHREADS, PM == 4 ? FWD_F16_WAVES : 2) void k_critic_chain_bf(Mlp3BwdArgs b, Mlp3FwdArgs q, Mlp3FwdArgs pn, Mlp3FwdArgs qt,
                                                                                           Mlp3FwdArgs pi, FwdGather fg, unsigned* tickets) {
  __shared__ float red[8];
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const int role = (int)blockIdx.y, tile = (int)blockIdx.x;
  critic_chain_fwd<PM, NT2>(q, pn, qt, pi, fg, role, Xs);
  if (role > 2) return;                                          // pi(s): nothing of it is read inside the launch
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's write-through stores are done
  __syncthreads();
  if (threadIdx.x < 2) {                                         // lane m arrives on member m's ticket: the chained workgroup on both at once
    bool last = false;
    if (role == 0 || role - 1 == (int)threadIdx.x) {
      const unsigned epoch = (unsigned)(fg.g.counter ? fg.g.counter[0] : 0);
      last = ticket_arrive(tickets + 2 * tile + threadIdx.x, (epoch << 2) | 1u);
    }
    red[threadIdx.x] = last ? 1.f : 0.f;
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");         // (no instruction: the agent-scope loads below stay below the tickets)
  const bool owes0 = red[0] != 0.f, owes1 = red[1] != 0.f;
  if (!owes0 && !owes1) return;
  lds_barrier();                                                 // everybody has read red before a seed's loss partials overwrite it
  static_assert(alignof(Mlp3BwdArgs) == 8, "`b` opens the kernel-argument segment");
  using KernArg = const __attribute__((address_space(4))) Mlp3BwdArgs;
  KernArg* ka = (KernArg*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  // (each tile behind an opaque test, as the forward tiles: its per-lane values die with it)
  if (owes0 && opaque_true()) mlp3_bwd_tile<false, 0, 1, PM, SEED_CRITIC_CHAIN>(*(const Mlp3BwdArgs*)ka, 0, tile, 2, Xs, red);
  if (owes0 && owes1) lds_barrier();                             // member 0's last LDS stores and its read of `red` are behind every wave
  if (owes1 && opaque_true()) mlp3_bwd_tile<false, 0, 1, PM, SEED_CRITIC_CHAIN>(*(const Mlp3BwdArgs*)ka, 1, tile, 2, Xs, red);
}

size_t critic_fwd_bf_lds(int S, int A) { return split_lds_bytes<4, TB>() + (size_t)TB * (S + A) * sizeof(float); }

template <int NT2, int CHAINS>
static int launch_critic_fwd_bf_t(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi, const FwdGather& fg,
                                  hipStream_t st) {
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_critic_fwd_bf<4, NT2, CHAINS>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_FWD, st);
  hipLaunchKernelGGL((k_critic_fwd_bf<4, NT2, CHAINS>), dim3((unsigned)cdiv(q.rows, TB), (unsigned)(CHAINS + 2 + (pi != nullptr ? 1 : 0))),
                     dim3(NTHREADS), critic_fwd_bf_lds(fg.g.S, fg.g.A), st, q, pn, qt, pi != nullptr ? *pi : Mlp3FwdArgs{}, fg);
  MB_LAUNCH_OK("k_critic_fwd_bf");
  return 0;
}

// Row tiles up to which the launch takes the two-chain form: its five workgroups per row block then number at most
// CRITIC_FWD_TWO_CHAIN_WGS, two per CU of the 256
#ifndef MOBODY_CRITIC_FWD_TWO_CHAIN_WGS            // A/B aid (build.py MOBODY_EXTRA_FLAGS)
#define MOBODY_CRITIC_FWD_TWO_CHAIN_WGS 512
#endif

template <int NT2>
static int launch_critic_chain_bf_t(const Mlp3BwdArgs& b, const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi,
                                    const FwdGather& fg, int* tickets, hipStream_t st) {
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_critic_chain_bf<4, NT2>, CRITIC_FWD_LDS_MAX);   // (dynamic bytes: the kernel also has `red`, static)
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_FWD, st);
  hipLaunchKernelGGL((k_critic_chain_bf<4, NT2>), dim3((unsigned)cdiv(q.rows, TB), (unsigned)(3 + (pi != nullptr ? 1 : 0))), dim3(NTHREADS),
                     critic_fwd_bf_lds(fg.g.S, fg.g.A), st, b, q, pn, qt, pi != nullptr ? *pi : Mlp3FwdArgs{}, fg, reinterpret_cast<unsigned*>(tickets));
  MB_LAUNCH_OK("k_critic_chain_bf");
  return 0;
}

// launch_critic_forward_gather (mlp_fwd.hip) has checked the shapes; pi null: no pi(s).  bq (or null) / tickets: the critic backward
// of the same step (seed mode 1 on sign words and W2^T planes, f16x2, no dx) and its 2 x row tiles ticket words; *chained tells
// whether the launch ran it (the one-chain form does, the two-chain form of small batches keeps the separate backward launch)
int launch_critic_fwd_bf(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi, const FwdGather& fg,
                         hipStream_t st, const Mlp3BwdArgs* bq, int* tickets, bool* chained) {
  const bool two = 5 * cdiv(q.rows, TB) <= MOBODY_CRITIC_FWD_TWO_CHAIN_WGS;
  if (chained != nullptr) *chained = false;
#ifndef MOBODY_NO_CRITIC_CHAIN                     // A/B aid (build.py MOBODY_EXTRA_FLAGS): the separate backward launch everywhere
  if (!two && bq != nullptr && tickets != nullptr && chained != nullptr && bq->seed.mode == 1 && bq->seed.qnext == nullptr &&
      bq->prec == PREC_F16X2 && bq->w2t_planes != nullptr && bq->m1 != nullptr && bq->m2 != nullptr && !bq->swish && bq->rows == q.rows &&
      bq->seed.q == q.out && bq->seed.qt == qt.out && bq->seed.r == fg.g.reward && bq->seed.nd == fg.g.not_done && bq->m1 == q.mask1 &&
      bq->m2 == q.mask2) {
    *chained = true;
    return pn.Np3 == 32 ? launch_critic_chain_bf_t<2>(*bq, q, pn, qt, pi, fg, tickets, st) : launch_critic_chain_bf_t<1>(*bq, q, pn, qt, pi, fg, tickets, st);
  }
#endif
  if (pn.Np3 == 32) return two ? launch_critic_fwd_bf_t<2, 2>(q, pn, qt, pi, fg, st) : launch_critic_fwd_bf_t<2, 1>(q, pn, qt, pi, fg, st);
  return two ? launch_critic_fwd_bf_t<1, 2>(q, pn, qt, pi, fg, st) : launch_critic_fwd_bf_t<1, 1>(q, pn, qt, pi, fg, st);
}

}  // namespace mobody
