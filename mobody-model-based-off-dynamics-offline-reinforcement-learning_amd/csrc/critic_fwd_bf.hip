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
#include <stdlib.h>

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

// launch_critic_forward_gather (mlp_fwd.hip) has checked the shapes; pi null: no pi(s)
int launch_critic_fwd_bf(const Mlp3FwdArgs& q, const Mlp3FwdArgs& pn, const Mlp3FwdArgs& qt, const Mlp3FwdArgs* pi, const FwdGather& fg,
                         hipStream_t st) {
  const bool two = 5 * cdiv(q.rows, TB) <= MOBODY_CRITIC_FWD_TWO_CHAIN_WGS;
  if (pn.Np3 == 32) return two ? launch_critic_fwd_bf_t<2, 2>(q, pn, qt, pi, fg, st) : launch_critic_fwd_bf_t<2, 1>(q, pn, qt, pi, fg, st);
  return two ? launch_critic_fwd_bf_t<1, 2>(q, pn, qt, pi, fg, st) : launch_critic_fwd_bf_t<1, 1>(q, pn, qt, pi, fg, st);
}

}  // namespace mobody
