// Fused 3-layer MLP forward with the 256 x 256 layer on the split-precision MFMA core (tile_bf.h): modes "bf16" / "bf16x2" /
// "bf16x3" / "f16x2" of the actor / twin-Q / reward-head forwards.  Layer 1 (K = the padded input width) and the output
// layer stay on exact fp32 MFMA; layer 1's epilogue writes its activations as 16-bit planes over the fp32 image (same LDS
// region: every layer separates its reads from its writes by a barrier), layer 2 contracts the planes with the weight
// planes kept in the T blob and writes an fp32 image for the output layer.
#include <stdlib.h>

#include "fwd_bf_tile.h"

namespace mobody {

// one or two independent networks per launch (blockIdx.y < members_a -> net a), as k_mlp3_fwd2
// NT / NT2: output-layer width (16-column tiles; 0 = any) of net a / net b -- a twin-Q (one output) and an actor with more than
// 16 actions (pen: 24) still share a launch
template <int ACT, int PM, int NT, bool DS = false, int NT2 = NT>
__global__ __launch_bounds__(NTHREADS, (PM == 4 && !DS) ? FWD_F16_WAVES : 2) void k_mlp3_fwd_bf(Mlp3FwdArgs a, Mlp3FwdArgs b, int members_a) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const bool second = (int)blockIdx.y >= members_a;
  const Mlp3FwdArgs s = second ? b : a;
  if ((long long)blockIdx.x * TB >= s.rows) return;
  if constexpr (NT2 == NT) {
    mlp3_fwd_bf_tile<ACT, PM, NT, DS>(s, second ? (int)blockIdx.y - members_a : (int)blockIdx.y, Xs);
  } else {
    if (second) mlp3_fwd_bf_tile<ACT, PM, NT2, DS>(s, (int)blockIdx.y - members_a, Xs);
    else mlp3_fwd_bf_tile<ACT, PM, NT, DS>(s, (int)blockIdx.y, Xs);
  }
}

// The paired ReLU launch with the gathering input stage (a kernel of its own: the stage's arguments are a fourth kernel
// argument, and every other instance keeps its signature and its code).  Same occupancy target as its plain twin.
template <int PM, int NT, int NT2 = NT>
__global__ __launch_bounds__(NTHREADS, PM == 4 ? FWD_F16_WAVES : 2) void k_mlp3_fwd_bf_gather(Mlp3FwdArgs a, Mlp3FwdArgs b, int members_a, FwdGather fg) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  const bool second = (int)blockIdx.y >= members_a;
  const Mlp3FwdArgs s = second ? b : a;
  if ((long long)blockIdx.x * TB >= s.rows) return;
  if constexpr (NT2 == NT) {
    mlp3_fwd_bf_tile<ACT_RELU, PM, NT, false, true>(s, second ? (int)blockIdx.y - members_a : (int)blockIdx.y, Xs, &fg, second);
  } else {
    if (second) mlp3_fwd_bf_tile<ACT_RELU, PM, NT2, false, true>(s, (int)blockIdx.y - members_a, Xs, &fg, true);
    else mlp3_fwd_bf_tile<ACT_RELU, PM, NT, false, true>(s, (int)blockIdx.y, Xs, &fg, false);
  }
}

template <int PM, int NT, int NT2 = NT>
static int launch_bf_gather_t(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<PM, TB>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_fwd_bf_gather<PM, NT, NT2>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_MLP_FWD, st);
  hipLaunchKernelGGL((k_mlp3_fwd_bf_gather<PM, NT, NT2>), dim3((unsigned)cdiv(a.rows, TB), (unsigned)(members_a + members_b)),
                     dim3(NTHREADS), lds, st, a, b, members_a, fg);
  MB_LAUNCH_OK("k_mlp3_fwd_bf_gather");
  return 0;
}

// the pairs the gathering kernels are built for (launch_mlp3_forward_gather has checked them): a one-output twin-Q next to
// an actor of up to 16 actions in every split mode, of up to 32 in f16x2
int launch_mlp3_fwd_bf_gather(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, const FwdGather& fg,
                              int prec, hipStream_t st) {
  if (prec == PREC_F16X2 && b.Np3 == 32) return launch_bf_gather_t<4, 1, 2>(a, members_a, b, members_b, fg, st);
  switch (prec) {
    case PREC_BF16: return launch_bf_gather_t<1, 1>(a, members_a, b, members_b, fg, st);
    case PREC_BF16X2: return launch_bf_gather_t<2, 1>(a, members_a, b, members_b, fg, st);
    case PREC_BF16X3: return launch_bf_gather_t<3, 1>(a, members_a, b, members_b, fg, st);
    default: return launch_bf_gather_t<4, 1>(a, members_a, b, members_b, fg, st);
  }
}

template <int ACT, int PM, int NT, bool DS = false, int NT2 = NT>
static int launch_bf_t(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<PM, TB>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_mlp3_fwd_bf<ACT, PM, NT, DS, NT2>, 160 * 1024);
    if (rc) return rc;
    once = true;
  }
  const long long rows = a.rows > b.rows ? a.rows : b.rows;
  ProfScope prof(PROF_MLP_FWD, st);
  hipLaunchKernelGGL((k_mlp3_fwd_bf<ACT, PM, NT, DS, NT2>), dim3((unsigned)cdiv(rows, TB), (unsigned)(members_a + members_b)),
                     dim3(NTHREADS), lds, st, a, b, members_a);
  MB_LAUNCH_OK("k_mlp3_fwd_bf");
  return 0;
}

template <int ACT, int PM>
static int launch_bf_nt(const Mlp3FwdArgs& a, int ma, const Mlp3FwdArgs& b, int mb, hipStream_t st) {
  if constexpr (PM == 4 && ACT == ACT_RELU) {       // f16x2: the mixed pair launch_mlp3_forward lets through, widths 16 | 32
    if (mb > 0 && a.Np3 != b.Np3)
      return a.Np3 == 16 ? launch_bf_t<ACT, PM, 1, false, 2>(a, ma, b, mb, st) : launch_bf_t<ACT, PM, 2, false, 1>(a, ma, b, mb, st);
  }
  return dispatch_out_width(a.Np3, [&](auto nt) { return launch_bf_t<ACT, PM, decltype(nt)::value>(a, ma, b, mb, st); });
}

// prec: 1 bf16, 2 bf16x2, 3 bf16x3, 4 f16x2.  Net a (non-empty) alone, or with a ReLU net b that launch_mlp3_forward found to share
// the launch.
// Workgroup shape: 32-row tiles of four waves.  Measured alternatives that lost (removed; they live in the history before
// this shape became the only one):
//   * two row groups (eight waves) sharing each weight fragment: twin-Q forward at 10 240 rows 41.5 us against 28.8 us in
//     bf16x3 (39.5 us in fp32);
//   * 64-row tiles in the f16x2 ReLU launches (each weight fragment feeds two row tiles, half the L2 -> CU weight stream, two
//     workgroups per CU): they win only on a bare twin-Q forward of several generations (40 960 rows: 48.3 us against 50.8;
//     10 240 rows: 19.8 against 17.4) and lose in the train step, whose forwards also save activations: c3 forward 302
//     against 297 us per step, c4 280 against 258.
int launch_mlp3_fwd_bf(const Mlp3FwdArgs& a, int members_a, const Mlp3FwdArgs& b, int members_b, int act, int prec, hipStream_t st) {
  if (a.save_d1 != nullptr || a.save_d2 != nullptr) {  // training forward of a Swish net (dynamics pre-training): f16x2, one net
    if (act != ACT_SWISH || prec != PREC_F16X2 || members_b != 0 || !a.save_d1 || !a.save_d2)
      return fail(MOBODY_E_ARG, "launch_mlp3_fwd_bf: derivative saves need one Swish net in the f16x2 mode");
    return dispatch_out_width(a.Np3, [&](auto nt) { return launch_bf_t<ACT_SWISH, 4, decltype(nt)::value, true>(a, members_a, b, 0, st); });
  }
#define BF_CASE(ACT, PM) launch_bf_nt<ACT, PM>(a, members_a, b, members_b, st)
  if (act == ACT_SWISH) return prec == PREC_BF16 ? BF_CASE(ACT_SWISH, 1) : prec == PREC_BF16X2 ? BF_CASE(ACT_SWISH, 2) : prec == PREC_BF16X3 ? BF_CASE(ACT_SWISH, 3) : BF_CASE(ACT_SWISH, 4);
  return prec == PREC_BF16 ? BF_CASE(ACT_RELU, 1) : prec == PREC_BF16X2 ? BF_CASE(ACT_RELU, 2) : prec == PREC_BF16X3 ? BF_CASE(ACT_RELU, 3) : BF_CASE(ACT_RELU, 4);
#undef BF_CASE
}

}  // namespace mobody
