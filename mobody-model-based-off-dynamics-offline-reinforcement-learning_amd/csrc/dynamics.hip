// Ensemble-dynamics imagined transition (the "rollout kernel" family).
//
//   k_dyn_fwd      mean[e,b,:] = forward_trg/forward_src(obs, act)   mobody_module.py:315-330
//                  one workgroup = 64 rows x ONE member, the 9 ensemble layers
//                  (zs1-3, za1-2, transition1-3) chained through one LDS image;
//                  grid = (ceil(B/64), 7) so even B = 4096 fills the chip (448 WGs).
//   k_dyn_sample   ensemble std, Gaussian sample of the elite member, the penalty of the
//                  uncertainty mode (pairwise-diff | aleatoric | ensemble_std), termination predicate
//                  (one thread per (row, state dim), whole rows per
//                  workgroup)                                       mobody_dynamics.py:218-256,
//                                                                    terminal_funs.py:10-113
//   reward head    generic fused MLP forward (Swish) on [s,a,s']     mobody_module.py:295-302
//   k_dyn_finalize reward = mean_e r_mu - coef*penalty               mobody_dynamics.py:236,261-263
//   k_eval_account (trajectory_return.hip) in k_dyn_finalize's place under mobody_ens_evaluate
//
// Roofline: k_dyn_fwd / reward head are MFMA-f32 bound (3.36 MFLOP per transition at
// S=17,A=6 against 240 algorithmic bytes); k_dyn_sample / k_dyn_finalize are HBM-bound
// streaming kernels over [E,B,S] floats.
#include "common.h"
#include "health.h"
#include "layers_bf.h"
#include "rng.h"
#include "term.h"

namespace mobody {

struct DynFwdArgs {
  const float* blob;
  MobodyDynLayout L;
  const float* obs;
  const float* act;
  float* mean;        // [E][B][S]
  long long B;
  int use_trg;
  const unsigned short* planes;   // split-precision modes: 16-bit planes of zs2 | transition2 | reward_model2 (dyn_planes_off)
};

// NT3: 16-column tiles of the transition head handled by the K-split narrow layer (Np == 16*NT3: 1, 2, 3 or 7), 0 = any width
// (row-split narrow_layer: half of the waves idle on a 32-row tile).
// PM: 0 = exact fp32 MFMA; 1..4 = the two 256 x 256 layers (zs2, transition2) on the split-precision core (tile_bf.h).
template <int MT, int NT3, int PM>
__global__ __launch_bounds__(NTHREADS, 2) void k_dyn_fwd(DynFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float Xs[];
  constexpr int TB = 32 * MT;
  constexpr int PMX = PM > 0 ? PM : 1;
  char* Ps = reinterpret_cast<char*>(Xs);
  float* scr = reinterpret_cast<float*>(Ps + split_scr_offset<PMX, TB>());
  BfRing<PMX> bring;
  const int e = blockIdx.y;
  const long long row0 = (long long)blockIdx.x * TB;
  const int rows_here = (int)min((long long)TB, a.B - row0);
  const int S = a.L.S, A = a.L.A;
  const int lane = lane_id(), w = wave_id();
  auto Wp = [&](int l) { return a.blob + a.L.layer[l].w_off + (long long)e * a.L.layer[l].Kp * a.L.layer[l].Np; };
  auto Bp = [&](int l) { return a.blob + a.L.layer[l].b_off + (long long)e * a.L.layer[l].Np; };

  // ---- state encoder: zs = mu-half of zs3(Sw(zs2(Sw(zs1(s)))))   (encode_state :217-225) ----
  // every wide layer's first weight fragments are requested one phase early (see wide_prefetch)
  WideRing ring;
  wide_prefetch(Wp(MOBODY_DL_ZS1), a.L.layer[MOBODY_DL_ZS1].Kp, ring);
  tile_load(Xs, 0, a.obs + row0 * S, S, S, 0, rows_here, TB);
  tile_zero_cols(Xs, S, a.L.layer[MOBODY_DL_ZS1].Kp, TB);
  lds_barrier();
  if constexpr (PM > 0) {
    const s16x8* pz = reinterpret_cast<const s16x8*>(a.planes + dyn_planes_off(0, e));
    const int ez = wide_layer_to_planes<ACT_SWISH, MT, PMX, TB>(Xs, Ps, scr, Wp(MOBODY_DL_ZS1), Bp(MOBODY_DL_ZS1),
                                                                a.L.layer[MOBODY_DL_ZS1].Kp, ring,
                                                                [&] { bf_prefetch<PMX>(pz, bring); });
    bf_layer<ACT_SWISH, MT, PMX, TB>(Xs, Ps, ez, pz, Bp(MOBODY_DL_ZS2), bring, [] {});
  } else {
    wide_layer<ACT_SWISH, MT>(Xs, Wp(MOBODY_DL_ZS1), Bp(MOBODY_DL_ZS1), a.L.layer[MOBODY_DL_ZS1].Kp, ring, NoExtra{},
                              [&] { wide_prefetch(Wp(MOBODY_DL_ZS2), HID, ring); });
    wide_layer<ACT_SWISH, MT>(Xs, Wp(MOBODY_DL_ZS2), Bp(MOBODY_DL_ZS2), HID, ring, NoExtra{}, [] {});
  }

  // From here to the latent sum every wave works on its own 16 rows: no barriers needed (waves without rows idle).
  if (16 * w < TB) {
    const int i = lane & 15, q = lane >> 4;
    float* myrow = Xs + (16 * w + 4 * q) * LDX;       // rows 16w+4q+r, r = 0..3 (C/D map of 16x16 MFMA)
    f32x4 zs[1];
    narrow_gemm<1>(Xs, Wp(MOBODY_DL_ZS3), HID, 16, 0, zs, TB);
    {
      const float b = Bp(MOBODY_DL_ZS3)[i];
#pragma unroll
      for (int r = 0; r < 4; ++r) { zs[0][r] += b; myrow[r * LDX + i] = zs[0][r]; }
    }
    // ---- action encoder on [zs, a]   (encode_trg_action :258-271 / encode_src_action :245-256) ----
    const int la1 = a.use_trg ? MOBODY_DL_ZA_TRG1 : MOBODY_DL_ZA_SRC1;
    const int la2 = a.use_trg ? MOBODY_DL_ZA_TRG2 : MOBODY_DL_ZA_SRC2;
    const int Kza = a.L.layer[la1].Kp;
    for (int idx = lane; idx < 16 * (Kza - LATENT); idx += 64) {
      const int r = idx / (Kza - LATENT), c = idx - r * (Kza - LATENT);
      const int row = 16 * w + r;
      const float v = a.act[(row0 + min(row, rows_here - 1)) * A + min(c, A - 1)];      // unconditional, clamped
      Xs[row * LDX + LATENT + c] = (c < A && row < rows_here) ? v : 0.f;
    }
    f32x4 g[2];
    narrow_gemm<2>(Xs, Wp(la1), Kza, 32, 0, g, TB);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const float b = Bp(la1)[16 * n + i];
#pragma unroll
      for (int r = 0; r < 4; ++r) myrow[r * LDX + 16 * n + i] = activate<ACT_SWISH>(g[n][r] + b);
    }
    f32x4 za[1];
    narrow_gemm<1>(Xs, Wp(la2), 32, 16, 0, za, TB);
    {
      const float b = Bp(la2)[i];
#pragma unroll
      for (int r = 0; r < 4; ++r) myrow[r * LDX + i] = zs[0][r] + za[0][r] + b;     // z_ns = zs + za  (:319,327)
    }
  }
  lds_barrier();

  // ---- transition decoder   (encode_transition :287-293) ----
  wide_prefetch(Wp(MOBODY_DL_TR1), 16, ring);
  const s16x8* pt = PM > 0 ? reinterpret_cast<const s16x8*>(a.planes + dyn_planes_off(1, e)) : nullptr;
  int et = 0;
  if constexpr (PM > 0)
    et = wide_layer_to_planes<ACT_SWISH, MT, PMX, TB>(Xs, Ps, scr, Wp(MOBODY_DL_TR1), Bp(MOBODY_DL_TR1), 16, ring,
                                                      [&] { bf_prefetch<PMX>(pt, bring); });
  else
    wide_layer<ACT_SWISH, MT>(Xs, Wp(MOBODY_DL_TR1), Bp(MOBODY_DL_TR1), 16, ring, NoExtra{},
                              [&] { wide_prefetch(Wp(MOBODY_DL_TR2), HID, ring); });
  const float* b3 = Bp(MOBODY_DL_TR3);
  float* mean = a.mean + ((long long)e * a.B + row0) * S;
  // transition2 at the requested precision; `between` runs after its last MFMA (the output layer's early requests)
  auto layer_tr2 = [&](auto&& between) {
    if constexpr (PM > 0) bf_layer<ACT_SWISH, MT, PMX, TB>(Xs, Ps, et, pt, Bp(MOBODY_DL_TR2), bring, between);
    else wide_layer<ACT_SWISH, MT>(Xs, Wp(MOBODY_DL_TR2), Bp(MOBODY_DL_TR2), HID, ring, NoExtra{}, between);
  };
  if constexpr (NT3 > 0) {
    NarrowRegs<NT3> br;
    const int mycol = threadIdx.x % (16 * NT3);          // column of every output element this thread finishes
    float bias;
    layer_tr2([&] {
      narrow_prefetch<NT3>(Wp(MOBODY_DL_TR3), 16 * NT3, br);
      bias = b3[mycol < S ? mycol : 0];
    });
    if constexpr (NT3 > 2) {                             // wide heads (pen 48, ant 112 columns): 32-row passes, bias by column
      narrow_run_wide<TB / 16, NT3>(Xs, br, [&](int row, int col, float v) {
        if (row < rows_here && col < S) mean[row * S + col] = v + b3[col];
      });
    } else {
      narrow_run<TB / 16, NT3>(Xs, br, [&](int row, int col, float v) {
        if (row < rows_here && col < S) mean[row * S + col] = v + bias;
      });
    }
  } else {
    layer_tr2([] {});
    narrow_layer(Xs, Wp(MOBODY_DL_TR3), HID, a.L.layer[MOBODY_DL_TR3].Np, [&](int row, int col, float v) {
      if (row < rows_here && col < S) mean[row * S + col] = v + b3[col];
    }, TB);
  }
}

// ------------------------------------------------------------------------------------------
struct DynSampleArgs {
  const float* mean;         // [E][B][S]
  const float* noise;        // [E][B][S] or null
  const int32_t* elite_idx;  // [B] or null
  const uint8_t* alive;      // [B] or null
  int32_t elites[NENS];
  int n_elites;
  uint32_t seed, call;
  const long long* call_dev; // optional device word added to `call` (graph replay: the step counter lives on the device)
  long long B;
  int S, task;
  float* next_obs;           // [B][S]
  float* penalty;            // [B]
  uint8_t* terminal;         // [B]
  // multi-step rollout bookkeeping fused in (MOBODY.rollout mobody.py:635-653 without host compaction), both optional:
  uint8_t* keep;             // [B] alive_in && (!use_filter || penalty <= env_filter)
  uint8_t* alive_out;        // [B] alive_in && !terminal   (may alias `alive`)
  float env_filter;
  int use_filter;
};

// One thread per (row, state dim) element, a workgroup owns rpb = 256 / S whole rows: the member means, the noise and
// next_obs are read / written at consecutive addresses by consecutive lanes.  (The first version used one thread per
// row walking its S floats: every store instruction scattered 64 dwords over 64 rows and WRITE_SIZE showed 10x the
// algorithmic bytes.)  The per-row sums over d (penalty) go through LDS and are added in increasing d by one thread
// per (row, member): same order as a serial loop, no atomics.
//
// MODE = uncertainty_mode of the reference's step() (mobody_dynamics.py:241-252); all three are built from the squared
// deviations t^2 = (mean_e - avg)^2 the sample already holds in LDS, so no mode reads or writes anything more than the default:
//   MOBODY_UNC_PAIRWISE   amax_e ||mean_e - avg||_2 over d < S-1                                        (:246-249)
//   MOBODY_UNC_ALEATORIC  amax_e ||std_e||_2 with std = torch.std(mean, 0) repeated over the members: seven equal norms,
//                         sqrt(sum_{d < S} var_d), var_d = sum_e t^2 / 6 -- the last state dim is NOT dropped  (:241-243)
//   MOBODY_UNC_ENS_STD    sqrt(mean_{d < S-1} var_d)                                                     (:250-252)
// The two barriers order LDS traffic only (nothing global is handed between threads).
template <int MODE>
__global__ __launch_bounds__(256) void k_dyn_sample(DynSampleArgs a, int rpb) {
  __shared__ float s_nxt[256];
  __shared__ float s_t2[256 * NENS];
  __shared__ float s_sq[64 * NENS];
  const int S = a.S;
  const int tid = threadIdx.x;
  const int r = tid / S, d = tid - r * S;
  const long long row0 = (long long)blockIdx.x * rpb;
  const long long b = row0 + r;
  const uint32_t call = a.call + (a.call_dev != nullptr ? (uint32_t)a.call_dev[0] : 0u);
  if (r < rpb && b < a.B) {
    int e_sel;
    if (a.elite_idx) e_sel = a.elite_idx[b];
    else e_sel = a.elites[rng_index_at(a.seed, STREAM_ELITE, call, (uint64_t)b, (uint32_t)a.n_elites)];
    float mval[NENS], avg = 0.f, msel = 0.f;
#pragma unroll
    for (int e = 0; e < NENS; ++e) {
      mval[e] = a.mean[((long long)e * a.B + b) * S + d];
      avg += mval[e];
      msel = (e == e_sel) ? mval[e] : msel;
    }
    avg *= (1.f / NENS);
    float var = 0.f;
#pragma unroll
    for (int e = 0; e < NENS; ++e) { const float t = mval[e] - avg; var += t * t; s_t2[tid * NENS + e] = t * t; }
    const float sd = sqrtf(var * (1.f / (NENS - 1)));                      // torch.std: unbiased (:218)
    float eps;
    if (a.noise) eps = a.noise[((long long)e_sel * a.B + b) * S + d];
    else eps = rng_normal_at(a.seed, STREAM_NOISE, call, (uint64_t)b * S + d);
    const float v = msel + eps * sd;                                       // :220-226
    a.next_obs[b * S + d] = v;
    s_nxt[tid] = v;
  }
  lds_barrier();
  const int nd = MODE == MOBODY_UNC_ALEATORIC ? S : S - 1;                 // state dims under the sum
  for (int t = tid; t < rpb * NENS; t += 256) {                            // (row, member): sum over d < nd, in order
    const int rr = t / NENS, e = t - rr * NENS;
    float sq = 0.f;
    for (int dd = 0; dd < nd; ++dd) sq += s_t2[(rr * S + dd) * NENS + e];
    s_sq[t] = sq;
  }
  lds_barrier();
  if (tid < rpb && row0 + tid < a.B) {
    const long long bb = row0 + tid;
    if constexpr (MODE == MOBODY_UNC_PAIRWISE) {
      // torch.amax propagates NaN (one non-finite member makes every norm of the row NaN); fmaxf would drop it and
      // the row would pass `penalty <= env_filter` with NaN next_obs, where the reference's comparisons are all False
      float pmax = 0.f;
      bool bad = false;
#pragma unroll
      for (int e = 0; e < NENS; ++e) { const float q = s_sq[tid * NENS + e]; bad = bad || (q != q); pmax = fmaxf(pmax, q); }
      a.penalty[bb] = bad ? __builtin_nanf("") : sqrtf(pmax);              // :246-249 (last state dim dropped)
    } else {
      // sum_d var_d = (sum_e sum_d t^2) / 6: plain adds, so a non-finite member mean (t = NaN for every member of that
      // dim, through the average) makes the row's penalty NaN as torch.var / norm / sqrt do
      float tot = 0.f;
#pragma unroll
      for (int e = 0; e < NENS; ++e) tot += s_sq[tid * NENS + e];
      const float den = MODE == MOBODY_UNC_ALEATORIC ? (float)(NENS - 1) : (float)(NENS - 1) * (float)(S - 1);
      a.penalty[bb] = sqrtf(tot / den);                                    // :241-243 | :250-252
    }
    bool done = term_predicate(a.task, s_nxt + tid * S, S);
    const bool was_alive = a.alive ? a.alive[bb] != 0 : true;
    if (!was_alive) done = true;
    a.terminal[bb] = done ? 1 : 0;
    const float pen = a.penalty[bb];
    if (a.keep) a.keep[bb] = (was_alive && (!a.use_filter || pen <= a.env_filter)) ? 1 : 0;     // NaN penalty: dropped (:648-653)
    if (a.alive_out) a.alive_out[bb] = (was_alive && !done) ? 1 : 0;
  }
}

struct DynFinalArgs {
  const float* r_mu;     // [E][B]
  const float* penalty;  // [B]
  float* reward;         // [B]
  float* raw_reward;     // [B] or null
  long long B;
  float coef;            // penalty_coef if (penalty_coef && use_penalty) else 0
};

__global__ __launch_bounds__(256) void k_dyn_finalize(DynFinalArgs a) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < NENS; ++e) s += a.r_mu[(long long)e * a.B + b];
  const float raw = s * (1.f / NENS);                                     // reward.mean(0) :236
  if (a.raw_reward) a.raw_reward[b] = raw;
  a.reward[b] = (a.coef != 0.f) ? raw - a.coef * a.penalty[b] : raw;       // :261-263
}

template <int MT, int NT3, int NPL>
static int launch_dyn_fwd_t(const DynFwdArgs& a, hipStream_t st) {
  constexpr size_t lds = split_lds_bytes<(NPL > 0 ? NPL : 1), 32 * MT>();
  static bool once = false;
  if (!once) {
    int rc = allow_big_lds(k_dyn_fwd<MT, NT3, NPL>, lds);
    if (rc) return rc;
    once = true;
  }
  ProfScope prof(PROF_DYN_FWD, st);
  hipLaunchKernelGGL((k_dyn_fwd<MT, NT3, NPL>), dim3((unsigned)cdiv(a.B, 32 * MT), NENS), dim3(NTHREADS), lds, st, a);
  MB_LAUNCH_OK("k_dyn_fwd");
  return 0;
}
template <int MT, int NPL>
static int launch_dyn_fwd_nt(const DynFwdArgs& a, int nt3, hipStream_t st) {
  return nt3 == 1 ? launch_dyn_fwd_t<MT, 1, NPL>(a, st) : nt3 == 2 ? launch_dyn_fwd_t<MT, 2, NPL>(a, st)
       : nt3 == 3 ? launch_dyn_fwd_t<MT, 3, NPL>(a, st) : nt3 == 7 ? launch_dyn_fwd_t<MT, 7, NPL>(a, st) : launch_dyn_fwd_t<MT, 0, NPL>(a, st);
}

static int launch_dyn_fwd(const float* blob, const MobodyDynLayout& L, const float* obs, const float* act, long long B,
                          int use_trg, float* mean, const float* planes, int prec, hipStream_t st) {
  DynFwdArgs a{blob, L, obs, act, mean, B, use_trg, reinterpret_cast<const unsigned short*>(planes)};
  // 64-row tiles (MT = 2) for fp32: the nine-layer chain has a wave-local narrow section in which a 32-row tile idles
  // half of the waves (measured 102 vs 88 TFLOP/s at 50 000 rows).
  const int np = L.layer[MOBODY_DL_TR3].Np;
  const int nt3 = np == 16 ? 1 : np == 32 ? 2 : np == 48 ? 3 : np == 112 ? 7 : 0;      // walker/hopper/cheetah, pen, ant heads; else generic
  if (prec == PREC_F32) return launch_dyn_fwd_nt<2, 0>(a, nt3, st);
  // split-precision modes: the planes of a 64-row tile are 32 / 64 / 96 KB for 1 / 2 / 3 terms -> the three-term mode
  // runs 32-row tiles (MT = 1: 48 KB, three workgroups per CU), the others 64-row tiles
  if (prec == PREC_BF16) return launch_dyn_fwd_nt<2, 1>(a, nt3, st);
  if (prec == PREC_BF16X2) return launch_dyn_fwd_nt<2, 2>(a, nt3, st);
  if (prec == PREC_F16X2) return launch_dyn_fwd_nt<2, 4>(a, nt3, st);
  return launch_dyn_fwd_nt<1, 3>(a, nt3, st);
}

// zs2 / transition2 / reward_model2 of every member -> their three bf16 planes (precision 0-3) or two fp16 planes of
// w * 2^F16_WSHIFT (precision 4)
__global__ __launch_bounds__(256) void k_dyn_planes(const float* blob, MobodyDynLayout L, short* planes, int precision, int* health) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 3LL * NENS * HID * HID) return;
  const int layer = (int)(gid / ((long long)NENS * HID * HID));
  const long long rem = gid - (long long)layer * NENS * HID * HID;
  const int e = (int)(rem / (HID * HID)), el = (int)(rem % (HID * HID)), k = el / HID, n = el % HID;
  const int li = layer == 0 ? MOBODY_DL_ZS2 : layer == 1 ? MOBODY_DL_TR2 : MOBODY_DL_RW2;
  const float w = blob[L.layer[li].w_off + (long long)e * HID * HID + wide_idx(k, n)];
  short* pl = planes + dyn_planes_off(layer, e);
  if (precision == 4) {
    short t[2];
    split_terms<4>(w * exp2i(F16_WSHIFT), t);
#pragma unroll
    for (int p = 0; p < 2; ++p) pl[bf_plane_idx(p, k, n)] = t[p];
    health_check_f16(health, w);
  } else {
    short t[3];
    split_terms<3>(w, t);
#pragma unroll
    for (int p = 0; p < 3; ++p) pl[bf_plane_idx(p, k, n)] = t[p];
  }
}

}  // namespace mobody

using namespace mobody;

extern "C" int64_t mobody_dyn_planes_floats(void) { return 3LL * NENS * DYN_PLANE_MEMBER / 2; }

extern "C" int mobody_dyn_planes(const float* dyn_blob, int S, int A, float* planes, int precision, void* stream) {
  MobodyDynLayout L;
  int rc = mobody_dyn_layout(S, A, &L);
  if (rc) return rc;
  MB_REQUIRE(dyn_blob && planes, "mobody_dyn_planes: null pointer");
  rc = check_precision("mobody_dyn_planes", precision, true);
  if (rc) return rc;
  hipLaunchKernelGGL(k_dyn_planes, dim3((unsigned)cdiv(3LL * NENS * HID * HID, 256)), dim3(256), 0, as_stream(stream), dyn_blob, L,
                     reinterpret_cast<short*>(planes), precision, health_words());
  MB_LAUNCH_OK("k_dyn_planes");
  return 0;
}

extern "C" int mobody_dyn_forward(const float* dyn_blob, const float* dyn_planes, int precision, int S, int A, const float* obs,
                                  const float* act, int64_t B, int use_trg, float* mean, void* stream) {
  MobodyDynLayout L;
  int rc = mobody_dyn_layout(S, A, &L);
  if (rc) return rc;
  MB_REQUIRE(B >= 0, "mobody_dyn_forward: B < 0");
  if (B == 0) return 0;                      // empty batch: nothing to do (pointers may be null)
  MB_REQUIRE(dyn_blob && obs && act && mean, "mobody_dyn_forward: null pointer");
  rc = check_precision("mobody_dyn_forward", precision, dyn_planes != nullptr);
  if (rc) return rc;
  return launch_dyn_fwd(dyn_blob, L, obs, act, B, use_trg, mean, dyn_planes, precision, as_stream(stream));
}

// ---- the ensemble step: one host path for the single step and the three trajectory drivers --------------------------
namespace mobody {

// floats of the step's own workspace: the ensemble means [E][B][S] and the per-member reward means [E][B]
static long long dyn_step_floats(int S, long long B) { return (long long)NENS * B * S + (long long)NENS * B; }

#define MB_NONNULL(who, blk, f) MB_REQUIRE((blk).f != nullptr, "%s: null pointer " #f, who)

// the rollout's bookkeeping, formed in the sample kernel (the last four fields of DynSampleArgs); every part optional
struct SampleBook { uint8_t *keep, *alive_out; float env_filter; int use_filter; };

// The model a call runs: what the four argument blocks share, read out of a block once (MobodyEnsStep's `call` is its call0).
// mopo_blob != null: the MOPO ablation (config['mopo'], mobody_module.py:114-118,218-219,251-254,264-266,288-289) --
// mean[e] = obs + MLP_e([obs, act]) with the 7-member Swish MLP (S+A -> 256 -> 256 -> S) za_src1..3 packed as
// mobody_mlp_layout(S + A, S, 7); encoders and decoder are bypassed, forward_trg == forward_src.  Everything after the means
// (std, sample, reward head, penalty, termination) is the same code.
struct EnsModel {
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T;
  int precision, S, A, task;
  const int32_t* elites; int n_elites;
  uint32_t seed, call0; const int64_t* call_dev;
  int use_trg, uncertainty_mode;
  MobodyDynLayout L; MobodyMlpLayout ML;       // set by check(): the ensemble's layers and, for the mopo model, its MLP

  template <class Block>
  static EnsModel of(const Block& a, uint32_t call0) {
    return {a.dyn_blob, a.dyn_planes, a.mopo_blob, a.mopo_blob_T, a.precision, a.S, a.A, a.task, a.elites,
            a.n_elites, a.seed, call0, a.call_dev, a.use_trg, a.uncertainty_mode};
  }

  // the rules an empty batch is held to as well
  int check_batch(const char* who, int64_t B) const {
    MB_REQUIRE(uncertainty_mode >= MOBODY_UNC_PAIRWISE && uncertainty_mode <= MOBODY_UNC_ENS_STD,
               "%s: unknown uncertainty_mode %d (0 pairwise-diff, 1 aleatoric, 2 ensemble_std)", who, uncertainty_mode);
    MB_REQUIRE(B >= 0, "%s: B < 0", who);
    return 0;
  }

  // The range and pointer rules of a batch with rows, every refusal naming its field; then the layouts.  `who`: the public
  // entry point named in error texts.  need_elites false: the single step was handed per-row picks (elite_idx).
  int check(const char* who, bool need_elites = true) {
    MB_REQUIRE(dyn_blob, "%s: null pointer dyn_blob", who);
    MB_REQUIRE(!need_elites || elites, "%s: null pointer elites", who);
    MB_REQUIRE(!need_elites || (n_elites >= 1 && n_elites <= NENS), "%s: n_elites %d outside 1..7", who, n_elites);
    int rc = check_precision(who, precision, dyn_planes != nullptr);
    if (rc) return rc;
    MB_REQUIRE(precision == PREC_F32 || !mopo_blob || mopo_blob_T, "%s: the split-precision modes need the T blob of the MLP (mopo_blob_T)", who);
    MB_REQUIRE(task >= MOBODY_TERM_NEVER && task <= MOBODY_TERM_PEN, "%s: unknown termination id %d (task)", who, task);
    MB_REQUIRE(task != MOBODY_TERM_PEN || S > 26, "%s: pen predicate needs S > 26 (task)", who);
    rc = mobody_dyn_layout(S, A, &L);
    if (rc || !mopo_blob) return rc;
    return mobody_mlp_layout(S + A, S, NENS, &ML);
  }

  // The MobodyEnsStep of trajectory step t on the rows (obs, act): call id call0 + t (uint32 wrap; the kernel adds
  // call_dev[0]).  The caller adds its outputs and workspace (the single step also noise, elite_idx and its penalty form).
  MobodyEnsStep step(int t, const float* obs, const float* act, int64_t B, const uint8_t* alive) const {
    MobodyEnsStep s{};
    s.dyn_blob = dyn_blob; s.dyn_planes = dyn_planes; s.mopo_blob = mopo_blob; s.mopo_blob_T = mopo_blob_T;
    s.precision = precision; s.S = S; s.A = A; s.task = task; s.obs = obs; s.act = act; s.B = B; s.alive = alive;
    s.elites = elites; s.n_elites = n_elites; s.seed = seed; s.call = call0 + (uint32_t)t; s.call_dev = call_dev;
    s.use_trg = use_trg; s.uncertainty_mode = uncertainty_mode;
    return s;
  }

  // The launches of one step on checked arguments: member forward (or the mopo MLP, the observation added in its output
  // stage) -> k_dyn_sample<MODE> -> reward head -> tail(r_mu), the launch the step ends in.
  template <class Tail>
  int launch(const MobodyEnsStep& a, const SampleBook& bk, hipStream_t st, Tail&& tail) const {
    const int64_t B = a.B;
    float* mean = a.mean_out ? a.mean_out : a.workspace;
    float* r_mu = a.workspace + (int64_t)NENS * B * S;
    int rc;
    if (mopo_blob != nullptr) {
      Mlp3FwdArgs f = fwd_net(mopo_blob, ML, B);
      fwd_set_src(f, 0, a.obs, S, S);
      fwd_set_src(f, 1, a.act, A, A);
      fwd_set_out(f, mean, 0, 1.f, a.obs, S);
      if (precision != PREC_F32) fwd_set_planes(f, mopo_blob_T, ML);
      rc = launch_mlp3_forward(f, NENS, ACT_SWISH, precision, st);
    } else {
      rc = launch_dyn_fwd(dyn_blob, L, a.obs, a.act, B, use_trg, mean, dyn_planes, precision, st);
    }
    if (rc) return rc;

    DynSampleArgs sa{};
    sa.mean = mean; sa.noise = a.noise; sa.elite_idx = a.elite_idx; sa.alive = a.alive;
    for (int k = 0; k < NENS; ++k) sa.elites[k] = (elites && k < n_elites) ? elites[k] : 0;
    sa.n_elites = n_elites; sa.seed = seed; sa.call = a.call; sa.call_dev = (const long long*)call_dev; sa.B = B; sa.S = S; sa.task = task;
    sa.next_obs = a.next_obs; sa.penalty = a.penalty; sa.terminal = a.terminal;
    sa.keep = bk.keep; sa.alive_out = bk.alive_out; sa.env_filter = bk.env_filter; sa.use_filter = bk.use_filter;
    const int rpb = 256 / S < 64 ? 256 / S : 64;         // whole rows per workgroup (the layout's 2S + A <= 256 holds S <= 127)
    const dim3 grid((unsigned)cdiv(B, rpb));
    if (uncertainty_mode == MOBODY_UNC_ALEATORIC) hipLaunchKernelGGL(k_dyn_sample<MOBODY_UNC_ALEATORIC>, grid, dim3(256), 0, st, sa, rpb);
    else if (uncertainty_mode == MOBODY_UNC_ENS_STD) hipLaunchKernelGGL(k_dyn_sample<MOBODY_UNC_ENS_STD>, grid, dim3(256), 0, st, sa, rpb);
    else hipLaunchKernelGGL(k_dyn_sample<MOBODY_UNC_PAIRWISE>, grid, dim3(256), 0, st, sa, rpb);
    MB_LAUNCH_OK("k_dyn_sample");

    // reward head on [s, a, s'] shared by the 7 members  (mobody_dynamics.py:235)
    Mlp3FwdArgs m = fwd_reward_head(dyn_blob, L, precision != PREC_F32 ? dyn_planes : nullptr, B);
    fwd_set_src(m, 0, a.obs, S, S);
    fwd_set_src(m, 1, a.act, A, A);
    fwd_set_src(m, 2, a.next_obs, S, S);
    fwd_set_out(m, r_mu, 0, 1.f);
    rc = launch_mlp3_forward(m, NENS, ACT_SWISH, precision, st);
    return rc ? rc : tail(r_mu);
  }
};

// the single step's and the rollout's tail: reward = the members' mean reward, less the penalty when the step asks for it
static int launch_finalize(const float* r_mu, const MobodyEnsStep& a, hipStream_t st) {
  DynFinalArgs fa{r_mu, a.penalty, a.reward, a.raw_reward, a.B, (a.penalty_coef != 0.f && a.use_penalty) ? a.penalty_coef : 0.f};
  hipLaunchKernelGGL(k_dyn_finalize, dim3((unsigned)cdiv(a.B, 256)), dim3(256), 0, st, fa);
  MB_LAUNCH_OK("k_dyn_finalize");
  return 0;
}

// mobody_ens_step and its two positional forms, which differ in `who` alone
static int ens_step(const char* who, const MobodyEnsStep& a, void* stream) {
  EnsModel m = EnsModel::of(a, a.call);
  int rc = mobody_dyn_layout(a.S, a.A, &m.L);         // the single step refuses a bad (S, A) for an empty batch too
  if (rc) return rc;
  rc = m.check_batch(who, a.B);
  if (rc || a.B == 0) return rc;                      // empty batch: nothing to do (pointers may be null)
  rc = m.check(who, a.elite_idx == nullptr);
  if (rc) return rc;
  MB_NONNULL(who, a, obs); MB_NONNULL(who, a, act); MB_NONNULL(who, a, next_obs); MB_NONNULL(who, a, reward);
  MB_NONNULL(who, a, terminal); MB_NONNULL(who, a, penalty); MB_NONNULL(who, a, workspace);
  hipStream_t st = as_stream(stream);
  return m.launch(a, SampleBook{}, st, [&](const float* r_mu) { return launch_finalize(r_mu, a, st); });
}

// a = pi(s) of the rollout and of the evaluation: the actor's arguments checked, then its forward
struct Policy {
  const float *blob, *blob_T;
  float max_action;
  MobodyMlpLayout La;
  int head = 0;                       // 0: the actor (S, A, 1); 1: the Gaussian policy (S, 2 A, 1), `act` of launch() is [B][2 A]
  const char* name = "actor";         // the block's field names in the refusals: <name>_blob, <name>_blob_T

  int check(const char* who, const EnsModel& m) {
    MB_REQUIRE(blob, "%s: null pointer %s_blob", who, name);
    MB_REQUIRE(m.precision == PREC_F32 || blob_T, "%s: the split-precision modes need the %s's T blob (%s_blob_T)", who, name, name);
    return mobody_mlp_layout(m.S, head == 1 ? 2 * m.A : m.A, 1, &La);
  }
  int launch(const float* obs, float* act, int64_t B, int precision, hipStream_t st) const {
    Mlp3FwdArgs p = fwd_net(blob, La, B);
    fwd_set_src(p, 0, obs, La.in_dim, La.in_dim);
    fwd_set_out(p, act, 1, max_action);
    if (precision != PREC_F32) fwd_set_planes(p, blob_T, La);
    return launch_mlp3_forward(p, 1, ACT_RELU, precision, st);
  }
};

}  // namespace mobody

extern "C" int64_t mobody_dyn_step_workspace(int S, int A, int64_t B) {
  (void)A;
  return dyn_step_floats(S, B);
}

extern "C" int mobody_ens_step(const MobodyEnsStep* a, void* stream) {
  MB_BLOCK("mobody_ens_step", a, MobodyEnsStep);
  return ens_step("mobody_ens_step", *a, stream);
}

extern "C" int mobody_dyn_step(const float* dyn_blob, const float* dyn_planes, int precision, int S, int A, int task,
                               const float* obs, const float* act,
                               int64_t B, const float* noise, const int32_t* elite_idx, const uint8_t* alive,
                               const int32_t* elites, int n_elites, uint32_t seed, uint32_t call, const int64_t* call_dev,
                               float penalty_coef, int use_penalty,
                               int use_trg, float* next_obs, float* reward, uint8_t* terminal, float* penalty,
                               float* raw_reward, float* mean_out, float* workspace, void* stream) {
  const EnsModel m{dyn_blob, dyn_planes, nullptr, nullptr, precision, S, A, task, elites, n_elites, seed, call, call_dev, use_trg,
                   MOBODY_UNC_PAIRWISE};
  MobodyEnsStep a = m.step(0, obs, act, B, alive);
  a.noise = noise; a.elite_idx = elite_idx; a.penalty_coef = penalty_coef; a.use_penalty = use_penalty;
  a.next_obs = next_obs; a.reward = reward; a.terminal = terminal; a.penalty = penalty; a.raw_reward = raw_reward;
  a.mean_out = mean_out; a.workspace = workspace;
  return ens_step("mobody_dyn_step", a, stream);
}

extern "C" int mobody_mopo_step(const float* dyn_blob, const float* dyn_planes, const float* mopo_blob, const float* mopo_blob_T,
                                int precision, int S, int A, int task, const float* obs, const float* act, int64_t B,
                                const float* noise, const int32_t* elite_idx, const uint8_t* alive, const int32_t* elites,
                                int n_elites, uint32_t seed, uint32_t call, float penalty_coef, int use_penalty, float* next_obs,
                                float* reward, uint8_t* terminal, float* penalty, float* raw_reward, float* mean_out,
                                float* workspace, void* stream) {
  MB_REQUIRE(B == 0 || mopo_blob != nullptr, "mobody_mopo_step: null MLP blob");
  const EnsModel m{dyn_blob, dyn_planes, mopo_blob, mopo_blob_T, precision, S, A, task, elites, n_elites, seed, call, nullptr, 1,
                   MOBODY_UNC_PAIRWISE};
  MobodyEnsStep a = m.step(0, obs, act, B, alive);
  a.noise = noise; a.elite_idx = elite_idx; a.penalty_coef = penalty_coef; a.use_penalty = use_penalty;
  a.next_obs = next_obs; a.reward = reward; a.terminal = terminal; a.penalty = penalty; a.raw_reward = raw_reward;
  a.mean_out = mean_out; a.workspace = workspace;
  return ens_step("mobody_mopo_step", a, stream);
}

// ---- whole H-step imagined rollout on the device (MOBODY.rollout + add_batch, mobody.py:596-657, utils.py:43-92) ----
namespace mobody {
struct RolloutWs {
  float *obs[2], *act, *reward, *penalty, *dyn;
  uint8_t *terminal, *keep, *alive;
  int32_t* scan;
  long long total;
};
static void rollout_carve(int S, int A, long long B, float* base, RolloutWs& w) {
  Carver take{base};
  w.obs[0] = take(B * S); w.obs[1] = take(B * S); w.act = take(B * A); w.reward = take(B); w.penalty = take(B);
  w.dyn = take(dyn_step_floats(S, B));
  w.terminal = (uint8_t*)take((B + 3) / 4); w.keep = (uint8_t*)take((B + 3) / 4); w.alive = (uint8_t*)take((B + 3) / 4);
  w.scan = (int32_t*)take(B + 1040);
  w.total = take.off;
}
}  // namespace mobody

extern "C" int64_t mobody_rollout_workspace(int S, int A, int64_t B) {
  RolloutWs w;
  rollout_carve(S, A, B, nullptr, w);
  return w.total;
}

// H steps of policy forward -> ensemble step (latent or mopo means) -> two-launch append: 7 launches per step for both models
static int rollout_impl(const char* who, const MobodyEnsRollout& a, void* stream) {
  const int S = a.S, A = a.A;
  const int64_t B = a.B;
  EnsModel m = EnsModel::of(a, a.call0);
  int rc = m.check_batch(who, B);
  if (rc) return rc;
  MB_REQUIRE(a.H >= 0, "%s: H < 0", who);
  if (B == 0 || a.H == 0) return 0;
  MB_REQUIRE(B <= a.cap, "%s: %lld rows per step overflow the ring of %lld twice (B > cap)", who, (long long)B, (long long)a.cap);
  rc = m.check(who);
  if (rc) return rc;
  Policy pi{a.actor_blob, a.actor_blob_T, a.max_action};
  rc = pi.check(who, m);
  if (rc) return rc;
  MB_NONNULL(who, a, init_obs); MB_NONNULL(who, a, ring); MB_NONNULL(who, a, ring->state); MB_NONNULL(who, a, ring->action);
  MB_NONNULL(who, a, ring->next_state); MB_NONNULL(who, a, ring->reward); MB_NONNULL(who, a, ring->not_done);
  MB_NONNULL(who, a, ptr_size); MB_NONNULL(who, a, workspace);
  RolloutWs w;
  rollout_carve(S, A, B, a.workspace, w);
  hipStream_t st = as_stream(stream);
  // the appends' arrival ticket (first words of the scan region) has to start at zero; every append leaves it at zero
  if (hipMemsetAsync(w.scan, 0, 8 * sizeof(int32_t), st) != hipSuccess) return fail(MOBODY_E_LAUNCH, "%s: memset failed", who);
  // rows that terminated earlier keep their index and are flagged (alive mask); the penalty filter and the alive update
  // are formed in the sample kernel
  const SampleBook bk{w.keep, w.alive, a.env_filter, a.filter_bad_rollout};
  const float* obs = a.init_obs;
  for (int t = 0; t < a.H; ++t) {
    float* nxt = w.obs[t & 1];
    rc = pi.launch(obs, w.act, B, m.precision, st);                  // a = pi(s)  (select_action, mobody.py:612)
    if (rc) return rc;
    MobodyEnsStep s = m.step(t, obs, w.act, B, t == 0 ? nullptr : w.alive);
    s.penalty_coef = a.penalty_coef; s.use_penalty = a.use_penalty;
    s.next_obs = nxt; s.reward = w.reward; s.terminal = w.terminal; s.penalty = w.penalty; s.workspace = w.dyn;
    rc = m.launch(s, bk, st, [&](const float* r_mu) { return launch_finalize(r_mu, s, st); });
    if (rc) return rc;
    rc = launch_ring_append(*a.ring, a.cap, (long long*)a.ptr_size, S, A, obs, w.act, nxt,
                            w.reward, w.terminal, w.keep, B, w.scan, st);
    if (rc) return rc;
    obs = nxt;
  }
  return 0;
}

extern "C" int64_t mobody_ens_rollout_workspace(const MobodyEnsRollout* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyEnsRollout) || a->B < 0)
    return fail(MOBODY_E_ARG, "mobody_ens_rollout_workspace: null struct, wrong struct_bytes or B < 0");
  return mobody_rollout_workspace(a->S, a->A, a->B);
}

extern "C" int mobody_ens_rollout(const MobodyEnsRollout* a, void* stream) {
  MB_BLOCK("mobody_ens_rollout", a, MobodyEnsRollout);
  return rollout_impl("mobody_ens_rollout", *a, stream);
}

// ---- the policy's return in the model (eval_policy_batch's accounting, train_mobody.py:60-98, over the learned step) ----
namespace mobody {
struct EvalWs {
  float *act, *next_obs, *penalty, *dyn, *act2;
  uint8_t *terminal, *alive_next;
  long long total;
};
// head 1 appends the Gaussian policy's [B][2 A] output: the pieces of head 0 keep their places
static void eval_carve(int S, int A, long long B, int head, float* base, EvalWs& w) {
  Carver take{base};
  w.act = take(B * A); w.next_obs = take(B * S); w.penalty = take(B);
  w.dyn = take(dyn_step_floats(S, B));
  w.terminal = (uint8_t*)take((B + 3) / 4); w.alive_next = (uint8_t*)take((B + 3) / 4);
  w.act2 = head == 1 ? take(B * 2 * A) : nullptr;
  w.total = take.off;
}
}  // namespace mobody

extern "C" int64_t mobody_ens_evaluate_workspace(const MobodyEnsEval* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyEnsEval) || a->B < 0 || a->S < 1 || a->A < 1)
    return fail(MOBODY_E_ARG, "mobody_ens_evaluate_workspace: null struct, wrong struct_bytes, B < 0 or S, A < 1");
  EvalWs w;
  eval_carve(a->S, a->A, a->B, 0, nullptr, w);
  return w.total;
}

// the two evaluation blocks differ in the policy's field names and in what MobodyEnsEvalPolicy adds
static MobodyEnsEvalPolicy eval_block_of(const MobodyEnsEval& a) {
  MobodyEnsEvalPolicy p{};
  p.struct_bytes = (int32_t)sizeof(MobodyEnsEvalPolicy); p.uncertainty_mode = a.uncertainty_mode;
  p.dyn_blob = a.dyn_blob; p.dyn_planes = a.dyn_planes; p.mopo_blob = a.mopo_blob; p.mopo_blob_T = a.mopo_blob_T;
  p.policy_blob = a.actor_blob; p.policy_blob_T = a.actor_blob_T;
  p.precision = a.precision; p.S = a.S; p.A = a.A; p.task = a.task; p.init_obs = a.init_obs; p.B = a.B; p.H = a.H;
  p.n_elites = a.n_elites; p.elites = a.elites; p.seed = a.seed; p.call0 = a.call0; p.call_dev = a.call_dev;
  p.max_action = a.max_action; p.discount = a.discount; p.use_trg = a.use_trg; p.resume = a.resume;
  p.obs_state = a.obs_state; p.alive = a.alive; p.ret = a.ret; p.pen_sum = a.pen_sum; p.disc = a.disc; p.length = a.length;
  p.workspace = a.workspace;
  return p;
}

// H steps of 5 launches: policy forward -> member forward -> sample (alive update into the workspace) -> reward head ->
// accounting; one launch more when the row state is initialised first.  head 1: the compaction [B][2 A] -> [B][A] after the
// policy forward (6 per step); member_mode 1: k_eval_members with the initialisation, `member` as the sample kernel's elite_idx
static int eval_impl(const char* who, const MobodyEnsEvalPolicy& a, const char* policy_name, void* stream) {
  const int S = a.S;
  const int64_t B = a.B;
  EnsModel m = EnsModel::of(a, a.call0);
  int rc = m.check_batch(who, B);
  if (rc) return rc;
  MB_REQUIRE(a.H >= 0, "%s: H < 0", who);
  MB_REQUIRE(a.resume == 0 || a.resume == 1, "%s: resume %d is neither 0 nor 1", who, a.resume);
  MB_REQUIRE(a.discount > 0.f && a.discount <= 1.f, "%s: discount %g outside (0, 1]", who, (double)a.discount);   // NaN fails both
  MB_REQUIRE(a.head == 0 || a.head == 1, "%s: head %d outside {0 (deterministic actor), 1 (Gaussian policy)}", who, a.head);
  MB_REQUIRE(a.member_mode == 0 || a.member_mode == 1, "%s: member_mode %d outside {0 (an elite per row and step), 1 (one per episode)}",
             who, a.member_mode);
  if (B == 0) return 0;
  MB_REQUIRE(a.head == 0 || 2 * a.A <= 128, "%s: A %d: the Gaussian policy's 2 A outputs must fit 128 columns (head 1)", who, a.A);
  rc = m.check(who);
  if (rc) return rc;
  Policy pi{a.policy_blob, a.policy_blob_T, a.max_action};
  pi.head = a.head; pi.name = policy_name;
  rc = pi.check(who, m);
  if (rc) return rc;
  MB_REQUIRE(a.resume == 1 || a.init_obs, "%s: null pointer init_obs (resume == 0)", who);
  MB_NONNULL(who, a, obs_state); MB_NONNULL(who, a, alive); MB_NONNULL(who, a, ret); MB_NONNULL(who, a, pen_sum);
  MB_NONNULL(who, a, disc); MB_NONNULL(who, a, length);
  MB_REQUIRE(a.member_mode == 0 || a.member, "%s: null pointer member (member_mode == 1)", who);
  MB_NONNULL(who, a, workspace);
  EvalWs w;
  eval_carve(S, a.A, B, a.head, a.workspace, w);
  hipStream_t st = as_stream(stream);
  const DynEvalHook hook{a.obs_state, a.alive, a.ret, a.pen_sum, a.disc, a.length, a.discount};
  if (a.resume == 0) {
    rc = launch_eval_init(a.init_obs, hook, B, S, st);
    if (rc) return rc;
    if (a.member_mode == 1 && (rc = launch_eval_members(a.elites, a.n_elites, B, a.member, st))) return rc;
  }
  SampleBook bk{}; bk.alive_out = w.alive_next;
  for (int t = 0; t < a.H; ++t) {
    rc = pi.launch(a.obs_state, a.head == 1 ? w.act2 : w.act, B, m.precision, st);   // a = pi(s)  (eval_policy_batch, train_mobody.py:76)
    if (rc) return rc;
    if (a.head == 1 && (rc = launch_fqe_action(w.act2, 2 * a.A, B, a.A, w.act, st))) return rc;   // tanh(mu): columns [0, A)
    MobodyEnsStep s = m.step(t, a.obs_state, w.act, B, a.alive);
    s.next_obs = w.next_obs; s.terminal = w.terminal; s.penalty = w.penalty; s.workspace = w.dyn;
    if (a.member_mode == 1) s.elite_idx = a.member;
    rc = m.launch(s, bk, st, [&](const float* r_mu) { return launch_eval_account(r_mu, w.penalty, w.next_obs, w.alive_next, hook, B, S, st); });
    if (rc) return rc;
  }
  return 0;
}

extern "C" int mobody_ens_evaluate(const MobodyEnsEval* ap, void* stream) {
  const char* who = "mobody_ens_evaluate";
  MB_BLOCK(who, ap, MobodyEnsEval);
  return eval_impl(who, eval_block_of(*ap), "actor", stream);
}

extern "C" int64_t mobody_ens_evaluate_policy_workspace(const MobodyEnsEvalPolicy* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyEnsEvalPolicy) || a->B < 0 || a->S < 1 || a->A < 1 || a->head < 0 || a->head > 1)
    return fail(MOBODY_E_ARG, "mobody_ens_evaluate_policy_workspace: null struct, wrong struct_bytes, B < 0, S, A < 1 or head outside {0, 1}");
  EvalWs w;
  eval_carve(a->S, a->A, a->B, a->head, nullptr, w);
  return w.total;
}

extern "C" int mobody_ens_evaluate_policy(const MobodyEnsEvalPolicy* ap, void* stream) {
  const char* who = "mobody_ens_evaluate_policy";
  MB_BLOCK(who, ap, MobodyEnsEvalPolicy);
  return eval_impl(who, *ap, "policy", stream);
}

// ---- open-loop error over recorded trajectories (the model fed the data's actions, compared with the data's outcomes) ----
namespace mobody {
struct ReplayWs {
  float *next_obs, *penalty, *dyn;
  uint8_t* terminal;
  long long total;
};
static void replay_carve(int S, long long B, float* base, ReplayWs& w) {
  Carver take{base};
  w.next_obs = take(B * S); w.penalty = take(B);
  w.dyn = take(dyn_step_floats(S, B));
  w.terminal = (uint8_t*)take((B + 3) / 4);
  w.total = take.off;
}
}  // namespace mobody

extern "C" int64_t mobody_ens_replay_workspace(const MobodyEnsReplay* a) {
  if (a == nullptr || a->struct_bytes != (int32_t)sizeof(MobodyEnsReplay) || a->B < 0 || a->S < 1 || a->A < 1)
    return fail(MOBODY_E_ARG, "mobody_ens_replay_workspace: null struct, wrong struct_bytes, B < 0 or S, A < 1");
  ReplayWs w;
  replay_carve(a->S, a->B, nullptr, w);
  return w.total;
}

// One launch for the row state, then H steps of 4 launches: member forward -> sample -> reward head -> accounting
extern "C" int mobody_ens_replay(const MobodyEnsReplay* ap, void* stream) {
  const char* who = "mobody_ens_replay";
  MB_BLOCK(who, ap, MobodyEnsReplay);
  const MobodyEnsReplay& a = *ap;
  const int S = a.S, A = a.A;
  const int64_t B = a.B;
  EnsModel m = EnsModel::of(a, a.call0);
  int rc = m.check_batch(who, B);
  if (rc) return rc;
  MB_REQUIRE(a.H >= 0, "%s: H < 0", who);
  MB_REQUIRE(a.reset_every >= 0, "%s: reset_every < 0", who);
  if (B == 0) return 0;
  MB_REQUIRE(a.data_rows >= 1, "%s: data_rows %lld < 1", who, (long long)a.data_rows);
  rc = m.check(who);
  if (rc) return rc;
  MB_NONNULL(who, a, data); MB_NONNULL(who, a, data->state); MB_NONNULL(who, a, data->action); MB_NONNULL(who, a, data->next_state);
  MB_NONNULL(who, a, data->reward); MB_NONNULL(who, a, row0); MB_NONNULL(who, a, obs_state); MB_NONNULL(who, a, act_state);
  if (a.H > 0) {                                       // the four tables are written by the steps alone
    MB_NONNULL(who, a, obs_err); MB_NONNULL(who, a, rew_err); MB_NONNULL(who, a, penalty); MB_NONNULL(who, a, term_model);
  }
  MB_NONNULL(who, a, workspace);
  MB_REQUIRE(a.data->pitch == 0 || a.data->pitch >= 2LL * S + A + 2, "%s: data->pitch %lld is neither 0 nor at least 2S + A + 2 = %d", who,
             (long long)a.data->pitch, 2 * S + A + 2);
  ReplayWs w;
  replay_carve(S, B, a.workspace, w);
  hipStream_t st = as_stream(stream);
  DynReplayHook hook{a.data, a.data_rows, (const long long*)a.row0, a.obs_state, a.act_state, nullptr, nullptr, nullptr, nullptr, 0, 0};
  rc = launch_replay_init(hook, B, S, A, st);
  if (rc) return rc;
  for (int t = 0; t < a.H; ++t) {
    MobodyEnsStep s = m.step(t, a.obs_state, a.act_state, B, nullptr);
    s.next_obs = w.next_obs; s.terminal = w.terminal; s.penalty = w.penalty; s.workspace = w.dyn;
    hook.obs_err = a.obs_err + (int64_t)t * B; hook.rew_err = a.rew_err + (int64_t)t * B; hook.penalty = a.penalty + (int64_t)t * B;
    hook.term_model = a.term_model + (int64_t)t * B;
    hook.t = t; hook.reset = a.reset_every > 0 && (t + 1) % a.reset_every == 0;
    rc = m.launch(s, SampleBook{}, st, [&](const float* r_mu) { return launch_replay_account(r_mu, w.penalty, w.next_obs, w.terminal, hook, B, S, A, st); });
    if (rc) return rc;
  }
  return 0;
}

extern "C" int mobody_rollout(const float* dyn_blob, const float* dyn_planes, const float* actor_blob, const float* actor_blob_T,
                              int precision, int S, int A, int task, float max_action,
                              const float* init_obs, int64_t B, int H, const int32_t* elites, int n_elites, uint32_t seed,
                              uint32_t call0, float penalty_coef, int use_penalty, int use_trg, float env_filter,
                              int filter_bad_rollout, const MobodyBufferView* ring, int64_t cap, int64_t* ptr_size, float* workspace,
                              void* stream) {
  MobodyEnsRollout a{};
  a.dyn_blob = dyn_blob; a.dyn_planes = dyn_planes; a.actor_blob = actor_blob; a.actor_blob_T = actor_blob_T;
  a.precision = precision; a.S = S; a.A = A; a.task = task; a.max_action = max_action; a.init_obs = init_obs; a.B = B; a.H = H;
  a.elites = elites; a.n_elites = n_elites; a.seed = seed; a.call0 = call0; a.penalty_coef = penalty_coef;
  a.use_penalty = use_penalty; a.use_trg = use_trg; a.uncertainty_mode = MOBODY_UNC_PAIRWISE; a.env_filter = env_filter;
  a.filter_bad_rollout = filter_bad_rollout; a.ring = ring; a.cap = cap; a.ptr_size = ptr_size; a.workspace = workspace;
  return rollout_impl("mobody_rollout", a, stream);
}

// ---- stand-alone predicate / rollout bookkeeping -------------------------------------------------
namespace mobody {
__global__ __launch_bounds__(256) void k_termination(int task, const float* next_obs, long long B, int S, uint8_t* done) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) done[b] = term_predicate(task, next_obs + b * S, S) ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_rollout_mask(const uint8_t* alive_in, const uint8_t* terminal, const float* penalty,
                                                      float env_filter, int use_filter, long long B, uint8_t* keep,
                                                      uint8_t* alive_out) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool alive = alive_in ? alive_in[b] != 0 : true;
  if (keep) keep[b] = (alive && (!use_filter || penalty[b] <= env_filter)) ? 1 : 0;     // mobody.py:648-653
  if (alive_out) alive_out[b] = (alive && !terminal[b]) ? 1 : 0;                         // :635-639
}
}  // namespace mobody

extern "C" int mobody_termination(int task, const float* next_obs, int64_t B, int S, uint8_t* done, void* stream) {
  MB_REQUIRE(B >= 0 && S >= 1, "mobody_termination: bad sizes");
  if (B == 0) return 0;
  MB_REQUIRE(next_obs && done, "mobody_termination: null pointer");
  MB_REQUIRE(task >= MOBODY_TERM_NEVER && task <= MOBODY_TERM_PEN, "mobody_termination: unknown termination id %d", task);
  MB_REQUIRE(task != MOBODY_TERM_PEN || S > 26, "mobody_termination: pen predicate needs S > 26");
  MB_REQUIRE(S >= 2 || task == MOBODY_TERM_NEVER || task == MOBODY_TERM_HALFCHEETAH || task == MOBODY_TERM_ANT || task == MOBODY_TERM_HUMANOID,
             "mobody_termination: predicate needs S >= 2");
  hipLaunchKernelGGL(k_termination, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, as_stream(stream), task, next_obs, (long long)B, S, done);
  MB_LAUNCH_OK("k_termination");
  return 0;
}

extern "C" int mobody_rollout_mask(const uint8_t* alive_in, const uint8_t* terminal, const float* penalty, float env_filter,
                                   int use_filter, int64_t B, uint8_t* keep, uint8_t* alive_out, void* stream) {
  MB_REQUIRE(B >= 0, "mobody_rollout_mask: B < 0");
  if (B == 0) return 0;
  MB_REQUIRE(terminal && penalty, "mobody_rollout_mask: null pointer");
  hipLaunchKernelGGL(k_rollout_mask, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, as_stream(stream), alive_in, terminal, penalty,
                     env_filter, use_filter, (long long)B, keep, alive_out);
  MB_LAUNCH_OK("k_rollout_mask");
  return 0;
}
