// The tile body of the fused MLP backward (mlp3_bwd_tile) with its masked epilogues and seed prologues, shared by its two translation
// units: mlp_bwd.hip (k_mlp3_bwd, k_actor_bwd_chain) and critic_fwd_bf.hip (the critic backward chained onto the merged critic forward).
#pragma once
#include "common.h"
#include "dara.h"
#include "layers_bf.h"
#include "train.h"

namespace mobody {

// Masked epilogue of a backward wide layer, in two parts around the barrier that separates the GEMM's LDS reads from the
// epilogue's LDS writes.
//
// wide_mask_apply (before the barrier, registers only): acc <- dz = (acc * prescale) * [h > 0].  The mask values of a lane
// are fetched with UNCONDITIONAL loads from clamped rows -- a `cond ? load : 0` select makes hipcc branch around every
// load and drain vmcnt(0) after it (64 serialized HBM round trips per layer, measured 60 % SQ_WAIT_ANY) -- so all of them
// are in flight together and cost one round trip.  Returns the lane's largest |dz| (the f16 mode's tile scale).
// MASK: 0 = ReLU mask from the saved activations (h > 0), 1 = ReLU mask from the forward's sign words,
//       2 = Swish: multiply by the saved derivative d = dy/dz (h points at save_d of the forward, mobody_module.py:9-15).
// The mask operand of one layer for this lane: two sign words per 32-row tile (MASK == 1) or the 32 saved values per tile
// (MASK 0: activations, 2: Swish derivatives).  It is requested BEFORE the GEMM whose epilogue consumes it (mask_fetch):
// fetched inside the epilogue it put one L2 / HBM round trip (~1 us) between each GEMM and its epilogue in every workgroup of
// the launch at the same moment (phase trace of a lone workgroup: mask epilogue 2.5 us of a 10.9 us backward).  All loads are
// UNCONDITIONAL from clamped rows (see above).  CH: the sign words were published inside this launch (agent-scope loads).
template <int MT, int MASK>
struct MaskPre {
  uint32_t w[MASK == 1 ? MT : 1][2];
  float v[MASK == 1 ? 1 : MT][2][MASK == 1 ? 1 : 16];
};
template <int MT, int MASK, bool CH = false>
__device__ __forceinline__ void mask_fetch(MaskPre<MT, MASK>& p, const float* __restrict__ h, const uint32_t* __restrict__ bits,
                                           int rows_here) {
  const int lane = lane_id(), w = wave_id(), i = lane & 31, hh = lane >> 5;
  if constexpr (MASK == 1) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int g = min(mt, (rows_here + 31) / 32 - 1);      // groups past the end of the batch have no words (their rows are masked)
      if constexpr (CH) { p.w[mt][0] = agent_load(bits + g * HID + 64 * w + i); p.w[mt][1] = agent_load(bits + g * HID + 64 * w + 32 + i); }
      else { p.w[mt][0] = bits[g * HID + 64 * w + i]; p.w[mt][1] = bits[g * HID + 64 * w + 32 + i]; }
    }
  } else {
    const float* hp = h + 64 * w + i;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = min(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh, rows_here - 1);
        p.v[mt][0][r] = hp[row * HID];
        p.v[mt][1][r] = hp[row * HID + 32];
      }
  }
}

template <int MT, int MASK>
__device__ __forceinline__ float wide_mask_apply(f32x16 (&acc)[MT][2], const MaskPre<MT, MASK>& pre, int rows_here, float prescale) {
  const int hh = lane_id() >> 5;
  constexpr bool BITS = MASK == 1;
  const auto& hv = pre.v;
  const auto& mw = pre.w;
  float mx = 0.f;
  f32x16 pa[MT][2];                                  // acc * prescale as whole vectors (v_pk_mul_f32)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) { pa[mt][0] = acc[mt][0] * prescale; pa[mt][1] = acc[mt][1] * prescale; }
  // full tile (wave uniform): no per-element row guard
  auto sweep = [&](auto guarded) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rb = (r & 3) + 8 * (r >> 2) + 4 * hh;
          const bool valid = !decltype(guarded)::value || 32 * mt + rb < rows_here;
          const float a = pa[mt][nt][r];
          float dz;
          if constexpr (MASK == 2) {
            dz = valid ? a * hv[mt][nt][r] : 0.f;
          } else {
            bool on;
            if constexpr (BITS) on = (mw[mt][nt] >> rb) & 1u;
            else on = hv[mt][nt][r] > 0.f;
            dz = (on && valid) ? a : 0.f;
          }
          acc[mt][nt][r] = dz;
          mx = fmaxf(mx, fabsf(dz));
        }
  };
  if (rows_here == 32 * MT) sweep(std::false_type{});
  else sweep(std::true_type{});
  return finite_tile_max<MT>(acc, mx);
}

// wide_store_colsum (after the barrier): dz -> LDS (the fp32 image, or -- PM > 0 -- the 16-bit planes the next GEMM
// contracts on the split-precision core, scaled by 2^e in the f16 mode), optional global copy (the weight-gradient operand,
// always fp32) and the per-column sums of the tile (bias gradient).  Lanes < 32 end up with the sums of columns
// 64w + 32nt + (lane&31), nt = 0,1.
template <int MT, int PM>
__device__ __forceinline__ void wide_store_colsum(f32x16 (&acc)[MT][2], float* Xs, float* gdst, int rows_here, int e,
                                                  float (&cs)[2], const PlaneSave& gs = PlaneSave{nullptr, 0, nullptr}) {
  const int lane = lane_id(), w = wave_id();
  const int i = lane & 31, hh = lane >> 5;
  cs[0] = cs[1] = 0.f;
  if constexpr (PM > 0) {
    const float sc = Split<PM>::F16 ? exp2i(e) : 1.f;
    if (gs.base != nullptr && (int)threadIdx.x < MT) gs.e_out[threadIdx.x] = e;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const f32x16 ys = Split<PM>::F16 ? acc[mt][nt] * sc : acc[mt][nt];               // v_pk_mul_f32
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float y4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) y4[j] = ys[4 * g + j];
          planes_store4<PM, 32 * MT>(reinterpret_cast<char*>(Xs), 64 * w + 32 * nt + i, 8 * mt + 2 * g + hh, y4, gs.base, gs.plane_stride);
        }
      }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float dz = acc[mt][nt][r];
        if constexpr (PM == 0) Xs[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh) * LDX + 64 * w + 32 * nt + i] = dz;
        cs[nt] += dz;
      }
  if (gdst != nullptr) wide_store_rows<MT>(acc, gdst, rows_here);
  cs[0] += __shfl_xor(cs[0], 32);
  cs[1] += __shfl_xor(cs[1], 32);
}

// Seed prologue (BwdSeed modes 1-4).  SEED is the seed form of the tile: SEED_RT = k_mlp3_bwd, whose launch carries mode 0 (dz3
// from memory, no prologue) or mode 1 and chooses at run time; 2 or 4 and 3 = the two tiles of k_actor_bwd_chain, known at compile
// time.  Modes 1, 2 and 4 (one-output nets) leave the TB seed values of column 0 in Xs[0..TB) -- the kernel forms the rank-1
// product dz3 W3^T from them -- with one thread per row (1, 2) or eight (4, which also sums the row's (pi - a)^2); modes 2 and 4
// return there, they have no loss partials.  Mode 3 fills Xs[r][0..Np3).  All global loads of a pass are independent (one round
// trip); the loss partials are reduced through `red` (static LDS, 8 floats).  `tile` is the row tile (row0 / TB).  Mode 2's / 4's
// bcw (and dx) are handed to the mode-3 tile of the same rows within the launch: they store them write-through (agent scope), mode 3
// loads them at agent scope -- past its CU's L1 -- and a row's loads stay on words its own tile has published.
// SEED_CRITIC_CHAIN: mode 1 as the tile chained onto the merged critic forward runs it (critic_fwd_bf.hip): q, qt, reward and not_done
// of its rows were published by other workgroups of the same launch, so every load of them -- and of the sign words, mask_fetch --
// is an agent-scope load; the expressions are SEED_RT's mode 1 without qnext.
constexpr int SEED_RT = -1;
constexpr int SEED_CRITIC_CHAIN = 10;
template <int SEED>
__device__ __forceinline__ void bwd_seed(const Mlp3BwdArgs& a, float* Xs, float* red, int m, int tile, long long row0,
                                         int rows_here, int TB) {
  const BwdSeed& sd = a.seed;
  const int Np3 = a.Np3;
  const int t = threadIdx.x;
  float l0 = 0.f, l1 = 0.f;
  if constexpr (SEED == 5) {                          // mode 5: one thread per row, all in wave 0 (TB <= 64)
    static_assert(MLP_TILE_ROWS <= 64, "mode 5 reduces its three partial sums inside wave 0");
    const IqlSeed& q = sd.iq;
    if (t < 64) {
      const bool ok = t < rows_here;
      const long long row = row0 + (ok ? t : 0);
      const float q0 = q.qt[row], q1 = q.qt[a.rows + row], vv = q.v[row];
      const float adv = fminf(q0, q1) - vv;
      const float w = fabsf(q.lam - (adv < 0.f ? 1.f : 0.f));
      const float v = ok ? -2.f * w * adv * q.inv : 0.f;
      float s0 = ok ? w * adv * adv : 0.f, s1 = ok ? adv : 0.f, s2 = ok ? vv : 0.f;
      if (t < TB) Xs[t] = v;
      if (ok) {
        q.adv_out[row] = adv;
        float* g = sd.dz3_out + row * Np3;
        g[0] = v;
        for (int c = 1; c < Np3; ++c) g[c] = 0.f;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
      if (t == 0) {
        const long long T = cdiv(a.rows, (long long)TB);
        sd.lossp[tile] = s0; sd.lossp[T + tile] = s1; sd.lossp[2 * T + tile] = s2;
      }
    }
    return;
  } else if constexpr (SEED == 6) {                   // mode 6: one thread per (row, column)
    const IqlSeed& q = sd.iq;
    if (tile == 0 && t == 0 && q.bc_out != nullptr) { // the policy's Adam constants at this step's cosine learning rate
      const long long k = q.t_dev[0];
      const double kd = (double)k;
      q.bc_out[0] = (float)((double)cosine_lr(q.lr0, k, q.T_max) / (1.0 - pow(0.9, kd)));
      q.bc_out[1] = (float)sqrt(1.0 - pow(0.999, kd));
    }
    for (int e = t; e < TB * Np3; e += NTHREADS) {
      const int rr = e / Np3, j = e - rr * Np3;
      const bool ok = rr < rows_here && j < q.A;
      const long long row = row0 + (rr < rows_here ? rr : 0);
      const int jc = j < q.A ? j : 0;
      const float z = q.z[row * q.ldz + jc], av = q.act[row * q.A + jc], adv = q.adv[row];   // unconditional, clamped
      float v = 0.f;                                  // columns >= A (logstd, padding) and rows past the batch: exactly 0
      if (ok) {
        const float w = fminf(expf(q.temp * adv), 100.f);      // e may be inf: the clamp comes first, nothing multiplies e
        const float th = tanhf(z), df = th - av;
        v = 2.f * w * df * (1.f - th * th) * q.inv;
        l0 += w * (df * df);
      }
      Xs[rr * LDX + j] = v;
      if (rr < rows_here) sd.dz3_out[(row0 + rr) * Np3 + j] = v;
    }
  } else if constexpr (SEED == 7) {                   // mode 7: one thread per row fills the row's Np3 columns
    const DaraSeed& q = sd.da;
    if (t < TB) {
      const bool ok = t < rows_here;
      const long long row = row0 + (ok ? t : 0);
      const float z0 = q.z[row * q.ldz], z1 = q.z[row * q.ldz + 1];               // unconditional, clamped
      float d0, d1;
      const float l = ce_on_probs(z0, z1, row < q.n_src ? 0 : 1, q.inv, d0, d1);
      if (!ok) d0 = d1 = 0.f;                         // rows past the batch: exactly 0
      l0 = ok ? l : 0.f;
      float* xr = Xs + t * LDX;
      xr[0] = d0; xr[1] = d1;
      for (int c = 2; c < Np3; ++c) xr[c] = 0.f;
      if (ok) {
        float* g = sd.dz3_out + row * Np3;
        g[0] = d0; g[1] = d1;
        for (int c = 2; c < Np3; ++c) g[c] = 0.f;
      }
    }
  } else if constexpr (SEED == 8) {                   // mode 8: mode 1 with a row weight, one thread per row
    if (t < TB) {
      const bool ok = t < rows_here;
      const long long row = row0 + (ok ? t : 0);
      const float qn = sd.qnext ? sd.qnext[row] : fminf(sd.qt[row], sd.qt[a.rows + row]);
      const float y = sd.r[row] + sd.nd[row] * sd.gamma * qn;
      const float d = sd.q[(long long)m * a.rows + row] - y;
      const float wr = sd.cw.w[row];
      const float v = ok ? 2.f * wr * d * sd.inv_ng : 0.f;
      l0 = ok ? wr * (d * d) : 0.f;
      if (ok) {
        float* g = sd.dz3_out + ((long long)m * a.rows + row) * Np3;
        g[0] = v;
        for (int c = 1; c < Np3; ++c) g[c] = 0.f;
      }
      Xs[t] = v;
    }
  } else if constexpr (SEED == 9) {                   // mode 9: mode 8 plus a per-row constant, one thread per row
    if (t < TB) {
      const bool ok = t < rows_here;
      const long long row = row0 + (ok ? t : 0);
      const float qn = sd.qnext ? sd.qnext[row] : fminf(sd.qt[row], sd.qt[a.rows + row]);
      const float y = sd.r[row] + sd.nd[row] * sd.gamma * qn;
      const float qm = sd.q[(long long)m * a.rows + row];
      const float d = qm - y;
      const float wr = sd.cs.w[row], cr = sd.cs.c[row];
      const float td = 2.f * wr * d * sd.inv_ng;
      const float v = ok ? (cr != 0.f ? td + cr : td) : 0.f;       // c == 0: mode 8's value, the sign of a zero included
      l0 = ok ? wr * (d * d) : 0.f;
      l1 = ok && cr != 0.f ? qm : 0.f;
      if (ok) {
        float* g = sd.dz3_out + ((long long)m * a.rows + row) * Np3;
        g[0] = v;
        for (int c = 1; c < Np3; ++c) g[c] = 0.f;
      }
      Xs[t] = v;
    }
  } else if constexpr (SEED == 4) {                   // mode 4: eight threads per row (TB * 8 == NTHREADS)
    static_assert(MLP_TILE_ROWS * 8 == NTHREADS, "mode 4 spreads a row's A <= 24 action columns over eight lanes");
    // sq = sum_j (pi - a)^2 needs A words of pi and of act per row: lane `sub` of a row's eight takes columns sub, sub + 8,
    // sub + 16 (A <= 24, checked by the launcher), all requested beside q0, q1 and stats[0] -- one round trip -- and the eight
    // partial sums meet in three shuffles.  (pi is the policy forward's output of an earlier launch: plain loads.)
    const ActorRowArgs& r = sd.ar;
    const int rr = t >> 3, sub = t & 7;
    const bool ok = rr < rows_here;
    const long long row = row0 + (ok ? rr : 0);
    const float *pp = r.pi + row * r.A, *ap = r.act + row * r.A;
    float pv[3], av[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) { const int j = sub + 8 * u, jc = j < r.A ? j : 0; pv[u] = pp[jc]; av[u] = ap[jc]; }
    const float q0 = r.qp[row], q1 = r.qp[r.N + row];
    const float c = -policy_weight(r) / (float)r.Ng;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < 3; ++u) if (sub + 8 * u < r.A) { const float df = pv[u] - av[u]; sq += df * df; }
    sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4);
    float dq = c, w = 1.f;
    if (r.h.q_weighted) {                             // w = min(exp(k q / m), 100) with its gradient through q (td3_bc.py:166-170)
      const float mean = r.stats[0] / (float)r.Ng;
      const float e = expf(sd.exp_scale * (fminf(q0, q1) / mean));
      w = fminf(e, 100.f);
      const float gw = r.h.bc_coef * (sd.exp_scale * e / mean) * sq / ((float)r.Ng * (float)r.A);
      dq = e <= 100.f ? c + gw : c;                   // a select: above the clamp e may be inf, and inf * 0 would seed a NaN
    }
    if (sub == 0) {
      const float g0 = q0 < q1 ? 1.f : (q0 == q1 ? 0.5f : 0.f);
      Xs[rr] = ok ? dq * (m == 0 ? g0 : 1.f - g0) : 0.f;
      if (m == 0 && ok) agent_store(r.bcw + row, w);  // every row is a BC row (Nt == N)
    }
    return;                                           // no loss partials
  } else if constexpr (SEED != 3) {                   // modes 1 and 2: one thread per row
    if (t < TB) {
      const bool ok = t < rows_here;
      const long long row = row0 + (ok ? t : 0);
      float v = 0.f;
      if constexpr (SEED == SEED_CRITIC_CHAIN) {                      // (no qnext: the launch evaluated target-Q itself)
        const float qn = fminf(agent_load(sd.qt + row), agent_load(sd.qt + a.rows + row));
        const float y = agent_load(sd.r + row) + agent_load(sd.nd + row) * sd.gamma * qn;
        const float d = agent_load(sd.q + (long long)m * a.rows + row) - y;
        v = ok ? 2.f * d * sd.inv_ng : 0.f;
        l0 = ok ? d * d : 0.f;
        if (sd.dz3_out != nullptr && ok) {
          float* g = sd.dz3_out + ((long long)m * a.rows + row) * Np3;
          g[0] = v;
          for (int c = 1; c < Np3; ++c) g[c] = 0.f;
        }
      } else if constexpr (SEED == SEED_RT) {
        const float qn = sd.qnext ? sd.qnext[row] : fminf(sd.qt[row], sd.qt[a.rows + row]);
        const float y = sd.r[row] + sd.nd[row] * sd.gamma * qn;
        const float d = sd.q[(long long)m * a.rows + row] - y;
        v = ok ? 2.f * d * sd.inv_ng : 0.f;
        l0 = ok ? d * d : 0.f;
        if (sd.dz3_out != nullptr && ok) {
          float* g = sd.dz3_out + ((long long)m * a.rows + row) * Np3;
          g[0] = v;
          for (int c = 1; c < Np3; ++c) g[c] = 0.f;
        }
      } else {
        const ActorRowArgs& r = sd.ar;
        const float q0 = r.qp[row], q1 = r.qp[r.N + row];
        const float c = -policy_weight(r) / (float)r.Ng;
        const float g0 = q0 < q1 ? 1.f : (q0 == q1 ? 0.5f : 0.f);
        v = ok ? c * (m == 0 ? g0 : 1.f - g0) : 0.f;
        if (m == 0 && ok && row < r.Nt) agent_store(r.bcw + row, bc_weight(r, row));
      }
      Xs[t] = v;
    }
    if constexpr (SEED == 2) return;                  // no loss partials
  } else {                                            // mode 3: one thread per (row, column)
    const ActorRowArgs& r = sd.ar;
    const float wscale = r.h.bc_coef * 2.f / ((float)r.Ntg * (float)r.A);
    // The agent-scope loads of dxa / bcw pass L1, so a thread requests the operands of ALL its elements (SEED_U passes of
    // NTHREADS elements: Np3 = 32 has four) before it uses the first: one round trip per tile, not one per pass.  The elements
    // are then formed in element order.
    constexpr int SEED_U = 4;
    for (int e0 = t; e0 < TB * Np3; e0 += SEED_U * NTHREADS) {
      float pv[SEED_U], d0v[SEED_U], d1v[SEED_U], av[SEED_U], wv[SEED_U], qv[SEED_U][2];
#pragma unroll
      for (int u = 0; u < SEED_U; ++u) {
        const int e = min(e0 + u * NTHREADS, TB * Np3 - 1);
        const int rr = e / Np3, j = e - rr * Np3;
        const long long row = row0 + (rr < rows_here ? rr : 0);
        const int jc = j < r.A ? j : 0;
        const float* dp = r.dxa + row * r.A + jc;
        pv[u] = r.pi[row * r.A + jc]; av[u] = r.act[row * r.A + jc];
        qv[u][0] = r.qp[row]; qv[u][1] = r.qp[r.N + row];
        d0v[u] = agent_load(dp); d1v[u] = agent_load(dp + r.N * r.A);
        // A non-BC row's weight is gated out below.  bcw[0] belongs to tile 0, which may not have run yet: such a row asks for its
        // own dxa word again instead, so that no word is touched before its writer has published it.  (An unconditional load
        // beside the others, same line as d0: a `bc ? load : 0` select branches around the load and waits for it.)
        wv[u] = agent_load(row < r.Nt ? r.bcw + row : dp);
      }
#pragma unroll
      for (int u = 0; u < SEED_U; ++u) {
        const int e = e0 + u * NTHREADS;
        if (e < TB * Np3) {
          const int rr = e / Np3, j = e - rr * Np3;
          const bool ok = rr < rows_here && j < r.A;
          const long long row = row0 + (rr < rows_here ? rr : 0);
          const bool bc = row < r.Nt;
          const float p = pv[u], w = wv[u];
          float v = 0.f;
          if (ok) {
            float d = d0v[u] + d1v[u];
            if (bc) { const float df = p - av[u]; d += wscale * w * df; l1 += w * (df * df); }
            const float th = p / r.h.max_action;
            v = d * r.h.max_action * (1.f - th * th);                   // d tanh
            if (j == 0) l0 = l0 - fminf(qv[u][0], qv[u][1]);
          }
          Xs[rr * LDX + j] = v;
          if (rr < rows_here) sd.dz3_out[(row0 + rr) * Np3 + j] = v;
        }
      }
    }
  }
  // loss partials of this tile
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { l0 += __shfl_xor(l0, o); l1 += __shfl_xor(l1, o); }
  if ((t & 63) == 0) { red[t >> 6] = l0; red[4 + (t >> 6)] = l1; }
  lds_barrier();                                     // (LDS only: __syncthreads would also drain the dz3_out stores, ~1 us per tile)
  if (t == 0) {
    l0 = red[0] + red[1] + red[2] + red[3];
    l1 = red[4] + red[5] + red[6] + red[7];
    if constexpr (SEED == 9) { sd.lossp[2 * (tile * 2 + m)] = l0; sd.lossp[2 * (tile * 2 + m) + 1] = l1; }
    else if constexpr (SEED == SEED_RT || SEED == SEED_CRITIC_CHAIN || SEED == 8) sd.lossp[tile * 2 + m] = l0;
    else if constexpr (SEED == 6 || SEED == 7) sd.lossp[tile] = l0;
    else { sd.lossp[2 * tile] = l0; sd.lossp[2 * tile + 1] = l1; }
  }
}

// NT (DX only): 16-column tiles of the input-gradient layer handled by the K-split narrow layer (Np1t == 16*NT),
// or 0 = any Np1t through the row-split path.
// MASK: see wide_mask_apply (1: sign words m1, m2; 0: saved activations h1, h2; 2: Swish derivatives in h1, h2).
// PM: 0 = exact fp32 MFMA; 1..4 = the 256 x 256 GEMM (dz2 W2^T) on the split-precision core, streaming W2^T's planes.
// The backward of one (32-row tile, member) of a launch of `members` members: Xs is the workgroup's dynamic LDS, red its eight
// static floats.  SEED: see bwd_seed.
template <bool DX, int NT, int MASK, int PM = 0, int SEED = SEED_RT>
__device__ __forceinline__ void mlp3_bwd_tile(const Mlp3BwdArgs& a, int m, int tile, int members, float* Xs, float* red) {
  constexpr bool BITS = MASK == 1;
  constexpr int TB = MLP_TILE_ROWS, MT = MLP_MT;
  constexpr int PMX = PM > 0 ? PM : 1;
  const long long row0 = (long long)tile * TB;
  const int rows_here = (int)min((long long)TB, a.rows - row0);
  const int lane = lane_id(), w = wave_id();
  const float* w3t = a.wt + m * a.t_mstride + a.w3t;
  const float* w2t = a.wt + m * a.t_mstride + a.w2t;
  const float* w1t = a.wt + m * a.t_mstride + a.w1t;
  const float* h1 = BITS ? nullptr : a.h1 + ((long long)m * a.rows + row0) * HID;
  const float* h2 = BITS ? nullptr : a.h2 + ((long long)m * a.rows + row0) * HID;
  const long long mtile = ((long long)m * cdiv(a.rows, 32) + row0 / 32) * HID;
  const uint32_t* m1 = BITS ? a.m1 + mtile : nullptr;
  const uint32_t* m2 = BITS ? a.m2 + mtile : nullptr;
  float* dz2 = a.dz2 ? a.dz2 + ((long long)m * a.rows + row0) * HID : nullptr;
  float* dz1 = a.dz1 ? a.dz1 + ((long long)m * a.rows + row0) * HID : nullptr;
  float* dbp = a.dbp + ((long long)tile * members + m) * (2 * HID + a.Np3);
  float* scr = reinterpret_cast<float*>(reinterpret_cast<char*>(Xs) + split_scr_offset<PMX, TB>());   // tile maximum (f16 mode)

  TR(0);
  MaskPre<MT, MASK> mk1, mk2;                       // layer 2's operand now; layer 1's too when it is two words, else before its GEMM
  constexpr bool CH = SEED == SEED_CRITIC_CHAIN;
  mask_fetch<MT, MASK, CH>(mk2, h2, m2, rows_here);
  if constexpr (BITS) mask_fetch<MT, MASK, CH>(mk1, h1, m1, rows_here);
  // (split modes: the ring only serves the K = Np3 GEMM, two to four chunks -- three stages keep the kernel at 128 registers)
  WideRingT<(PM > 0 ? 3 : WIDE_RING)> ring;
  // Seed modes 1 and 2 seed column 0 of a one-output net: dz3 W3^T is the rank-1 product seed[row] * W3^T[0][col], formed in
  // registers -- no weight ring, no K = Np3 GEMM.  (An fp32 fma chain whose only non-zero product is its first yields
  // round(v * w): the same values as the GEMM gave, up to the sign of an exact zero.)  Mode 2 also has no bias partials.
  const bool rank1 = SEED == SEED_RT ? a.seed.mode == 1 : (SEED == 2 || SEED == 4 || SEED == 5 || SEED == 8 || SEED == 9 || SEED == SEED_CRITIC_CHAIN);
  constexpr bool with_db = SEED != 2 && SEED != 4;
  const int c0 = (64 * w + (lane & 31)) * 4;        // wide_idx(0, col) of this lane's two columns: same round trip as the masks
  const float w3c[2] = {w3t[c0], w3t[c0 + 128]};
  if (!rank1) wide_prefetch(w3t, a.Np3, ring);    // weight fragments travel while the seed rows are fetched
  if (SEED == SEED_RT && !rank1) tile_load(Xs, 0, a.dz3 + ((long long)m * a.rows + row0) * a.Np3, a.Np3, a.Np3, 0, rows_here, TB);
  else bwd_seed<SEED>(a, Xs, red, m, tile, row0, rows_here, TB);
  lds_barrier();
  TR(1);
  if (with_db && (int)threadIdx.x < a.Np3) {      // db3 partial of this tile (rank-1: column 0 alone is non-zero)
    float s = 0.f;
    if (!rank1) for (int r = 0; r < TB; ++r) s += Xs[r * LDX + threadIdx.x];
    else if (threadIdx.x == 0) for (int r = 0; r < TB; ++r) s += Xs[r];
    dbp[2 * HID + threadIdx.x] = s;
  }

  f32x16 acc[MT][2];
  float cs[2];
  // dh2 = dz3 * W3^T ; dz2 = dh2 * [h2 > 0]
  if (rank1) {
    const int hh = lane >> 5;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(Xs + 32 * mt + 8 * g + 4 * hh);     // rows (r & 3) + 8 (r >> 2) + 4 hh, r = 4 g + j
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[mt][0][4 * g + j] = sv[j] * w3c[0]; acc[mt][1][4 * g + j] = sv[j] * w3c[1]; }
      }
  } else {
    wide_zero<MT>(acc);
    wide_gemm<MT>(Xs, w3t, a.Np3, acc, ring);
  }
  TR(2);
  BfRing<PMX> bring;
  const s16x8* w2tp = PM > 0 ? reinterpret_cast<const s16x8*>(a.w2t_planes + m * a.planes_ms) : nullptr;
  if constexpr (PM > 0) bf_prefetch<PMX>(w2tp, bring);
  else wide_prefetch(w2t, HID, ring);             // next layer's first fragments overlap the mask epilogue
  int e2 = 0;
  {
    const float mx = wide_mask_apply<MT, MASK>(acc, mk2, rows_here, 1.f);
    if constexpr (PM == 4) f16_tile_max_put(mx, scr);
  }
  lds_barrier();
  if constexpr (PM == 4) e2 = f16_scale_exp(f16_tile_max_get(scr));
  PlaneSave gs{nullptr, 0, nullptr};
  if (PM == 4 && a.dz2p != nullptr) {              // the weight-gradient GEMM reads dz2 as the planes formed here
    gs.base = reinterpret_cast<short*>(a.dz2p) + m * a.dz2p_ms + (row0 / 8) * (HID * 8);
    gs.plane_stride = a.dz2p_plane;
    gs.e_out = a.e2_out + (long long)m * cdiv(a.rows, 32) + row0 / 32;
  }
  wide_store_colsum<MT, PM>(acc, Xs, dz2, rows_here, e2, cs, gs);
  if (with_db && lane < 32) { dbp[HID + 64 * w + lane] = cs[0]; dbp[HID + 64 * w + 32 + lane] = cs[1]; }
  lds_barrier();
  TR(3);
  // dh1 = dz2 * W2^T ; dz1 = dh1 * [h1 > 0]
  if constexpr (!BITS) mask_fetch<MT, MASK>(mk1, h1, m1, rows_here);
  wide_zero<MT>(acc);
  if constexpr (PM > 0) bf_gemm<MT, PMX, TB>(reinterpret_cast<const char*>(Xs), w2tp, acc, bring);
  else wide_gemm<MT>(Xs, w2t, HID, acc, ring);
  TR(4);
  NarrowRegs<(NT > 0 ? NT : 1)> br;
  if constexpr (DX && NT > 0) narrow_prefetch<NT>(w1t, 16 * NT, br);
  wide_mask_apply<MT, MASK>(acc, mk1, rows_here, PM == 4 ? exp2i(-(e2 + F16_WSHIFT)) : 1.f);
  lds_barrier();
  wide_store_colsum<MT, 0>(acc, Xs, dz1, rows_here, 0, cs);
  if (with_db && lane < 32) { dbp[64 * w + lane] = cs[0]; dbp[64 * w + 32 + lane] = cs[1]; }
  TR(5);
  if constexpr (DX) {
    lds_barrier();
    float* dx = a.dx + ((long long)m * a.rows + row0) * a.dx_n;
    auto emit = [&](int row, int col, float v) {
      const int c = col - a.dx_c0;
      if (row < rows_here && c >= 0 && c < a.dx_n) {
        if constexpr (SEED != SEED_RT) agent_store(dx + row * a.dx_n + c, v);
        else dx[row * a.dx_n + c] = v;
      }
    };
    if constexpr (NT > 0) narrow_run<TB / 16, NT>(Xs, br, emit);
    else narrow_layer(Xs, w1t, HID, a.Np1t, emit, TB);
  }
  TR(6);
}

}  // namespace mobody
