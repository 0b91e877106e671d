/* mobody_hip.h -- C ABI of the MI355X-native MOBODY hot path (libmobody_hip.so, gfx950).
 *
 * The reference (github guoyihonggyh/MOBODY-...) is pure Python/PyTorch and has no FFI
 * of its own; these entry points are what a binding for its hot path binds instead of
 * the ATen op sequences at the cited reference sites (paths relative to the reference):
 *
 *   mobody_dyn_forward   <- MOBODYModule.forward_trg/forward_src  algo/dynamics/mobody_module.py:315-330
 *   mobody_dyn_step      <- MOBODYEnsembleDynamics.step           algo/dynamics/mobody_dynamics.py:193-265
 *                           (+ termination predicates             algo/mb_utils/terminal_funs.py:10-149)
 *   mobody_ens_step      <- the same step() for either model and every uncertainty_mode   mobody_dynamics.py:193-265 (:241-252)
 *   mobody_ens_rollout   <- MOBODY.rollout + add_batch, likewise  mobody.py:596-657, utils.py:43-92
 *   mobody_ens_evaluate  <- eval_policy_batch, in the learned model   train_mobody.py:60-98
 *   mobody_mlp3_forward  <- Policy / DoubleQFunc / ValueFunc fwd  algo/offline_offline/mobody.py:35-83
 *   mobody_rollout       <- MOBODY.rollout + add_batch            algo/offline_offline/mobody.py:596-657, algo/utils.py:43-92
 *   mobody_gather_batch  <- ReplayBuffer.sample x3 + torch.cat    algo/utils.py:127-148, mobody.py:399-400,516-529
 *   mobody_ring_append   <- ReplayBuffer.add_batch (+ filter)     algo/utils.py:43-92, mobody.py:468,648-653
 *   mobody_critic        <- update_q_functions + backward (+ Adam.step + update_target)   mobody.py:189-208,544-552
 *   mobody_actor_forward / mobody_actor_backward
 *                        <- update_policy + bc_loss + backward (+ Adam.step)   mobody.py:246-276,314-345,555-573
 *   mobody_adam_polyak   <- Adam.step + update_target             mobody.py:127-131,183-187,548,552,573
 *   mobody_pretrain / mobody_pretrain_mopo
 *                        <- one learn() batch: zero_grad + loss.backward (+ Adam.step)   algo/dynamics/mobody_dynamics.py:594-642
 *   mobody_pretrain_*    <- MOBODYEnsembleDynamics.learn / validate  algo/dynamics/mobody_dynamics.py:300-384,594-653,1113-1140
 *   mobody_task_interact <- select_action + env.step + ReplayBuffer.add of the online modes, in the analytic task
 *                           train_mobody.py:675-770, iql.py:74-89,160-166, utils.py:25-41
 *   mobody_rng_*         <- torch.normal / np.random.choice / np.random.randint draws
 *                           (mobody_dynamics.py:220, mobody_module.py:355-357, utils.py:128)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch `tensor.data_ptr()`), fp32
 *     row-major contiguous unless stated; the caller owns every buffer; the library
 *     allocates nothing and needs no context object.  Between calls it keeps, per device, the
 *     pre-training side stream and the pointer to the caller's health words (mobody_health_bind);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no call
 *     synchronises; calls are graph-capturable;
 *   - every function returns 0 on success, a negative MOBODY_E* code otherwise and
 *     never throws; mobody_last_error() gives the text (thread local);
 *   - not thread safe per stream: one caller per stream.
 *   - network weights are passed as PACKED blobs whose layout is computed by
 *     mobody_dyn_layout / mobody_mlp_layout (zero padded [K_pad][N_pad] per member; matrices with
 *     N_pad == 256 are stored K-interleaved by four, element (k,n) at ((k/4)*256 + n)*4 + k%4, narrow
 *     ones row major); the host-side mirror (mobody_amd/packing.py) packs/unpacks the reference's
 *     state_dict tensors;
 *   - every launch of a call is ordered on the caller's `stream`; the library owns no stream of its own.
 */
#ifndef MOBODY_HIP_H
#define MOBODY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOBODY_ABI_VERSION 7
#define MOBODY_E_ARG (-1)      /* bad argument (dims, null pointer, unsupported size) */
#define MOBODY_E_LAUNCH (-2)   /* hipLaunch / runtime error */
#define MOBODY_E_UNSUPPORTED (-3)

#define MOBODY_HIDDEN 256
#define MOBODY_ENSEMBLE 7
#define MOBODY_LATENT 16

/* termination predicate ids (terminal_funs.py:123-149 dispatch, resolved on the host) */
enum { MOBODY_TERM_NEVER = 0, MOBODY_TERM_HALFCHEETAH = 1, MOBODY_TERM_HOPPER = 2, MOBODY_TERM_ANT = 3,
       MOBODY_TERM_WALKER2D = 4, MOBODY_TERM_HUMANOID = 5, MOBODY_TERM_PEN = 6 };

/* ---- packed layouts -------------------------------------------------------------------- */
typedef struct MobodyLayer {
  int32_t in_dim, out_dim;   /* logical dims actually used by the hot path */
  int32_t Kp, Np;            /* padded dims of the packed matrix W[member][Kp][Np] */
  int64_t w_off, b_off;      /* float offsets of member 0 inside the blob; bias is [member][Np] */
} MobodyLayer;

enum { MOBODY_DL_ZS1 = 0, MOBODY_DL_ZS2, MOBODY_DL_ZS3, MOBODY_DL_ZA_SRC1, MOBODY_DL_ZA_SRC2, MOBODY_DL_ZA_TRG1,
       MOBODY_DL_ZA_TRG2, MOBODY_DL_TR1, MOBODY_DL_TR2, MOBODY_DL_TR3, MOBODY_DL_RW1, MOBODY_DL_RW2, MOBODY_DL_RW3,
       MOBODY_DL_COUNT };

typedef struct MobodyDynLayout {
  int32_t S, A, E, _pad;
  MobodyLayer layer[MOBODY_DL_COUNT];
  int64_t total_floats;
} MobodyDynLayout;

/* 3-layer MLP (in -> 256 -> 256 -> out), `members` independent copies (twin-Q = 2).
 * Parameter blob, per member: W1[Kp1][256] b1[256] W2[256][256] b2[256] W3[256][Np3] b3[Np3]
 * (W stored [in][out], i.e. the transpose of nn.Linear.weight).  The same layout is used for
 * gradients and both Adam moments.  The "T" blob holds the transposes the backward pass
 * streams as MFMA B operands: W3T[Np3][256] W2T[256][256] W1T[256][Np1t] per member, followed by the 16-bit planes of
 * W2 and W2^T that the split-precision modes stream.  Precision modes (`precision` arguments, MobodyHyper.precision):
 *   0 "f32"     exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the reference's arithmetic
 *   1 "bf16"    one bf16 plane, one product (~3e-3)
 *   2 "bf16x2"  two bf16 planes, three products (~6e-6)
 *   3 "bf16x3"  three bf16 planes, six products: fp32-grade
 *   4 "f16x2"   two fp16 planes (w * 2^8 in the weight planes, per-tile power-of-two scales on the activation side),
 *               three products: fp32-grade at half the MFMA work of bf16x3
 * Modes 0-3 share one plane format (three bf16 planes); mode 4 keeps its two fp16 planes in the first two plane slots.
 * Whoever writes planes (mobody_mlp_transpose, the Adam entry points, mobody_dyn_planes) is told the mode. */
typedef struct MobodyMlpLayout {
  int32_t in_dim, out_dim, members, Kp1, Np3, Np1t;
  int64_t w1, b1, w2, b2, w3, b3;   /* float offsets inside one member */
  int64_t member_floats, total_floats;
  int64_t w3t, w2t, w1t;            /* float offsets inside one member of the T blob */
  int64_t t_member_floats, t_total_floats;
  int64_t w2p, w2tp;                /* float offsets (inside one member of the T blob) of the planes of W2 and W2^T:
                                       [3 planes][32][256][8] 16-bit each, x = x0 + x1 (+ x2) (split-precision modes) */
} MobodyMlpLayout;

const char* mobody_last_error(void);
int mobody_abi_version(void);
/* S in [2, 127], A in [1, 64] and 2S + A <= 256 (the reward head's input is one 256-wide tile: S = 127 only with A <= 2). */
int mobody_dyn_layout(int S, int A, MobodyDynLayout* out);
int mobody_mlp_layout(int in_dim, int out_dim, int members, MobodyMlpLayout* out);

/* ---- optional per-kernel timing (measurement only; process-global state) ----
 * Between prof_begin and prof_end every launch of the heavy kernel families is bracketed by a HIP
 * event pair on its launch stream.  prof_end SYNCHRONISES, then returns the summed milliseconds
 * and launch counts per family id: 0 mlp3_fwd, 1 mlp3_bwd, 2 wgrad, 3 dyn_fwd (4..7 reserved). */
#define MOBODY_PROF_IDS 8
int mobody_prof_begin(int max_events);
int mobody_prof_end(double* ms_by_id, int64_t* count_by_id, int n_ids);

/* ---- device health words ------------------------------------------------------------------
 * A caller-owned block of MOBODY_HEALTH_WORDS int32 in device memory that the kernels writing weights report into, so
 * that a fault is seen where it happens and not when NaN reaches the host:
 *   words[0]  bit mask.  MOBODY_HEALTH_F16_RANGE: a value w with !(|w| < MOBODY_F16_W_LIMIT) was written into a
 *             precision-4 ("f16x2") weight plane, whose fp16 terms of w * 2^8 then hold Inf (online and target planes, W2
 *             and W2^T; the optimizer entry points, mobody_mlp_transpose, mobody_dyn_planes and the pre-training
 *             transposes).  MOBODY_HEALTH_NONFINITE: an optimizer step produced a non-finite parameter (every mode).
 *   words[1]  Adam step count of the first optimizer launch that raised a bit (0: none, or a plane builder did)
 *   words[2..3] internal (one 64-bit key of that launch; the block must be 8-byte aligned); words[4..] reserved
 * Lanes write (atomically) only when they see a violation; a clean run costs one compare per parameter.
 * FREEZE: every entry point that applies an optimizer step (mobody_adam_polyak, the fused forms -- m, v given -- of mobody_critic,
 * mobody_actor_backward, mobody_pretrain and mobody_pretrain_mopo, mobody_pretrain[_mopo]_adam, mobody_pretrain_za_adam) reads
 * words[0] on entry; when an
 * EARLIER launch has set a bit it applies nothing -- parameters, moments, target, T blob, planes and `bump` stay as they
 * are (gradient and loss outputs are still written).  The launch in which the fault happens completes: its fp32 results
 * are exact, only the plane holds Inf.  So the state stops at the last update computed from healthy planes, however many
 * replayed steps pass before the host looks.  A captured optimizer launch must read a device step count that advances
 * between replays (a `t_dev` word, as replay requires anyway): that is how a replay tells itself from the faulting one.
 * CONSEQUENCE for callers that pass `t_dev`: whatever advances those step words keeps advancing them while the updates are
 * frozen (only `bump` stops), so after a fault they run ahead of the steps that were applied: words[1] holds the faulting
 * launch's own count, and the caller re-seeds its step words from it before it goes on (the host mirror does).
 * OVERLAP: the verdict is taken per workgroup when it starts.  It is one verdict per launch as long as no other optimizer
 * launch raises a fault while the launch runs; an optimizer launch that overlaps the faulting one on another stream (the
 * pre-training step runs its nets' optimizer launches on two streams) may be applied in part -- each element it applied is a
 * complete, finite step computed from healthy planes.
 * With no block bound, or a bound block that stays zero, every output is bit-identical to a library without the guard.
 * mobody_health_bind stores the pointer for the CURRENT device (NULL unbinds); launches pass it to their kernels as an
 * argument, so a graph captured after the bind carries it.  mobody_health_clear zeroes the block on `stream`. */
#define MOBODY_HEALTH_WORDS 8
#define MOBODY_HEALTH_F16_RANGE 1
#define MOBODY_HEALTH_NONFINITE 2
#define MOBODY_F16_W_LIMIT 255.875f   /* 65504 / 2^8 */
int mobody_health_bind(int32_t* words_dev);
int mobody_health_clear(void* stream);

/* ---- counter based RNG (Philox4x32-10; CPU twin: oracle/mobody_oracle.py rng_*) ---------- */
int mobody_rng_normal(uint32_t seed, uint32_t stream_id, uint32_t call, int64_t n, float* out, void* stream);
int mobody_rng_index(uint32_t seed, uint32_t stream_id, uint32_t call, int64_t n, uint32_t bound, int32_t* out,
                     void* stream);

/* ---- ensemble dynamics ----------------------------------------------------------------- */
/* mean[E][B][S] = forward_trg/forward_src(obs, act) in inference mode. */
int mobody_dyn_forward(const float* dyn_blob, const float* dyn_planes, int precision, int S, int A, const float* obs,
                       const float* act, int64_t B, int use_trg, float* mean, void* stream);
/* dyn_planes / precision (here and in mobody_dyn_step / mobody_rollout): 0 = exact fp32 MFMA (planes may be NULL);
 * 1 bf16, 2 bf16x2, 3 bf16x3, 4 f16x2 = the three 256 x 256 layers of every member (zs2, transition2, reward_model2) on the
 * split-precision core, streaming the planes mobody_dyn_planes built from the blob FOR THAT MODE
 * (mobody_dyn_planes_floats() floats: [3 layers][7 members][3 planes][65536] 16-bit). */
int64_t mobody_dyn_planes_floats(void);
int mobody_dyn_planes(const float* dyn_blob, int S, int A, float* planes, int precision, void* stream);

/* floats of scratch mobody_dyn_step needs for a batch of B rows */
int64_t mobody_dyn_step_workspace(int S, int A, int64_t B);

/* One imagined transition for B rows (A.1 of SURVEY.md).
 *   noise      [E][B][S] unit normals, or NULL -> generated on device from (seed, call + call_dev[0])
 *   call_dev   optional device int64 word added to `call` (NULL = 0): a captured HIP graph keeps its step counter on the
 *              device, so every replay draws fresh noise without new kernel arguments
 *   elite_idx  [B] member id per row,   or NULL -> elites[philox % n_elites]
 *   alive      [B] optional uint8 mask (NULL = all alive); dead rows are computed but flagged
 *              terminal=1 so an on-device multi-step rollout can keep fixed row indices
 *   elites     HOST array of n_elites member ids (MOBODYModule.elites), used when elite_idx is NULL
 *   outputs    next_obs[B][S], reward[B], terminal[B] (uint8), penalty[B], raw_reward[B] (nullable)
 *   mean_out   optional [E][B][S] copy of the ensemble means (info['samples']) */
int mobody_dyn_step(const float* dyn_blob, const float* dyn_planes, int precision, int S, int A, int task,
                    const float* obs, const float* act, int64_t B,
                    const float* noise, const int32_t* elite_idx, const uint8_t* alive, const int32_t* elites,
                    int n_elites, uint32_t seed,
                    uint32_t call, const int64_t* call_dev, float penalty_coef, int use_penalty, int use_trg, float* next_obs,
                    float* reward,
                    uint8_t* terminal, float* penalty, float* raw_reward, float* mean_out, float* workspace,
                    void* stream);

/* The same step for the MOPO ablation (config['mopo'] = 1, mobody_module.py:114-118,218-219,251-254,264-266,288-289): the
 * ensemble means are obs + MLP_e([obs, act]) with the 7-member Swish MLP za_src1..3 (S+A -> 256 -> 256 -> S) packed as
 * mobody_mlp_layout(S + A, S, 7) (mopo_blob; mopo_blob_T from mobody_mlp_transpose, needed when precision != 0);
 * encoders / decoder are bypassed and forward_trg == forward_src, so there is no use_trg.  The reward head is read
 * from dyn_blob exactly as in mobody_dyn_step; every other argument has the same meaning. */
int mobody_mopo_step(const float* dyn_blob, const float* dyn_planes, const float* mopo_blob, const float* mopo_blob_T,
                     int precision, int S, int A, int task, const float* obs, const float* act, int64_t B,
                     const float* noise, const int32_t* elite_idx, const uint8_t* alive, const int32_t* elites,
                     int n_elites, uint32_t seed, uint32_t call, float penalty_coef, int use_penalty, float* next_obs,
                     float* reward, uint8_t* terminal, float* penalty, float* raw_reward, float* mean_out,
                     float* workspace, void* stream);

/* uncertainty_mode of MOBODYEnsembleDynamics (mobody_dynamics.py:241-252): which penalty the sample kernel forms from the
 * ensemble means (avg = their mean over the 7 members, var_d = the unbiased variance over the members of state dim d) */
enum { MOBODY_UNC_PAIRWISE = 0,    /* 'pairwise-diff' amax_e ||mean_e - avg||_2 over d < S-1              (:246-249) */
       MOBODY_UNC_ALEATORIC = 1,   /* 'aleatoric'     amax_e ||std_e||_2 = sqrt(sum_{d < S} var_d): ALL S dims (:241-243) */
       MOBODY_UNC_ENS_STD = 2 };   /* 'ensemble_std'  sqrt(mean_{d < S-1} var_d)                           (:250-252) */

/* MOBODYEnsembleDynamics.step (mobody_dynamics.py:193-265) in every runnable variant, arguments by name: what
 * mobody_dyn_step takes (same meanings), plus
 *   mopo_blob / mopo_blob_T  NULL = the latent model; else the MOPO ablation's 7-member MLP as in mobody_mopo_step
 *                            (use_trg is ignored: forward_trg == forward_src, mobody_module.py:264-266)
 *   uncertainty_mode         MOBODY_UNC_* (:241-252); any other value is MOBODY_E_ARG (the reference raises ValueError)
 *   call_dev                 for both models
 * struct_bytes = sizeof(MobodyEnsStep) (a binding built against another header is refused).  A NaN / Inf member mean
 * makes the row's penalty NaN in every mode, as torch's amax / norm / var / sqrt do.  mobody_dyn_step and mobody_mopo_step
 * are this call with MOBODY_UNC_PAIRWISE.  workspace: mobody_dyn_step_workspace(S, A, B) floats. */
typedef struct MobodyEnsStep {
  int32_t struct_bytes, uncertainty_mode;
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T;
  int32_t precision, S, A, task;
  const float *obs, *act;
  int64_t B;
  const float* noise; const int32_t* elite_idx; const uint8_t* alive;
  const int32_t* elites;            /* HOST array */
  int32_t n_elites; uint32_t seed, call; int32_t use_penalty;
  const int64_t* call_dev;
  float penalty_coef; int32_t use_trg;
  float *next_obs, *reward; uint8_t* terminal; float *penalty, *raw_reward, *mean_out, *workspace;
} MobodyEnsStep;
int mobody_ens_step(const MobodyEnsStep* a, void* stream);

/* ---- replay buffer views (used by the rollout below and by the gather / append entry points) ---- */
typedef struct MobodyBufferView {   /* ReplayBuffer fields, algo/utils.py:19-23 */
  const float* state; const float* action; const float* next_state; const float* reward; const float* not_done;
  int64_t pitch;   /* floats between consecutive rows of EVERY field; 0 = five separate contiguous arrays
                      ([rows][S], [rows][A], [rows][S], [rows], [rows]: the reference's shape) */
} MobodyBufferView;
/* Row-interleaved ring (what the mirror's ReplayBuffer allocates): one allocation of [rows][pitch] floats with
 * pitch = mobody_ring_pitch(S, A) = 2S+A+2 rounded up to 16 floats (64 bytes), a row laid out
 * state[S] | action[A] | next_state[S] | reward | not_done | zero padding, i.e. state = base, action = base + S,
 * next_state = base + S + A, reward = base + 2S + A, not_done = reward + 1.  A view of exactly this shape with a
 * 16-byte aligned base takes the kernels' fast path (a random row = whole aligned 64-byte sectors, 16-byte accesses);
 * any other view (separate arrays, other pitches) is handled piecewise. */
int64_t mobody_ring_pitch(int S, int A);

/* The whole H-step imagined rollout on the device, appended to a ring buffer (MOBODY.rollout + add_batch,
 * mobody.py:596-657, utils.py:43-92): per step a = pi(s) (actor blob, mobody_mlp_layout(S, A, 1)), one fused ensemble
 * step with device-Philox noise / elite picks at call id call0 + t, the penalty filter (`penalty <= env_filter` when
 * filter_bad_rollout) and the alive update formed in the sample kernel, and a two-launch stream-compacting append of the
 * kept rows: 7 launches per step, no host work and no synchronisation between steps.  Rows keep their index across
 * steps; a row that terminated is computed but never appended again (the reference drops it from the batch, :635-639).
 * NB quirk Q1: MOBODY.rollout passes its `use_trg` argument in step()'s `use_penalty` slot -- callers mirror that here.
 * workspace: mobody_rollout_workspace(S, A, B) floats. */
int64_t mobody_rollout_workspace(int S, int A, int64_t B);
int mobody_rollout(const float* dyn_blob, const float* dyn_planes, const float* actor_blob, const float* actor_blob_T,
                   int precision, int S, int A, int task, float max_action,
                   const float* init_obs, int64_t B, int H, const int32_t* elites, int n_elites, uint32_t seed, uint32_t call0,
                   float penalty_coef, int use_penalty, int use_trg, float env_filter, int filter_bad_rollout,
                   const MobodyBufferView* ring, int64_t cap, int64_t* ptr_size, float* workspace, void* stream);

/* MOBODY.rollout + add_batch (mobody.py:596-657, utils.py:43-92) for either model and every uncertainty_mode, arguments by
 * name: what mobody_rollout takes (same meanings), plus mopo_blob / mopo_blob_T, uncertainty_mode and call_dev as in
 * MobodyEnsStep (step t draws at call id call0 + t + call_dev[0]).  The mopo form has the latent form's 7 launches per
 * horizon step -- policy forward, member MLP with the observation added in its output stage, sample with filter / alive
 * update, reward head, finalize, the two-launch append -- and no host work between steps.  mobody_rollout is this call
 * with the latent model and MOBODY_UNC_PAIRWISE.  workspace: mobody_ens_rollout_workspace(a) floats (reads S, A, B). */
typedef struct MobodyEnsRollout {
  int32_t struct_bytes, uncertainty_mode;
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T, *actor_blob, *actor_blob_T;
  int32_t precision, S, A, task;
  const float* init_obs;
  int64_t B;
  int32_t H, n_elites;
  const int32_t* elites;            /* HOST array */
  uint32_t seed, call0;
  const int64_t* call_dev;
  float max_action, penalty_coef, env_filter; int32_t use_penalty, use_trg, filter_bad_rollout;
  const MobodyBufferView* ring;
  int64_t cap;
  int64_t* ptr_size;
  float* workspace;
} MobodyEnsRollout;
int64_t mobody_ens_rollout_workspace(const MobodyEnsRollout* a);
int mobody_ens_rollout(const MobodyEnsRollout* a, void* stream);

/* The policy's return in the learned model, on the device: the stand-in for eval_policy_batch (train_mobody.py:60-98) in a
 * build without simulators -- B episodes are rolled through the ensemble for H steps and their rewards summed per row,
 * the terminating step's reward included (`reward_all[i, :done_index[i] + 1]`, :86-93).  Fields as MobodyEnsRollout, plus
 * the caller-owned ROW STATE (in/out).  resume == 0 first sets, per row b, obs_state = init_obs[b], alive = 1,
 * ret = pen_sum = 0, length = 0, disc = 1; resume == 1 continues from the state as it is.  Then for t = 0 .. H-1:
 *   a = pi(obs_state)                       the bits of mobody_mlp3_forward(out_mode 1, max_action)
 *   (obs', raw, term, pen) = mobody_ens_step(obs_state, a) with the current alive mask, noise = elite_idx = NULL, call id
 *                            call0 + t + call_dev[0], use_penalty = 0 (raw = the ensemble's mean reward), this block's
 *                            use_trg, uncertainty_mode and model
 *   if alive:  ret = fmaf(disc, raw, ret);  pen_sum += pen;  length += 1;  disc = disc * discount
 *   alive = alive && !term;  obs_state = obs'
 * Rows that died keep their index and are computed but never accumulated.  H == 0 with resume == 0 only initialises.
 * 5 launches per step (policy forward, member forward, sample, reward head, accounting), one more for the initialisation;
 * no host work and no synchronisation between steps.  With resume = 1 and call_dev a captured chunk of C steps is replayed
 * ceil(H / C) times (mobody_counter_add inside the graph advances the call word).  MOBODY_E_ARG, before any runtime call:
 * struct_bytes, uncertainty_mode, B < 0, H < 0, resume not 0 / 1, discount NaN or outside (0, 1], every null pointer
 * (init_obs only when resume == 0), precision / planes as mobody_ens_rollout.  B == 0 returns 0.
 * workspace: mobody_ens_evaluate_workspace(a) floats (reads S, A, B).
 * (Declared as a tagged struct plus its typedef: the layout is that of `typedef struct MobodyEnsEval { ... } MobodyEnsEval`.) */
struct MobodyEnsEval {
  int32_t struct_bytes, uncertainty_mode;
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T, *actor_blob, *actor_blob_T;
  int32_t precision, S, A, task;
  const float* init_obs;            /* [B][S]; read only when resume == 0 */
  int64_t B;
  int32_t H, n_elites;
  const int32_t* elites;            /* HOST array */
  uint32_t seed, call0;
  const int64_t* call_dev;          /* nullable */
  float max_action, discount;       /* discount in (0, 1] */
  int32_t use_trg, resume;
  float* obs_state;                 /* [B][S] current observation */
  uint8_t* alive;                   /* [B] */
  float *ret, *pen_sum, *disc;      /* [B] each */
  int32_t* length;                  /* [B] */
  float* workspace;
};
typedef struct MobodyEnsEval MobodyEnsEval;
int64_t mobody_ens_evaluate_workspace(const MobodyEnsEval* a);
int mobody_ens_evaluate(const MobodyEnsEval* a, void* stream);

/* Open-loop model error over recorded trajectories, on the device: B windows of a transition dataset held in dataset
 * order (`data`, rows 0 .. data_rows-1; ring form pitch >= 2S+A+2 or five arrays, pitch 0) are replayed through the ensemble
 * -- the model starts at the recorded state of row row0[b], is fed the RECORDED actions, and its state, reward and
 * termination flag are compared with the recorded ones at every step (the compounding-error curve).  Model fields as
 * MobodyEnsEval.  First, per row b:  obs_state[b] = data.state[row0[b]],  act_state[b] = data.action[row0[b]].  Then for
 * t = 0 .. H-1, with data row r = min(row0[b] + t, data_rows - 1):
 *   (obs', raw, term, pen) = mobody_ens_step(obs_state, act_state) with alive = NULL, noise = elite_idx = NULL, call id
 *                            call0 + t + call_dev[0], use_penalty = 0 (raw = the ensemble's mean reward: seven adds, one
 *                            multiply by 1/7), this block's use_trg, uncertainty_mode and model
 *   obs_err[t][b]    = sqrtf(sum_{d=0..S-1} (obs'[b][d] - data.next_state[r][d])^2)   fp32, sequential in increasing d, no fma
 *   rew_err[t][b]    = raw - data.reward[r]                                          signed; the caller squares it
 *   penalty[t][b]    = pen;   term_model[t][b] = term (the predicate on the model's obs')
 *   obs_state[b]     = (reset_every > 0 && (t + 1) % reset_every == 0) ? data.next_state[r] : obs'
 *   act_state[b]     = data.action[min(r + 1, data_rows - 1)]
 * reset_every = 0 is the open loop, reset_every = 1 the one-step error at every offset of the window.  Every row runs all H
 * steps; nothing is masked, so a NaN from the model stays visible in the tables.  4 launches per step (member forward,
 * sample, reward head, accounting) plus one for the row state; no host work and no synchronisation between steps.
 * row0 lives on the device and is NOT checked: the kernels clamp every row index into [0, data_rows - 1], so no load
 * leaves the view, but a window that runs over an episode boundary or past the last row compares against rows that do
 * not belong to it -- choosing windows with row0[b] >= 0 and row0[b] + H <= data_rows inside one episode is the caller's
 * job.  MOBODY_E_ARG, before any runtime call: struct_bytes, uncertainty_mode, B < 0, H < 0, reset_every < 0, and when
 * B > 0 data_rows < 1, every null pointer (data and its state / action / next_state / reward count; not_done is not
 * read; the four tables only when H > 0), a pitch that is neither 0 nor at least 2S+A+2, n_elites, task, precision / planes / T blob as
 * mobody_ens_evaluate.  B == 0 returns 0; H == 0 with B > 0 only sets the row state.
 * workspace: mobody_ens_replay_workspace(a) floats (reads S, A, B). */
struct MobodyEnsReplay {
  int32_t struct_bytes, uncertainty_mode;
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T;
  int32_t precision, S, A, task;
  const MobodyBufferView* data;
  int64_t data_rows;
  const int64_t* row0;              /* DEVICE array [B] */
  int64_t B;
  int32_t H, reset_every, n_elites;
  const int32_t* elites;            /* HOST array */
  uint32_t seed, call0;
  const int64_t* call_dev;          /* nullable */
  int32_t use_trg;
  float *obs_state, *act_state;     /* [B][S], [B][A] */
  float *obs_err, *rew_err, *penalty;   /* [H][B] each */
  uint8_t* term_model;              /* [H][B] */
  float* workspace;
};
typedef struct MobodyEnsReplay MobodyEnsReplay;
int64_t mobody_ens_replay_workspace(const MobodyEnsReplay* a);
int mobody_ens_replay(const MobodyEnsReplay* a, void* stream);

/* Termination predicate alone: done[B] (uint8) = terminal_fn(next_obs[B][S])  (terminal_funs.py:10-121). */
int mobody_termination(int task, const float* next_obs, int64_t B, int S, uint8_t* done, void* stream);

/* Bookkeeping of an on-device multi-step rollout (MOBODY.rollout mobody.py:635-653 without host
 * compaction): keep[b] = alive_in[b] && (!use_filter || penalty[b] <= env_filter);
 * alive_out[b] = alive_in[b] && !terminal[b].  alive_in == NULL means all alive; alive_out may alias alive_in. */
int mobody_rollout_mask(const uint8_t* alive_in, const uint8_t* terminal, const float* penalty, float env_filter,
                        int use_filter, int64_t B, uint8_t* keep, uint8_t* alive_out, void* stream);

/* Replay indices drawn on the device (np.random.randint(0, size, n), utils.py:128, throughput mode):
 * out[i] = philox(seed, stream_id, call = (uint32)(counter[0] + call_offset))[i] % size[0]-ish
 * (multiply-high), with `counter` and `size` read from DEVICE int64 words so a captured graph
 * advances without new kernel arguments.  size[0] must be >= 1. */
int mobody_sample_indices(uint32_t seed, uint32_t stream_id, const int64_t* counter, int64_t call_offset, int64_t n,
                          const int64_t* size, int32_t* out, void* stream);

/* counter[i] += inc for i < n (device int64 words, n <= 64): one launch advances the RNG call id and both Adam
 * step counts of a captured train() step */
int mobody_counter_add(int64_t* counter, int n, int64_t inc, void* stream);

/* ---- 3-layer MLP forward (ReLU) -------------------------------------------------------- */
/* x = concat(src0[rows][n0], src1[rows][n1]) (src1 may be NULL), n0+n1 == in_dim.
 * out_mode 0: out[m][rows][out_dim] raw;  1: max_action*tanh(.) (Policy.forward mobody.py:68-72).
 * save_x [rows][Kp1], save_h1/save_h2 [members][rows][256] are optional (backward inputs). */
int mobody_mlp3_forward(const float* blob, const float* blob_T, int precision, int in_dim, int out_dim, int members,
                        const float* src0, int n0, const float* src1, int n1, int64_t rows, int out_mode,
                        float max_action, float* out, float* save_x, float* save_h1, float* save_h2, void* stream);
/* blob_T / precision: 0 = exact fp32 MFMA (blob_T may be NULL); 1..4 = the split-precision modes, which stream W2's
 * planes from the T blob (mobody_mlp_transpose builds them, the Adam kernels keep them current -- both for the SAME mode). */

/* ---- replay gather / ring append ------------------------------------------------------- */
/* Concatenate rows idx_k of up to three buffers (src | tar | fake order, mobody.py:525-529)
 * into one minibatch: state[N][S] action[N][A] next_state[N][S] reward[N] not_done[N]. */
int mobody_gather_batch(const MobodyBufferView* bufs, const int32_t* const* idx, const int64_t* counts, int nbuf,
                        int S, int A, float* state, float* action, float* next_state, float* reward, float* not_done,
                        void* stream);

/* Same gather with the row indices drawn on the device (np.random.randint(0, size, n), utils.py:128, throughput
 * mode): index i of source k = philox(seeds[k], stream 3, call)[i] * size >> 32 with
 * call = (counter ? counter[0] : 0) + call_offsets[k] and size read from the DEVICE word sizes[k][0]
 * (`seeds`, `call_offsets`, `counts` and the `sizes` pointer array are host arrays).  Identical draws to
 * mobody_rng_index / mobody_sample_indices for the same (seed, call).  `bump`: host array of nbump <= 4 device int64
 * words (none of them `counter`) that one thread of the launch increments by one (a captured step advances its Adam
 * step counts here); nbump = 0: none. */
int mobody_gather_batch_rng(const MobodyBufferView* bufs, const int64_t* counts, int nbuf, int S, int A,
                            const uint32_t* seeds, const int64_t* call_offsets, const int64_t* counter,
                            const int64_t* const* sizes, float* state, float* action, float* next_state,
                            float* reward, float* not_done, int64_t* const* bump, int nbump, void* stream);

/* Append the rows with keep[i] != 0 (NULL = all), in order, to the ring `ring` of `cap` rows (written through the
 * view's pointers) at *ptr_size (device int64[2] = {ptr, size}), reproducing add_batch's single-wrap arithmetic
 * (utils.py:43-92); not_done = 1 - terminal; the row-interleaved ring also gets its row padding zeroed.
 * `scan_ws` needs (M + 1040) int32 whose FIRST EIGHT must be zero on entry (zero the workspace once when allocating it;
 * every call leaves them zero: they hold the scan's arrival ticket, and a memset launch per append would cost more than
 * a short append itself).  Two launches: a block scan whose last block commits the new {ptr, size}, and the row scatter. */
int mobody_ring_append(const MobodyBufferView* ring, int64_t cap, int64_t* ptr_size, int S, int A, const float* obs,
                       const float* act, const float* next_obs, const float* reward, const uint8_t* terminal,
                       const uint8_t* keep, int64_t M, int32_t* scan_ws, void* stream);

/* ---- training step --------------------------------------------------------------------- */
typedef struct MobodyTrainDims {
  int32_t S, A;
  int64_t N;          /* rows of the mixed critic batch on this rank */
  int64_t Nt;         /* leading rows that form the "true" BC batch (src|tar) */
  int64_t N_global;   /* sum of N over data-parallel ranks (== N on one GPU) */
  int64_t Nt_global;
} MobodyTrainDims;

typedef struct MobodyHyper {
  float gamma, tau, max_action, weight, bc_coef;
  int32_t q_weighted, scale_q;
  int32_t precision;   /* MFMA mode of the 256 x 256 GEMMs of the forward and backward passes and of the 256 x 256
                          weight-gradient job: 0 exact fp32 (the reference's arithmetic), 1 bf16, 2 bf16x2, 3 bf16x3, 4 f16x2;
                          the update entry points also write the nets' W2 planes in this mode's format */
} MobodyHyper;

/* floats of scratch the training calls need.  The SAME workspace has to be handed to mobody_actor_forward and the
 * following mobody_actor_backward: it carries pi(s), the Q values, the saved activations and the ReLU sign words
 * between the two calls (the data-parallel caller all-reduces `stats` in between); one MobodyActor block serves both. */
int64_t mobody_train_workspace(const MobodyTrainDims* d);

/* ---- argument blocks of the train step: every field named, as MobodyEnsStep ----------------------------------------
 * struct_bytes = sizeof(the block) (a binding built against another header is refused before anything else is read);
 * MobodyTrainDims and MobodyHyper are embedded by value.  GRADIENT-ONLY OR FUSED is chosen by the fields: exactly one of the
 * gradient blob (grad_q / grad_actor / grad) and the optimizer state m, v is non-NULL; both or neither is MOBODY_E_ARG.
 *   gradient blob given   the data-parallel form: the gradient is written (SUM all-reduce it, then mobody_adam_polyak)
 *   m, v given            the single-GPU form: the gradient reduction applies the Adam step (1-based t, or the device word
 *                         t_dev[0] when t_dev != NULL) itself, so the gradient blob is never written -- one launch and one
 *                         gradient round trip fewer.  Bit-identical to the gradient form followed by mobody_adam_polyak.
 * Every argument check runs before the first HIP runtime call. */

/* Critic update (A.2; update_q_functions + backward, mobody.py:189-208,540-552): grad_q (MobodyMlpLayout(S+A,1,2) layout) or,
 * fused, the Adam step of q_blob and the Polyak update of qtarg_blob (tau from `h`); loss_out[0] = L_Q of the LOCAL rows
 * scaled by 1/N_global (sum over ranks == global loss). */
typedef struct MobodyGatherRng {   /* mobody_gather_batch_rng's host arrays */
  const MobodyBufferView* bufs;
  const int64_t* counts;
  int nbuf;
  const uint32_t* seeds;
  const int64_t* call_offsets;
  const int64_t* counter;
  const int64_t* const* sizes;
  int64_t* const* bump;
  int nbump;
} MobodyGatherRng;
typedef struct MobodyCritic {
  int32_t struct_bytes;
  int32_t phase;            /* 0 the whole step.  1 / 2: the step in two calls -- phase 1 enqueues its forwards (none of them
                               reads `reward`), phase 2 the backward, the weight gradients and the reduction / optimizer step.
                               Between the two the caller may join a stream that rewrites `reward` (penalty_type 'par',
                               mobody.py:428-434: an ensemble step on the source rows that otherwise sits in front of the critic) */
  MobodyTrainDims d;
  MobodyHyper h;
  const float *actor_blob, *actor_blob_T;   /* actor_blob_T / qtarg_blob_T are only read when h.precision != 0 (their W2
                                               planes); NULL is fine at precision 0 */
  float *q_blob, *q_blob_T;                 /* written by the fused form only */
  float *qtarg_blob;
  float *qtarg_blob_T;      /* nullable: the target net's T blob; when given, the W2 planes of the target follow the Polyak update */
  float *state, *action, *next_state, *reward, *not_done;   /* the minibatch: read -- or, with `gather`, WRITTEN */
  const float* q_next;      /* NULL -> min target-Q(s', pi(s')) is computed here (update_q_functions, mobody.py:189-208);
                               non-NULL -> [N] bootstrap values supplied by the caller, V(s') in the advantage variant
                               (update_q_functions_1, :210-229; actor_blob / qtarg_blob / next_state may then be NULL) */
  float* grad_q;
  float *m, *v;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  int32_t policy_forward;   /* != 0 (needs q_next == NULL): the target-Q launch also evaluates pi(s) with its saves for the coming
                               mobody_actor_forward (policy_ready = 1) on the same workspace -- the actor does not change in
                               between, and the merged launch fills the chip better than the two it replaces */
  float *loss_out, *workspace;
  int64_t* bump;            /* nullable, != t_dev, fused form only: a device int64 word the optimizer launch increments by one -- a
                               captured step advances the RNG call id it has already consumed here instead of in a launch of
                               its own */
  const MobodyGatherRng* gather;
                            /* NULL: none.  Else mobody_gather_batch_rng + this call in one call and one launch fewer: the
                               step's first forward launch (twin-Q(s,a) next to pi(s')) draws its tiles' row indices and takes
                               the rows straight from the rings, and writes the minibatch arrays state .. not_done for the
                               launches behind it and for the caller.  Same draws, same bump words, bit-identical results to
                               the two calls.  Its counts must add up to d.N.  Refused with MOBODY_E_ARG: a source with rows
                               to draw that is not a row-interleaved ring (mobody_ring_pitch), q_next != NULL, phase != 0 (the
                               first forward launch writes the minibatch the backward reads) */
} MobodyCritic;
int mobody_critic(const MobodyCritic* a, void* stream);

/* Actor phase (update_policy + bc_loss + backward, mobody.py:246-276,314-345,554-578): ONE block for its two calls, filled
 * once; mobody_actor_forward reads the fields up to `workspace` and policy_ready, mobody_actor_backward all but policy_ready.
 *   mobody_actor_forward   part 1: forwards + the two batch statistics stats[0]=sum|min Q(s,pi(s))|,
 *                          stats[1]=sum|min Q(s_t,a_t)| over LOCAL rows (all-reduce them across ranks before part 2)
 *   mobody_actor_backward  part 2: grad_actor (MobodyMlpLayout(S,A,1)) or, fused, the Adam step of actor_blob (no target);
 *                          loss_out[0]=L_pi, [1]=L_BC (local share) */
typedef struct MobodyActor {
  int32_t struct_bytes;
  int32_t policy_ready;     /* != 0: pi(s) and its saves are already in the workspace (mobody_critic with policy_forward = 1) */
  MobodyTrainDims d;
  MobodyHyper h;
  float *actor_blob, *actor_blob_T;         /* written by the fused form only */
  const float *q_blob, *q_blob_T, *state, *action;
  float* stats;
  float* workspace;
  const float* v_true;      /* NULL -> BC weights exp(3*q_b/mean|q_b|); [Nt] V(s_true) -> exp(3*(q_b - V)) (config['advantage'],
                               :255-256) */
  float* grad_actor;
  float *m, *v;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  float* loss_out;
} MobodyActor;
int mobody_actor_forward(const MobodyActor* a, void* stream);
int mobody_actor_backward(const MobodyActor* a, void* stream);

/* TD3_BC actor phase (the reference's td3_bc.py update_policy :160-176) on the same MobodyActor block, workspace and call order as
 * the pair above (mobody_critic serves TD3_BC's critic update as it is).  BC runs on EVERY row against the batch's own actions,
 * weighted -- when h.q_weighted (the reference's config['advantage'] == 1) -- by w = min(exp(q/m), 100), q = min Q(s, pi(s)) the
 * policy term uses, m = stats[0]/N_global; q is not detached inside w, so the BC loss also reaches the actor through the frozen Q.
 *   mobody_td3bc_actor_forward    pi(s) unless policy_ready, ONE twin-Q forward Q(s, pi(s)), stats[0] = sum|q|, stats[1] = 0
 *                                 (no Q(s_t, a_t) forward: N twin-Q rows fewer than mobody_actor_forward)
 *   mobody_td3bc_actor_backward   grad_actor or, fused, the Adam step (same rule, t / t_dev as above); loss_out as above
 * Refused with MOBODY_E_ARG before any runtime call: d.Nt != d.N, d.Nt_global != d.N_global, v_true != NULL, h.scale_q != 1,
 * d.A > 24.  With h.q_weighted == 0 the results are the bits of the pair above at q_weighted = 0, scale_q = 1, Nt = N. */
int mobody_td3bc_actor_forward(const MobodyActor* a, void* stream);
int mobody_td3bc_actor_backward(const MobodyActor* a, void* stream);

/* BOSA actor phase (the reference's bosa.py:612-629) on the same MobodyActor block (its size stays) and workspace:
 * pi = actor(s), q = critic_1(s, pi) -- member 0 of the twin-Q blob ALONE, not the minimum --, norm_q = 1 / mean|q| detached,
 * actor_loss = -norm_q mean(q) + lamda mean(-ll(s, pi)).  The second term reaches the actor as a per-element addend.
 *   mobody_bosa_actor_forward   pi(s) with its saves, member 0's Q(s, pi) with its ReLU signs, stats[0] = sum |q_0|, stats[1] = sum q_0
 *                               over the local rows; pi_out [N][A] is a copy of pi(s): what the caller hands to
 *                               mobody_bosa_loglik_grad as `action`.  a->action is not read.  3 launches and the copy.
 *   mobody_bosa_actor_backward  dq_0/da under the seed -(1/m)/N_global, m = stats[0]/N_global (:614, :620); d(pre-tanh) = (dq_0/da +
 *                               dpi_extra) * max_action (1 - (pi / max_action)^2) with dpi_extra [N][A] from the caller (BOSA:
 *                               -(lamda / N) dll_da, :617-620); the actor's weight gradients into grad_actor or, fused, its Adam step
 *                               (t / t_dev as above).  loss_out[0] = -(1/m) stats[1] / N_global, loss_out[1] = 0.  6 launches: two
 *                               row-wise seeds, the two backwards in seed mode 0, the weight gradients and their reduction.
 * Every launch is a later launch on the stream; no kernel waits on another and no tickets are used.  Precisions: 0 (f32), 3 (bf16x3)
 * and 4 (f16x2) run, through the launches the other phases use at that precision; 1 (bf16) and 2 (bf16x2) are refused by name.
 * Refused with MOBODY_E_ARG before any runtime call: d.N > 2^21, v_true != NULL, policy_ready != 0, such a precision, pi_out /
 * dpi_extra NULL, both or neither of grad_actor and m, v, null pointers. */
int mobody_bosa_actor_forward(const MobodyActor* a, float* pi_out /* [N][A] */, void* stream);
int mobody_bosa_actor_backward(const MobodyActor* a, const float* dpi_extra /* [N][A] */, void* stream);

/* ---- IQL baseline (the reference's algo/offline_offline/iql.py) -----------------------------------------------
 * One block type for the step's three calls, in the step's order; each call reads the fields named for it, `grad` / `m, v` /
 * `t` / `t_dev` / `lr` are those of the net the call trains (gradient form or fused form by the rule above).  Every row is
 * trained on (d.Nt is not read).  All nets are packed MLPs: V = mobody_mlp_layout(S, 1, 1), twin-Q = (S + A, 1, 2), the policy
 * = (S, 2 A, 1) whose first A outputs are mu and whose last A (logstd) take an exactly zero gradient.  The T blobs are read in
 * every precision (the backward streams them) and written by the fused forms.
 *   mobody_iql_value    iql.py:174-185, :217-220.  Forwards target-Q(s, a) and V(s) (one launch), then V's backward with the
 *                       expectile seed formed in its prologue: adv = min(Qt1, Qt2) - V, L_V = mean(|lam - 1[adv < 0]| adv^2).
 *                       Reads v_blob(_T), qtarg_blob(_T), state, action; writes adv[N], loss_out[0] = local share of L_V and,
 *                       when log_out != NULL, log_out[0] = sum adv / N_global, log_out[1] = sum V / N_global (train/adv, train/value).
 *   mobody_iql_critic   iql.py:187-196, :222-228.  V(s') with the updated V next to Q(s, a) (one launch), then mobody_critic's
 *                       backward and update with y = r + nd gamma V(s') (its q_next form): Adam on q_blob, Polyak on qtarg_blob.
 *                       Reads v_blob(_T), q_blob(_T), qtarg_blob(_T), state .. not_done, bump; loss_out[0] = L_Q.
 *   mobody_iql_actor    iql.py:91-95, :198-202, :233-237.  The policy forward (linear 2 A outputs), then its backward with the
 *                       advantage-weighted regression seed in the prologue: w = min(exp(temp adv), 100) from the adv of
 *                       mobody_iql_value (V before its update), L_pi = mean over N A of w (tanh(mu) - a)^2 -- no max_action.
 *                       Fused form: the Adam step runs at the cosine learning rate of gradient step k (t, or t_dev[0]),
 *                       lr (1 + cos(pi (k - 1) / T_max)) / 2, formed in double and rounded to fp32; with t_dev on the device.
 *                       The gradient form writes `grad` only (the caller steps with the scheduled rate).
 *                       Reads pi_blob(_T), state, action, adv; loss_out[0] = L_pi.
 * The same workspace (mobody_iql_workspace floats) for all three.
 * Refused with MOBODY_E_ARG before any runtime call, with the field named: 2 A > 128, lam outside (0, 1), T_max < 1 (actor).
 * (Declared as a tagged struct plus its typedef, as MobodyEnsEval.) */
typedef struct MobodyIql MobodyIql;
struct MobodyIql {
  int32_t struct_bytes;
  int32_t reserved;         /* 0 */
  MobodyTrainDims d;
  MobodyHyper h;            /* gamma, tau, precision are read */
  float lam, temp;
  int64_t T_max;
  float *v_blob, *v_blob_T, *q_blob, *q_blob_T, *qtarg_blob, *qtarg_blob_T, *pi_blob, *pi_blob_T;
  const float *state, *action, *next_state, *reward, *not_done;
  float* adv;
  float* grad;
  float *m, *v;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  int64_t* bump;            /* mobody_iql_critic, as MobodyCritic.bump */
  float *loss_out, *log_out, *workspace;
};
int64_t mobody_iql_workspace(const MobodyTrainDims* d);
int mobody_iql_value(const MobodyIql* a, void* stream);
int mobody_iql_critic(const MobodyIql* a, void* stream);
int mobody_iql_actor(const MobodyIql* a, void* stream);

/* Expectile loss of the V function (update_v_function, mobody.py:231-242): adv = min(qt[0],qt[1]) - v;
 * dz3[N][16] column 0 = dL_V/dV (1/N_global scaling), loss_out[0] = local share of L_V; lossp_ws: ceil(N/256) floats. */
int mobody_value_loss_grad(const float* qt, const float* v, int64_t N, int64_t N_global, float* dz3, float* loss_out,
                           float* lossp_ws, void* stream);

/* Adam (torch defaults b1=.9 b2=.999 eps=1e-8) on a packed blob (mobody_mlp_layout(in_dim, out_dim, members)); refreshes the
 * transposed blob used by the backward kernels. */
typedef struct MobodyAdam {
  int32_t struct_bytes, in_dim, out_dim, members;
  float *blob, *blob_T;     /* blob_T may be NULL */
  const float* grad;
  float *m, *v;
  float *target;            /* optional Polyak update target = tau*p + (1-tau)*target (tau < 0 or target == NULL: skip) */
  float *target_T;          /* nullable: T blob of the target net, whose W2 planes then follow the Polyak update */
  int64_t t;                /* 1-based step count */
  const int64_t* t_dev;     /* nullable: the step count is read from DEVICE memory (t_dev[0]) instead, so that a captured HIP
                               graph advances without new kernel arguments (bias corrections are formed in double on the device) */
  float lr, tau;
  float grad_scale;         /* multiplies the gradient first (1/world for an all-reduced SUM) */
  int32_t precision;        /* format of the W2 planes written into blob_T / target_T (the mode the nets are evaluated in) */
} MobodyAdam;
int mobody_adam_polyak(const MobodyAdam* a, void* stream);

/* PAR reward shaping: reward[i] -= coef * mean_d (next_state_true[i][d] - next_state_model[i][d])^2  (mobody.py:428-434) */
int mobody_par_penalty(const float* next_state_true, const float* next_state_model, float* reward, float coef,
                       int64_t n, int S, void* stream);

/* ---- generic gradient of one packed MLP + DARA classifier pieces (mobody.py:11-33,146-181,354-381) ---- */
/* grad (parameter-blob layout) from dz3[members][rows][Np3] and the activations mobody_mlp3_forward saved. */
int64_t mobody_mlp3_backward_workspace(int in_dim, int out_dim, int members, int64_t rows);
int mobody_mlp3_backward(const float* blob_T, int in_dim, int out_dim, int members, const float* dz3, const float* x,
                         const float* h1, const float* h2, int64_t rows, float* grad, float* workspace, void* stream);

/* Classifier inputs x_sas[N][2S+A] = [s,a,s'] + std*eps, x_sa[N][S+A] = [s,a] + std*eps' (eps explicit or device
 * Philox streams 4/5 at (seed, call); std = 0 -> no noise). */
int mobody_dara_inputs(const float* s, const float* a, const float* s2, int64_t N, int S, int A, float std,
                       const float* noise_sas, const float* noise_sa, uint32_t seed, uint32_t call, float* x_sas,
                       float* x_sa, void* stream);

/* loss_out = (loss_sa, loss_sas) = mean cross_entropy(softmax(logits), label) with the reference's double softmax;
 * dz_*[N][16] = d(loss)/d(logits) (columns 2..15 zero).  labels NULL -> rows < n_src are 0, the rest 1.
 * lossp_ws: 2*ceil(N/256) floats. */
int mobody_dara_loss_grad(const float* z_sas, const float* z_sa, const int32_t* labels, int64_t N, int64_t n_src,
                          float* dz_sas, float* dz_sa, float* loss_out, float* lossp_ws, void* stream);

/* delta = clamp(log p~_sas[1] - log p~_sa[1] - log p~_sas[0] + log p~_sa[0], -10, 10), p~ = softmax(softmax(logits)) + 1e-10;
 * reward[i] += coef * delta (reward may be NULL), delta_out optional. */
int mobody_dara_penalty(const float* z_sas, const float* z_sa, int64_t n, float coef, float* reward, float* delta_out,
                        void* stream);

/* ---- DARA baseline (the reference's algo/offline_offline/dara.py) ---------------------------------------------
 * DARA's step is IQL's (the three mobody_iql_* calls above, same nets and blocks) behind two additions, each one call on the
 * block below.  The classifier's two heads are packed MLPs: sa = mobody_mlp_layout(S + A, 2, 1), sas = (2 S + A, 2, 1); their T
 * blobs are read in every precision and written by the fused form.  Rows are [src | tar]: rows < n_src carry label 0, the rest
 * label 1 (n_src = 0 means d.N / 2; the reference's randperm of the rows is dropped: the loss is a mean over rows).
 *   mobody_dara_classifier  dara.py:131-144, :202-223.  One classifier update on d.N rows: x_sas = [s | a | s'] + noise_std eps,
 *                       x_sa = [s | a] + noise_std eps' (eps explicit unit normals noise_sas / noise_sa, or the device generator's
 *                       streams 4 / 5 at (seed, call) -- with call_dev != NULL at call id call_dev[0] + call_offset), both heads'
 *                       forwards in one launch at `precision`, per head the backward with the loss seed formed in its prologue
 *                       (cross_entropy applied to the head's softmax PROBABILITIES, as the reference does) and the weight
 *                       gradients.  Gradient form: grad_sa and grad_sas are written.  Fused form (m_*, v_* given): ONE Adam
 *                       over both heads, one step count t (or t_dev[0]) at rate lr.  loss_out[0] = loss_sa, [1] = loss_sas
 *                       (local share, scaled by 1 / N_global).
 *   mobody_dara_relabel     dara.py:281-292.  Noise-free pass of both heads on the first n_src rows of state | action | next_state
 *                       (read in place), penalty = clamp(log p~_sas[1] - log p~_sa[1] - log p~_sas[0] + log p~_sa[0], -10, 10),
 *                       p~ = softmax(head probabilities) + 1e-10 (mobody_dara_penalty's arithmetic); reward[row] += eta * penalty
 *                       for row < n_src (eta == 0: no reward is written), delta_out[row] = penalty and log_out[0] = its mean when
 *                       given.  Rows >= n_src are not touched.
 * Both take mobody_dara_workspace floats: mobody_iql_workspace's, which the IQL calls of the step use, with the classifier's
 * scratch behind them.  Refused with MOBODY_E_ARG before any runtime call, with the field named: 2 A > 128, 2 S + A > 256, N odd
 * without n_src, n_src outside [0, N], precision, null pointers, both or neither of the gradient blobs and the optimizer state. */
typedef struct MobodyDara MobodyDara;
struct MobodyDara {
  int32_t struct_bytes;
  int32_t precision;
  MobodyTrainDims d;
  int64_t n_src;
  float *sa_blob, *sa_blob_T, *sas_blob, *sas_blob_T;
  const float *state, *action, *next_state;
  float* reward;
  const float *noise_sas, *noise_sa;
  float noise_std, eta;
  uint32_t seed, call;
  const int64_t* call_dev;
  int64_t call_offset;
  float *grad_sa, *grad_sas;
  float *m_sa, *v_sa, *m_sas, *v_sas;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  int32_t reserved;
  float *delta_out, *loss_out, *log_out, *workspace;
};
int64_t mobody_dara_workspace(const MobodyTrainDims* d);
int mobody_dara_classifier(const MobodyDara* a, void* stream);
int mobody_dara_relabel(const MobodyDara* a, void* stream);

/* ---- IGDF baseline (the reference's algo/offline_offline/igdf.py) ---------------------------------------------
 * IGDF's step is IQL's behind a data filter: two contrastive encoders score the source rows, the k best are kept, and the critic
 * loss is row-weighted.  The encoders are packed MLPs with linear outputs: sa = mobody_mlp_layout(S + A, Z, 1), ss = (S, Z, 1),
 * Z = repr_dim <= 128; their T blobs are read in every precision and written by the fused form.  Row-wise pieces, callable alone:
 *   mobody_igdf_contrast  igdf.py:427-440.  The in-batch contrastive loss on n rows: logits l[i][0] = phi_i . psi_tar_i,
 *                       l[i][j] = phi_i . psi_src_{j-1} (j = 1 .. n-1), binary cross-entropy against a 1 in column 0 in the stable
 *                       form max(l, 0) - l y + log1p(exp(-|l|)), mean over n^2.  phi [n][ldz], psi_tar [n][ldz], psi_src
 *                       [n-1][ldz]: columns >= Z are never read.  Writes loss_out[0], dz3_sa [n][Np3] = dL/dphi and dz3_ss
 *                       [2n-1][Np3] = dL/dpsi (tar rows, then src rows), Np3 = round_up(Z, 16), columns >= Z zero.  The n x n
 *                       logits never reach memory; all sums run in a fixed order (no float atomics): two runs give the same
 *                       bits.  lossp: ceil(n / 32) floats of scratch.  2 <= n <= 4096, 1 <= Z <= 128, ldz >= Z.
 *   mobody_igdf_select    igdf.py:505-508, :515.  kept[k] = positions of the k largest of score[n] in ascending order
 *                       (argsort(score)[-k:]), w[k] = exp(importance_weight * score[kept]).  The order is total for every bit
 *                       pattern: an integer key of the float, ties to the lower index first, a non-finite score below every finite
 *                       one (-0 below +0): the ranks are always a permutation.  1 <= k <= n <= 4096.
 * and the calls on the block below:
 *   mobody_igdf_info      igdf.py:418-447.  One contrastive update: both encoders' forwards in one launch (sa on the n rows
 *                       state | action, ss on the 2n-1 rows of next_state = [tar s' (n) | src s' (n-1)]), mobody_igdf_contrast,
 *                       then per encoder the backward (dz3 from memory) and the weight gradients.  Gradient form: grad_sa, grad_ss
 *                       are written.  Fused form (m_*, v_* given): ONE Adam over both encoders, one step count t (or t_dev[0])
 *                       at rate lr; bump (fused form, or NULL): a device word the last optimizer launch increments.
 *                       loss_out[0] = the loss.
 *   mobody_igdf_filter    igdf.py:494-524.  Both encoders' forwards (one launch) on the first n rows of the staged batch state |
 *                       action | next_state (read in place, rows [src(n) | tar(d.N - k)]), score_i = phi_i . psi_i / (|phi_i|
 *                       |psi_i|) over the Z real columns (no epsilon), mobody_igdf_select, then the training batch out_* =
 *                       [kept src rows | tar rows], d.N = k + n_tar rows, and row_weight[d.N] = w on the kept rows, 1 on the
 *                       target rows.  Optional: score_out[n], kept_out[k].  The staged batch is not modified.
 *   mobody_igdf_critic    igdf.py:468-479.  mobody_iql_critic with the critic loss mean(w (q1 - y)^2) + mean(w (q2 - y)^2):
 *                       dz3 = 2 w (q_m - y) / N_global.  row_weight NULL: mobody_iql_critic, bit for bit.
 * mobody_igdf_workspace(d, n, Z) floats: mobody_iql_workspace(d)'s in front (the IQL calls of the step use the same tensor), the
 * encoders' scratch for n (sa) and 2n-1 (ss) rows behind.  Refused with MOBODY_E_ARG before any runtime call, with the field
 * named: n outside [2, 4096], Z outside [1, 128], k outside [1, n], d.N < k (filter), 2 A > 128, precision, null pointers, both
 * or neither of the gradient blobs and the optimizer state. */
typedef struct MobodyIgdf MobodyIgdf;
struct MobodyIgdf {
  int32_t struct_bytes;
  int32_t precision;
  MobodyTrainDims d;
  int64_t n, k;
  int32_t Z;
  float importance_weight;
  float *sa_blob, *sa_blob_T, *ss_blob, *ss_blob_T;
  const float *state, *action, *next_state, *reward, *not_done;
  float *out_state, *out_action, *out_next_state, *out_reward, *out_not_done, *row_weight;
  float* score_out;
  int32_t* kept_out;
  float *grad_sa, *grad_ss;
  float *m_sa, *v_sa, *m_ss, *v_ss;
  int64_t t;
  const int64_t* t_dev;
  int64_t* bump;
  float lr;
  int32_t reserved;
  float *loss_out, *workspace;
};
int64_t mobody_igdf_workspace(const MobodyTrainDims* d, int64_t n, int32_t Z);
int mobody_igdf_contrast(const float* phi, const float* psi_tar, const float* psi_src, int64_t n, int32_t Z, int32_t ldz,
                         float* dz3_sa, float* dz3_ss, float* lossp, float* loss_out, void* stream);
int mobody_igdf_select(const float* score, int64_t n, int64_t k, float importance_weight, int32_t* kept, float* w, void* stream);
int mobody_igdf_info(const MobodyIgdf* a, void* stream);
int mobody_igdf_filter(const MobodyIgdf* a, void* stream);
int mobody_igdf_critic(const MobodyIql* a, const float* row_weight, void* stream);

/* ---- dynamics pre-training (MOBODYEnsembleDynamics.learn / validate, algo/dynamics/mobody_dynamics.py:300-384,
 *      594-653, 1113-1140; Swish/reparameterisation mobody_module.py:9-15,237-243) ----------------------------------
 * All trained parameters of the 7-member ensemble live in ONE blob: three MobodyMlpLayout regions with 7 members
 * (state encoder zs1-3: S -> 256 -> 256 -> 32 = mu | logvar; decoder transition1-3: 16 -> 256 -> 256 -> S; reward head
 * reward_model1-3: 2S+A -> 256 -> 256 -> 2) and the two action encoders (za_src*, za_trg*), per member
 * W1[16+A][32] b1[32] W2[32][16] b2[16] row major (only the mu half of za_*2 takes part in the loss).  Gradients and
 * both Adam moments use the same layout; the T blob holds the three regions' transposes. */
typedef struct MobodyPretrainLayout {
  int32_t S, A, za_in, _pad;
  MobodyMlpLayout enc, tr, rw;
  int64_t off_enc, off_tr, off_rw, off_za_src, off_za_trg;    /* float offsets inside the parameter blob */
  int64_t za_w1, za_b1, za_w2, za_b2, za_member_floats;       /* inside one member of an action encoder */
  int64_t total_floats;
  int64_t t_off_enc, t_off_tr, t_off_rw, t_total_floats;      /* T blob */
} MobodyPretrainLayout;
int mobody_pretrain_layout(int S, int A, MobodyPretrainLayout* out);
/* `precision` of the pre-training entry points: 0 = exact fp32 MFMA, 4 = "f16x2" (the 256 x 256 layers of the three
 * 7-member nets on the split core, h1 / dz2 handed to the weight-gradient GEMM as fp16 planes; other modes are refused).
 * The T blob carries the W2 / W2^T planes of the mode it was built for; Adam keeps them current. */
int mobody_pretrain_transpose(int S, int A, const float* blob, float* blob_T, int precision, void* stream);
int64_t mobody_pretrain_workspace(int S, int A, int64_t b);

/* Bootstrap gather of one batch (learn() slices train_obss[:, k*bs:(k+1)*bs] of the per-member bootstrapped arrays,
 * :604-612): member e takes dataset rows idx[e][start + r], r < b.  idx is a DEVICE int32 [7][n_idx] matrix.
 * Outputs: xenc[7][2b][S] (s rows, then s' rows), act[7][b][A], rew[7][b]. */
int mobody_pretrain_gather(const float* state, const float* action, const float* next_state, const float* reward,
                           const int32_t* idx, int64_t n_idx, int64_t start, const int64_t* start_dev, int64_t b, int S,
                           int A, float* xenc, float* act, float* rew, void* stream);
/* start_dev (nullable): DEVICE int64 batch counter, start += start_dev[0] * b, so a captured graph walks the index matrix
 * batch by batch (advance it with mobody_counter_add); reads are clamped to the matrix. */

/* Loss and gradients of one learn() batch (zero_grad + loss.backward, :594-642), arguments by name; gradient-only or fused by
 * the fields, as the train-step blocks above (exactly one of `grad` and m, v).
 *   grad given   every float of `grad` (blob layout) is written, layout padding (W1 rows >= in_dim, W3 / b3 columns >= out_dim
 *                of the three regions) as exactly 0 -- except the action encoder that is not used this step (za_trg* on source
 *                batches, za_src* on target ones), which is left untouched.  SUM all-reduce it before mobody_pretrain_adam.
 *   m, v given   single-GPU form of this call + mobody_pretrain_adam: every gradient reduction applies the Adam step of the
 *                elements it has just reduced (no gradient blob, four launches fewer).  Needs b_global == b.
 * The workspace needs no initialisation: the results do not depend on what it held. */
typedef struct MobodyPretrain {
  int32_t struct_bytes, S, A, use_trg;
  int64_t b;                /* rows per member on this rank */
  int64_t b_global;         /* rows per member over all data-parallel ranks (gradients / losses are local shares of the global
                               means) */
  float encoder_loss_coef;
  float transition_coef, reward_coef;
                            /* weights of transition_loss and reward_loss in this call's loss (1, 1 = learn()).
                               inverse_sep_reward_loss = 1 runs learn() with reward_coef 0 and learn_sep_reward (:482-519) with
                               encoder_loss_coef 0, transition_coef 0, reward_coef 1 */
  int32_t precision;
  float *blob, *blob_T;     /* written by the fused form only */
  const float *xenc, *act, *rew;   /* as mobody_pretrain_gather writes them */
  const float *noise6;      /* [6][7][b][16] = the six reparameterisation draws in the reference's order z1(s) z2(s') z3(s) z4(s')
                               z5(s) z6(s) */
  const float *noise7;      /* [7][b][S] = the fake-next-state draw; NULL (either) -> device Philox streams 16..22 at (seed, call) */
  uint32_t seed, call;
  const int64_t* call_dev;  /* nullable: DEVICE int64 word added to `call` (graph replay) */
  float* grad;
  float *m, *v;
  int64_t t_main, t_za;     /* 1-based step counts of the three MLP regions / of this step's action encoder */
  const int64_t* t_dev;     /* nullable: DEVICE int64[2] = {t_main, t_za} read instead of the host counts (graph replay) */
  float lr;
  float *loss_out;          /* [5] = (loss, transition_loss, encoder_loss, recon_loss, kl_loss) */
  float *loss_acc;          /* nullable: DEVICE float[5], loss_acc += loss_out in the step's last launch (learn()'s running sums,
                               :630-650) */
  float *workspace;
} MobodyPretrain;
int mobody_pretrain(const MobodyPretrain* a, void* stream);

/* torch.optim.Adam step on the blob (and its T blob): the three MLP regions use the 1-based step count t_main, the
 * action encoder of this step's domain t_za; the other action encoder is skipped (its .grad is None in the reference,
 * so its Adam state does not advance). */
int mobody_pretrain_adam(int S, int A, int use_trg, float* blob, float* blob_T, const float* grad, float* m, float* v,
                         int64_t t_main, int64_t t_za, float lr, float grad_scale, int precision, int net_mask, int64_t t_rw,
                         void* stream);
/* net_mask: bit 0 state encoder, bit 1 decoder, bit 2 reward head -- a net without a gradient in this step is skipped and
 * keeps its step count (7 and t_rw = t_main: every net, one count -- learn()); the reward head steps with its own t_rw. */

/* Adam step of ONE action encoder only (blob layout, its own 1-based step count): the second encoder of a learn_src_trg step
 * (config train_together = 1, :521-590 -- the summed source + target loss moves both, mobody_pretrain_adam steps one). */
int mobody_pretrain_za_adam(int S, int A, int use_trg, float* blob, const float* grad, float* m, float* v, int64_t t_za,
                            float lr, float grad_scale, void* stream);

/* validate() (:1113-1140) on an inference blob (mobody_dyn_layout): out[0..6] = per-member mean_{b,d}(mean_e - s')^2,
 * out[7..13] = per-member mean_b (r_mu_e(s, a, mean_e) - r)^2.  Workspace floats: mobody_dyn_validate_workspace. */
int64_t mobody_dyn_validate_workspace(int S, int A, int64_t B);
int mobody_dyn_validate(const float* dyn_blob, int S, int A, const float* obs, const float* act, const float* next_obs,
                        const float* rew, int64_t B, int use_trg, float* out, float* workspace, void* stream);

/* ---- dynamics pre-training of the MOPO ablation (config mopo = 1: mean_e = s + MLP_e([s, a]), mobody_module.py:114-118,
 *      133-137,218-219,251-254,264-266; learn() / validate() as above) ----------------------------------------------------
 * ONE parameter blob: the 7-member MLP za_src1-3 (S+A -> 256 -> 256 -> S) in mobody_mlp_layout(S + A, S, 7) format at off_dyn
 * (the format of the inference path's mopo blob), then the reward head reward_model1-3 (2S+A -> 256 -> 256 -> 2) at off_rw.
 * Both domains train the same MLP (encode_trg_action delegates to encode_src_action); za_trg*, zs*, transition* and za_de_*
 * take no part.  Gradients and both Adam moments use the same layout, the T blob holds the two regions' transposes. */
typedef struct MobodyPretrainMopoLayout {
  int32_t S, A, _pad0, _pad1;
  MobodyMlpLayout dyn, rw;
  int64_t off_dyn, off_rw, total_floats;          /* float offsets inside the parameter blob */
  int64_t t_off_dyn, t_off_rw, t_total_floats;    /* T blob */
} MobodyPretrainMopoLayout;
int mobody_pretrain_mopo_layout(int S, int A, MobodyPretrainMopoLayout* out);
/* precision 0 (exact fp32) or 4 (f16x2), as for the latent entry points above */
int mobody_pretrain_mopo_transpose(int S, int A, const float* blob, float* blob_T, int precision, void* stream);
int64_t mobody_pretrain_mopo_workspace(int S, int A, int64_t b);
/* Loss and gradients of one learn() batch of the mopo model, arguments by name: the fields of MobodyPretrain with the same
 * meanings (gradient-only or fused likewise), except
 *   noise   [7][b][S] = the fake-next-state draw (NULL -> device Philox stream 22 at (seed, call))
 *   t       the 1-based step count shared by both regions; t_dev (nullable): DEVICE int64 read instead of t
 * loss_out[5] = (loss, transition_loss, encoder_loss, recon_loss = 0, kl_loss). */
typedef struct MobodyPretrainMopo {
  int32_t struct_bytes, S, A, use_trg;
  int64_t b, b_global;
  float encoder_loss_coef;
  int32_t precision;
  float *blob, *blob_T;
  const float *xenc, *act, *rew, *noise;
  uint32_t seed, call;
  const int64_t* call_dev;
  float* grad;
  float *m, *v;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  float *loss_out, *loss_acc, *workspace;
} MobodyPretrainMopo;
int mobody_pretrain_mopo(const MobodyPretrainMopo* a, void* stream);
/* torch.optim.Adam step of both regions with the one step count t (every learn() step gives both a gradient). */
int mobody_pretrain_mopo_adam(int S, int A, float* blob, float* blob_T, const float* grad, float* m, float* v, int64_t t,
                              float lr, float grad_scale, int precision, void* stream);
/* validate() of a mopo model: the reward head from the inference blob (mobody_dyn_layout), the MLP from the mopo blob
 * (mobody_mlp_layout(S + A, S, 7)); outputs and workspace as mobody_dyn_validate. */
int mobody_dyn_validate_mopo(const float* dyn_blob, const float* mopo_blob, int S, int A, const float* obs, const float* act,
                             const float* next_obs, const float* rew, int64_t B, float* out, float* workspace, void* stream);

/* (Re)build the transposed blob from a parameter blob (after loading a checkpoint); `precision` selects the format of
 * the W2 / W2^T planes it writes (the mode the net will be evaluated in). */
int mobody_mlp_transpose(int in_dim, int out_dim, int members, const float* blob, float* blob_T, int precision,
                         void* stream);

/* ---- packed MLPs of any hidden width (BOSA's VAE nets, the reference's algo/offline_offline/bosa.py) ----------
 * in_dim -> hidden -> hidden -> out_dim, ReLU on both hidden layers, `members` independent copies: the shape of the policy
 * VAE's encoder / decoder (bosa.py:28-47, one member) and of the dynamics VAE's EnsembleFC stacks (bosa.py:176-200, :208-236).
 * 1 <= in_dim <= 256, 8 <= hidden <= 1024, 1 <= out_dim <= 256, 1 <= members <= 8.  Parameter blob, per member, all row major:
 * W1[Kp1][Hp] b1[Hp] W2[Hp][Hp] b2[Hp] W3[Hp][Np3] b3[Np3] (W stored [in][out]), Kp1 = round_up(in_dim, 16),
 * Hp = round_up(hidden, 32), Np3 = round_up(out_dim, 32).  Padding is zero and stays zero through training: a padded hidden
 * unit has pre-activation 0, so its ReLU mask and with it every gradient entry of the padding is exactly 0, and Adam maps a
 * zero gradient with m = v = 0 to a zero update.  Gradients and both Adam moments use the same layout.  The wide nets run in
 * exact fp32 (v_mfma_f32_32x32x2_f32) only: a `precision` other than 0 is MOBODY_E_ARG. */
typedef struct MobodyWideLayout {
  int32_t in_dim, hidden, out_dim, members, Kp1, Hp, Np3, _pad;
  int64_t w1, b1, w2, b2, w3, b3;   /* float offsets inside one member */
  int64_t member_floats, total_floats;
} MobodyWideLayout;
int mobody_wide_layout(int in_dim, int hidden, int out_dim, int members, MobodyWideLayout* out);

enum { MOBODY_WIDE_OUT_RAW = 0, MOBODY_WIDE_OUT_TANH = 1 };

/*   mobody_wide_mlp3_forward   bosa.py:49-70, :238-255 (the nn.Sequential / EnsembleFC stacks).  out[members][rows][out_dim] =
 *                       layer3(relu(layer2(relu(layer1(x))))), raw or max_action * tanh.  x = [src0 | src1 | src2] row by row;
 *                       source i is [rows][src_width_i] row major, member e's copy src_member_stride_i floats behind member
 *                       e-1's (0: every member reads the same rows); a width of 0 drops the source; the widths add up to in_dim.
 *                       src_rows_i (0: `rows`): the source holds that many rows and row r of x reads its row r % src_rows_i (the
 *                       estimator's decoder runs num_samples copies of the batch against one copy of the states).
 *                       x_shared = 1 when every used source has stride 0, else 0 (checked).  Saves (each nullable): save_x
 *                       [x_shared ? 1 : members][rows][Kp1], save_h1 and save_h2 [members][rows][Hp], padding columns zero; what
 *                       is not saved lives in `workspace` (mobody_wide_mlp3_forward_workspace floats; NULL when all three saves
 *                       are given).  Four launches: the concatenation, one product per layer with its bias / activation folded in. */
typedef struct MobodyWideFwd MobodyWideFwd;
struct MobodyWideFwd {
  int32_t struct_bytes;
  int32_t precision;
  MobodyWideLayout layout;
  const float* blob;
  const float *src0, *src1, *src2;
  int32_t src_width0, src_width1, src_width2, x_shared;
  int64_t src_member_stride0, src_member_stride1, src_member_stride2;
  int64_t src_rows0, src_rows1, src_rows2;
  int64_t rows;
  int32_t out_mode;
  float max_action;
  float *out, *save_x, *save_h1, *save_h2, *workspace;
};
int64_t mobody_wide_mlp3_forward_workspace(const MobodyWideLayout* L, int64_t rows);
int mobody_wide_mlp3_forward(const MobodyWideFwd* a, void* stream);

/*   mobody_wide_mlp3_backward  what loss.backward() does to such a stack (bosa.py:525, :545).  From dz3[members][rows][out_dim] (the
 *                       gradient of the loss with respect to the last layer's pre-activation output; for the tanh output mode the
 *                       caller folds the tanh's derivative in) and the forward's saves x, h1, h2 it writes the parameter gradient
 *                       `grad` in blob layout, padding included (zeros), and -- dx != NULL -- dx[members][rows][dx_col1 - dx_col0],
 *                       the gradient with respect to columns [dx_col0, dx_col1) of x.  Every sum over rows runs inside one
 *                       workgroup in ascending row order, no float atomics: two runs give the same bits.  workspace:
 *                       mobody_wide_mlp3_backward_workspace floats.  Six launches, seven with dx: three weight gradients, two
 *                       masked input gradients, the three bias gradients in one. */
typedef struct MobodyWideBwd MobodyWideBwd;
struct MobodyWideBwd {
  int32_t struct_bytes;
  int32_t precision;
  MobodyWideLayout layout;
  const float* blob;
  const float *dz3, *x, *h1, *h2;
  int32_t x_shared, reserved;
  int64_t rows;
  float* grad;
  float* dx;
  int32_t dx_col0, dx_col1;
  float* workspace;
};
int64_t mobody_wide_mlp3_backward_workspace(const MobodyWideLayout* L, int64_t rows);
int mobody_wide_mlp3_backward(const MobodyWideBwd* a, void* stream);
/*   mobody_wide_mlp3_input_grad  the same block with grad == NULL and dx != NULL: dx alone, for a net whose parameters are held fixed
 *                       (the estimator's gradient, bosa.py:615-619, differentiates through the frozen VAE).  Three launches -- dz2,
 *                       dz1 and dx[:, dx_col0:dx_col1], the products mobody_wide_mlp3_backward issues, in its order -- so dx has the
 *                       bits of the full backward's dx.  x is not read.  The same workspace entry.  Refused as its sibling refuses,
 *                       and additionally: grad given, dx missing. */
int mobody_wide_mlp3_input_grad(const MobodyWideBwd* a, void* stream);

/*   mobody_wide_adam          torch.optim.Adam(lr) with torch's defaults (bosa.py:424-425) on n floats of a flat blob -- one
 *                       wide net or several laid end to end -- from a gradient of the same layout.  t is the 1-based step count;
 *                       t_dev (nullable): a DEVICE int64 read instead, so that a captured graph advances.  One launch. */
typedef struct MobodyWideAdam MobodyWideAdam;
struct MobodyWideAdam {
  int32_t struct_bytes;
  int32_t reserved;
  float* blob;
  const float* grad;
  float *m, *v;
  int64_t n;
  int64_t t;
  const int64_t* t_dev;
  float lr;
  int32_t reserved1;
};
int mobody_wide_adam(const MobodyWideAdam* a, void* stream);

/* ---- BOSA's VAE stage (bosa.py:23-133, :203-327, :516-550) ----------------------------------------------------
 * Both VAEs are two wide nets each, the encoder's blob directly followed by the decoder's in ONE tensor (gradient and Adam
 * moments alike), with Lz the latent width:
 *   kind MOBODY_BOSA_POLICY    members = 1, Lz = 2 A; encoder mobody_wide_layout(S + A, hidden, 2 Lz, 1) on [s | a];
 *                              decoder (S + Lz, hidden, A, 1) on [s | z], output max_action * tanh
 *   kind MOBODY_BOSA_DYNAMICS  members = E, Lz = 2 S; encoder (2 S + A, hidden, 2 Lz, E) on [s | a | s'], the same rows for
 *                              every member; decoder (S + A + Lz, hidden, S, E) on [s | a | z_e], linear output
 * Columns [0, Lz) of the encoder's output are the `mean` head, [Lz, 2 Lz) the `log_std` head.
 *   mobody_bosa_reparam   bosa.py:116-117, :68, :521 (and :309-310, :253, :539), the row-wise piece, callable alone.  enc
 *                       [n][2 Lz] (n = members * B rows), eps [n][Lz].  log_std = clamp(., -4, 15), std = exp, z = mean + std *
 *                       eps -> z [n][Lz]; kl_out[0] = -0.5 mean(1 + log(std^2) - mean^2 - std^2) over the n Lz elements.  With
 *                       dz != NULL ([n][Lz], dLoss/dz) it also writes denc [n][2 Lz], the gradient of
 *                       (the loss behind dz) + beta * KL with respect to enc: the clamp passes gradient where -4 <= x <= 15, both
 *                       ends inclusive, as torch's does.  Fixed summation order.  lossp: ceil(n Lz / 256) floats of scratch.
 *   mobody_bosa_vae       bosa.py:516-550.  One training step of the VAE `kind` on B rows: encoder forward, the
 *                       reparameterisation, decoder forward, recon = mean((u - target)^2) over all elements (the member axis
 *                       included; target = action | next_state), KL as above, loss = recon + beta * KL, both backwards into
 *                       `grad` (always written, blob layout), and -- m, v given -- one Adam over both nets with the step count t
 *                       (or t_dev[0]) at rate lr.  eps [members][B][Lz], or NULL: element i is drawn from the device generator,
 *                       stream MOBODY_BOSA_STREAM_POLICY / _DYNAMICS, call `call` + (call_dev ? call_dev[0] : 0).
 *                       loss_out = (recon, KL, loss).  26 launches (25 without Adam).
 *   mobody_bosa_loglik    bosa.py:72-105, :257-298.  The importance-sampling estimator, forward only, n = num_samples in [1, 64]:
 *                       encode, draw n latents per row (and member), decode the n B rows, w = sum log N(x; dec, sqrt(beta / 4)) +
 *                       sum log N(z; 0, 1) - sum log N(z; mean, std), ll = logsumexp_n(w) - log n with the maximum subtracted.
 *                       ll [members][B]; dynamics only: min_ll [B] = min over members, mask [B] = (min_ll > log_eps) as 0 / 1,
 *                       mask_mean [1] (each nullable).  A NaN ll of any member makes the row's min_ll NaN and its mask 0, as
 *                       torch.min and the comparison do (:585-590): the minimum does not skip a NaN member.  w_out (nullable)
 *                       [members][n][B].  eps: the reference's layouts, [B][n][Lz]
 *                       (policy) / [n][members][B][Lz] (dynamics), or NULL: drawn at that linear index from stream
 *                       MOBODY_BOSA_STREAM_POLICY_LL / _DYNAMICS_LL.  Forward only: grad, m, v must be NULL; t, t_dev, lr and
 *                       loss_out are not read.  10 launches, 11 with mask_mean.
 *   mobody_bosa_loglik_grad  bosa.py:615-619: the policy VAE's estimator AND its derivative with respect to the action,
 *                       what autograd gives the actor loss's neg_log_beta term per row; kind MOBODY_BOSA_DYNAMICS is refused (that
 *                       estimator only runs under no_grad, :583-590).  a->action is the point of evaluation (the class passes
 *                       pi(s)).  ll and w_out are written by mobody_bosa_loglik itself, eps follows its rules (NULL: stream
 *                       MOBODY_BOSA_STREAM_POLICY_LL at `call`).  dll_da[b][j] = d ll[b] / d action[b][j] with the VAE's parameters
 *                       and eps held fixed: with p_k = softmax_k(w_k) and var = beta / 4, the direct term -sum_k p_k (a - u_k) / var,
 *                       plus the encoder's input gradient over columns [S, S + A) of the seed [sum_k g_k | pass (sum_k g_k eps_k std
 *                       + 1)], g_k = dz_k - p_k z_k, dz_k the decoder's latent input gradient of p_k (a - u_k) / var * max_action
 *                       (1 - (u_k / max_action)^2) on row k B + b; `pass` is mobody_bosa_reparam's inclusive clamp test.  The
 *                       estimator's launches, then 9: two row-wise kernels, mobody_wide_mlp3_input_grad on the decoder (n B rows)
 *                       and on the encoder, the final sum.  Later launches on one stream; no kernel waits on another; every loop is
 *                       bounded by an argument; fixed summation order, no float atomics.  workspace:
 *                       mobody_bosa_loglik_grad_workspace floats (mobody_bosa_workspace's pieces first, then the seed, dz and
 *                       backward scratch on n B rows); -1 for a bad block.  Refused as mobody_bosa_loglik refuses, and: kind,
 *                       dll_da NULL.
 * mobody_bosa_workspace(a) floats serve both calls on the block (for mobody_bosa_loglik with its num_samples).  Refused with
 * MOBODY_E_ARG before any runtime call, with the field named: kind, members != 1 for the policy VAE, a net outside
 * mobody_wide_layout's ranges, precision != 0, B < 1, beta <= 0, num_samples outside [1, 64], one of m, v without the other,
 * null pointers. */
enum { MOBODY_BOSA_POLICY = 0, MOBODY_BOSA_DYNAMICS = 1 };
enum { MOBODY_BOSA_STREAM_POLICY = 6, MOBODY_BOSA_STREAM_DYNAMICS = 7, MOBODY_BOSA_STREAM_POLICY_LL = 8, MOBODY_BOSA_STREAM_DYNAMICS_LL = 9,
       MOBODY_BOSA_STREAM_TARGET_NOISE = 10 /* the second stage's target noise [N][A] (bosa.py:571), drawn by the host class with mobody_rng_normal, or inside mobody_bosa_target */ };
typedef struct MobodyBosaVae MobodyBosaVae;
struct MobodyBosaVae {
  int32_t struct_bytes;
  int32_t kind;
  int32_t S, A, hidden, members;
  int32_t precision, num_samples;
  int64_t B;
  float beta, max_action;
  float* blob;
  const float *state, *action, *next_state;
  const float* eps;
  uint32_t seed, call;
  const int64_t* call_dev;
  float* grad;
  float *m, *v;
  int64_t t;
  const int64_t* t_dev;
  float lr, log_eps;
  float* loss_out;
  float *ll, *min_ll, *mask, *mask_mean, *w_out;
  float* workspace;
};
int64_t mobody_bosa_workspace(const MobodyBosaVae* a);
int mobody_bosa_reparam(const float* enc, const float* eps, const float* dz, int64_t n, int32_t Lz, float beta, float* z,
                        float* denc, float* lossp, float* kl_out, void* stream);
int mobody_bosa_vae(const MobodyBosaVae* a, void* stream);
int mobody_bosa_loglik(const MobodyBosaVae* a, void* stream);
int64_t mobody_bosa_loglik_grad_workspace(const MobodyBosaVae* a);
int mobody_bosa_loglik_grad(const MobodyBosaVae* a, float* dll_da /* [B][A] */, void* stream);
/*   mobody_bosa_critic    bosa.py:580-607: the twin-Q update of BOSA's second stage on a MobodyCritic block whose q_next
 *                       [N] the caller supplies (min target-Q(s', a') with its clipped target noise); phase, gather and
 *                       policy_forward must be 0 / NULL, the actor and target blobs are not read.  Q(s, a) with saves, then the
 *                       backward seeded with dz3[m][row][0] = 2 w (q_m - y) / N_global + c, w = row_weight[row], c = row_const[row]
 *                       (seed mode 9; c == 0 gives mobody_igdf_critic's seed bit for bit), the weight gradients and -- m, v given --
 *                       Adam, WITHOUT a Polyak update.  BOSA: w = mask / 2, c = conservation_coef / batch_size on the source rows
 *                       and 0 on the target rows.  loss_out[1] = sum over members and the rows with c != 0 of q_m, divided by
 *                       cons_rows_global (src_q1.mean() + src_q2.mean()); loss_out[0] = sum_m sum_rows w (q_m - y)^2 / N_global +
 *                       cons_coef * loss_out[1] (critic_loss; critic_td_loss is the difference).  workspace:
 *                       mobody_train_workspace floats. */
int mobody_bosa_critic(const MobodyCritic* a, const float* row_weight, const float* row_const, float cons_coef,
                       int64_t cons_rows_global, void* stream);

/* ---- BOSA's critic / actor stage without a torch op (bosa.py:565-634) -------------------------------------------
 * The row-wise pieces that sit between the stage's launches, so that a stage-2 call is a sequence of this library's launches
 * alone and can be captured as a HIP graph.  The new kernels use no flags, no tickets and no atomics (float or integer); each launch
 * reads what an earlier launch on the stream wrote and nothing waits inside a kernel; every loop is bounded by an argument (N, A,
 * nbump, the fixed grid); every sum and maximum runs in a fixed order, so two runs give the same bits.
 *   mobody_bosa_target    bosa.py:570-577: q_next [N] = min over the two target critics of Q_target(s', a') with
 *                       a' = clamp(pi_target(s') + clamp(noise * expl_noise, -noise_clip, noise_clip), -max_action, max_action).
 *                       Four launches, in order: mobody_mlp3_forward of the target actor (out_mode 1, max_action);
 *                       k_bosa_target_action, in place over pi; mobody_mlp3_forward of the two-member target critic on [s' | a'];
 *                       k_bosa_qnext.  noise [N][A], or NULL: element i is rng.h's unit normal (the one mobody_rng_normal writes at
 *                       index i) of (seed, stream MOBODY_BOSA_STREAM_TARGET_NOISE, call + (call_dev ? call_dev[0] : 0)).  The four
 *                       steps of a' are one correctly rounded fp32 operation each (multiply, clamp, add, clamp; nothing is
 *                       contracted); both clamps keep a NaN, as torch.clamp does; the minimum does not skip a NaN member, as
 *                       torch.min and mobody_bosa_loglik's min_ll do not.  The packed forwards' ReLU (fmaxf) turns a NaN
 *                       pre-activation into 0, so k_bosa_qnext also reads the row's s' and a' and gives a row with a NaN among
 *                       them q_next = NaN, as torch's forward would; no other row is touched.  On finite rows the result has the bits of mobody_rng_normal + torch's
 *                       mul / clamp / add / clamp + mobody_mlp3_forward + torch.min at precisions 0 (f32), 3 (bf16x3) and 4 (f16x2);
 *                       1 (bf16) and 2 (bf16x2) are refused by name, as the rest of the stage refuses them.  actor_blob_T / q_blob_T
 *                       are read at precision != 0 only.  workspace: mobody_bosa_target_workspace floats = round4(N A) + round4(2 N)
 *                       (a' and the twin Q, each piece rounded up to 4 floats); -1 for a bad block.  Both row-wise kernels run a
 *                       grid-stride loop over at most 4 workgroups of 256 threads (the stage's batches are a few hundred rows).
 *                       Refused with MOBODY_E_ARG before the first runtime call, the field named: struct_bytes, S outside [1, 256],
 *                       A outside [1, 128], S + A > 256 (mobody_mlp_layout's ranges), N < 1 or N > 2^21, precision, a NULL
 *                       actor_blob / q_blob / next_state / q_next / workspace, noise_clip < 0, max_action <= 0, a NaN among the three.
 *   mobody_bosa_stage2_rows   ONE launch: row_weight[i] = mask[i] * 0.5 over N rows (mask != NULL) and / or dpi[i][j] = dll[i][j] *
 *                       dpi_scale over N A elements (dll != NULL) -- single fp32 multiplies, torch.mul's bits.  dpi_scale is the
 *                       caller's -(lamda / N), formed in double and rounded once (what torch.mul does with a Python scalar).
 *   mobody_bosa_stage2_words  ONE launch of one workgroup: the logged words, STAGE2_LOG order.  closs != NULL (mobody_bosa_critic's
 *                       loss_out): words[0] = mask_mean[0], words[1] = closs[0], words[3] = closs[1], words[2] = closs[0] - cons_coef *
 *                       closs[1].  ll != NULL ([N], the policy estimator's): words[5] = mean_i(-ll[i]), words[6] = max_i(-ll[i]) with a
 *                       NaN giving NaN (torch.amax), words[4] = aloss[0] + lamda * words[5]; thread t adds rows t, t + 256, ... in
 *                       ascending order and a fixed tree joins the 256 partial results -- not torch.mean's bits, these words feed the
 *                       log only.  words[7] is not touched.  Last, bump[k] += bump_inc[k] for k < nbump <= 4 (device int64 words, by
 *                       one thread): a captured call advances its noise call id, step counts and draw count in its last launch.
 *                       Refused with MOBODY_E_ARG before any runtime call, the field named (both entries): struct_bytes, N < 1 or
 *                       N > 2^21, neither part given, a part's output or companion pointer NULL (row_weight, dpi; words, mask_mean,
 *                       aloss), A outside [1, 128] with dll, a NaN dpi_scale, nbump outside [0, 4], bump NULL with nbump > 0.
 * LAUNCHES of a stage-2 call: a critic call makes 4 (mobody_bosa_target) + 11 (mobody_bosa_loglik with mask_mean) + mobody_bosa_critic's
 * + 2 (rows before the critic, words after it); an actor call makes those with the critic in gradient form + mobody_adam_polyak's
 * + 3 (mobody_bosa_actor_forward and its copy) + mobody_bosa_loglik_grad's 19 + 6 (mobody_bosa_actor_backward) + mobody_adam_polyak's
 * + 3 (rows before the critic, rows before the actor's backward, ONE words launch with both parts at the end): two beyond the named
 * entries on a critic call and one more on an actor call. */
typedef struct MobodyBosaTarget MobodyBosaTarget;
struct MobodyBosaTarget {
  int32_t struct_bytes;
  int32_t precision;
  int32_t S, A;
  int64_t N;
  const float *actor_blob, *actor_blob_T;   /* the TARGET actor, mobody_mlp_layout(S, A, 1) */
  const float *q_blob, *q_blob_T;           /* the TARGET twin-Q, mobody_mlp_layout(S + A, 1, 2) */
  const float* next_state;                  /* [N][S] */
  const float* noise;                       /* [N][A] unit normals, or NULL */
  uint32_t seed, call;
  const int64_t* call_dev;                  /* nullable */
  float expl_noise, noise_clip, max_action;
  int32_t reserved;                         /* 0 */
  float* q_next;                            /* [N] */
  float* workspace;
};
int64_t mobody_bosa_target_workspace(const MobodyBosaTarget* a);
int mobody_bosa_target(const MobodyBosaTarget* a, void* stream);
typedef struct MobodyBosaStage2 MobodyBosaStage2;
struct MobodyBosaStage2 {
  int32_t struct_bytes;
  int32_t A;
  int64_t N;
  const float* mask;                        /* [N], mobody_bosa_loglik's */
  float* row_weight;                        /* [N] */
  const float* dll;                         /* [N][A], mobody_bosa_loglik_grad's */
  float* dpi;                               /* [N][A] */
  float dpi_scale, cons_coef, lamda;
  int32_t nbump;
  const float *mask_mean, *closs, *ll, *aloss;
  float* words;                             /* [8] */
  int64_t* bump;
  int64_t bump_inc[4];
};
int mobody_bosa_stage2_rows(const MobodyBosaStage2* a, void* stream);
int mobody_bosa_stage2_words(const MobodyBosaStage2* a, void* stream);

/* ---- Fitted Q evaluation ------------------------------------------------------------------------------------------
 * The reference has no counterpart: it scores a policy in its simulators, which this build does not have.  FQE needs the recorded
 * target transitions and the frozen policy alone: a fresh twin-Q net is regressed onto y = r + gamma not_done Q_targ(s', pi(s'))
 * (mobody_fqe_target supplies the bootstrap value, mobody_critic in its q_next form the update) and Q(s0, pi(s0)) is reported over
 * episode starts (mobody_fqe_value).  Both entries take the policy in one of the two forms the six algorithm classes use:
 *   head 0   a deterministic actor, mobody_mlp_layout(S, A, 1): action = mobody_mlp3_forward(out_mode 1, max_action)
 *            (MOBODY, TD3_BC, BOSA)
 *   head 1   a Gaussian policy, mobody_mlp_layout(S, 2 A, 1): action = columns [0, A) of the same out_mode 1 forward over all 2 A
 *            columns = max_action * tanh(mu), what the IQL family's select_action(test=True) returns (IQL, DARA, IGDF)
 * The new kernels use no flags, no tickets and no atomics; each launch reads what an earlier launch on the stream wrote; every loop
 * is bounded by an argument; every sum and maximum runs in a fixed order, so two runs give the same bits.  The grid-stride kernels
 * size their grid from the row count (one workgroup per 256 elements).
 *   mobody_fqe_target   q_next [N] = the mean over the two members of Q_targ(s', pi(s')).  Launches, in order: the policy forward;
 *                       k_fqe_action, the pitch-changing copy [N][2 A] -> [N][A], for head 1 only (head 0 SKIPS it: three launches);
 *                       mobody_mlp3_forward of the two-member target net on [s' | a']; k_fqe_qnext, which forms
 *                       __fmul_rn(__fadd_rn(q0, q1), 0.5f) and copies a' to action_out [N][A] when that is given.  The packed
 *                       forwards' ReLU (fmaxf) turns a NaN pre-activation into 0, so k_fqe_qnext also reads the row's s' and a' and
 *                       gives a row with a NaN among them q_next = NaN; every other row keeps its bits.  On finite rows the result
 *                       has the bits of mobody_mlp3_forward, a slice [:, :A], mobody_mlp3_forward and (q[0] + q[1]) * 0.5 at
 *                       precisions 0 (f32), 3 (bf16x3) and 4 (f16x2); 1 (bf16) and 2 (bf16x2) are refused by name.  The T blobs are
 *                       read at precision != 0 only.  workspace: mobody_fqe_target_workspace floats = round4(N A) + round4(2 N) +
 *                       (head 1: round4(2 N A)), each piece rounded up to 4 floats; -1 for a bad block.
 *   mobody_fqe_value    the estimate over B start states: pi(s0) by the same head rule, the twin-Q forward of q_blob on [s0 | a0],
 *                       k_fqe_value_rows (a row with a NaN among s0, a0 gets q = NaN in both members; q_out [2][B], when given, takes
 *                       the rows) and k_fqe_value, ONE workgroup of 256 threads: out[4] = (mean q0, mean q1, mean 0.5 (q0 + q1),
 *                       max |q0 - q1|), nan_flag[0] = 1 when a q is NaN (all four words are then NaN) and 0 otherwise.  Thread t
 *                       adds rows t, t + 256, ... in ascending order and a fixed tree joins the 256 partial results; the third word
 *                       is (sum q0 + sum q1) / (2 B) of the two joined sums.  workspace: mobody_fqe_value_workspace floats, the
 *                       closed form above with B for N.
 * Refused with MOBODY_E_ARG before the first runtime call, the field named (both entries): struct_bytes, head outside {0, 1},
 * S outside [1, 256], A outside [1, 128] (head 0) or 2 A > 128 (head 1), S + A > 256, N (B) < 1 or > 2^21, precision, the T blobs
 * missing at precision != 0, a NULL policy_blob / q_blob / next_state (state) / q_next (out, nan_flag) / workspace, max_action <= 0
 * or NaN. */
typedef struct MobodyFqeTarget MobodyFqeTarget;
struct MobodyFqeTarget {
  int32_t struct_bytes;
  int32_t precision;
  int32_t head;                             /* 0 deterministic actor, 1 Gaussian policy */
  int32_t S, A;
  int32_t reserved;                         /* 0 */
  int64_t N;
  const float *policy_blob, *policy_blob_T; /* the frozen policy: mobody_mlp_layout(S, A, 1) (head 0) or (S, 2 A, 1) (head 1) */
  const float *q_blob, *q_blob_T;           /* FQE's TARGET twin-Q, mobody_mlp_layout(S + A, 1, 2) */
  const float* next_state;                  /* [N][S] */
  float max_action;
  int32_t reserved1;                        /* 0 */
  float* action_out;                        /* [N][A], or NULL */
  float* q_next;                            /* [N] */
  float* workspace;
};
int64_t mobody_fqe_target_workspace(const MobodyFqeTarget* a);
int mobody_fqe_target(const MobodyFqeTarget* a, void* stream);
typedef struct MobodyFqeValue MobodyFqeValue;
struct MobodyFqeValue {
  int32_t struct_bytes;
  int32_t precision;
  int32_t head;
  int32_t S, A;
  int32_t reserved;                         /* 0 */
  int64_t B;
  const float *policy_blob, *policy_blob_T;
  const float *q_blob, *q_blob_T;           /* FQE's ONLINE twin-Q */
  const float* state;                       /* [B][S] start states */
  float max_action;
  int32_t reserved1;                        /* 0 */
  float* q_out;                             /* [2][B], or NULL */
  float* out;                               /* [4] */
  int32_t* nan_flag;                        /* [1] */
  float* workspace;
};
int64_t mobody_fqe_value_workspace(const MobodyFqeValue* a);
int mobody_fqe_value(const MobodyFqeValue* a, void* stream);

/* ---- Every policy in the learned model, with member spread -----------------------------------------------------------
 * mobody_ens_evaluate_policy is mobody_ens_evaluate for both policy head forms, with an optional fixed member per episode; the two
 * entries run one host loop.  What it computes: the row state of mobody_ens_evaluate (same semantics per step, same accounting),
 * with the action of step t formed by the head rule of mobody_fqe_target:
 *   head 0   policy_blob is mobody_mlp_layout(S, A, 1); a = mobody_mlp3_forward(out_mode 1, max_action)
 *   head 1   policy_blob is mobody_mlp_layout(S, 2 A, 1); a = columns [0, A) of the same out_mode 1 forward over all 2 A columns
 *            = max_action * tanh(mu), what the IQL family's select_action(test=True) returns
 * and the elite of row b at step t chosen by member_mode:
 *   0   drawn per row and per step by the sample kernel (elite_idx = NULL), as mobody_ens_evaluate
 *   1   member[b] for every step of the episode (PETS' TS-infinity): `member` int32 [B] is caller-owned row state, read and written
 *       in this mode only.  resume == 0 sets member[b] = elites[b % n_elites]; resume == 1 reads it as it is.  Every step hands
 *       `member` to the sample kernel as elite_idx; the noise stays the device generator's at call id call0 + t + call_dev[0].
 *       With B = n_elites * K rows, row b is start state b / n_elites under member b % n_elites.
 * Launches, in order.  resume == 0: k_eval_init, then k_eval_members (member_mode 1 only).  Per step: the policy forward;
 * k_fqe_action, the pitch-changing copy [B][2 A] -> [B][A] (head 1 only: head 0 SKIPS it); the member forward; k_dyn_sample; the
 * reward head; k_eval_account.  5 launches per step at head 0, 6 at head 1, whatever member_mode is.  With head = 0 and
 * member_mode = 0 the launches and the bits are those of mobody_ens_evaluate.  Head 1 has the bits of mobody_mlp3_forward on the
 * (S, 2 A, 1) net, the slice [:, :A], mobody_ens_step under the carried alive mask (elite_idx = member in mode 1) and the accounting.
 * MOBODY_E_ARG before the first runtime call, the field named: struct_bytes, head outside {0, 1}, member_mode outside {0, 1},
 * 2 A > 128 at head 1, a null `member` in mode 1, and everything mobody_ens_evaluate refuses (the policy's blobs under the names
 * policy_blob / policy_blob_T).  B == 0 returns 0.  H == 0 with resume == 0 only initialises the row state, `member` included.
 * workspace: mobody_ens_evaluate_policy_workspace(a) floats (reads S, A, B, head; -1 for a bad block) = round4(B A) + round4(B S) +
 * round4(B) + round4(7 B S + 7 B) + 2 round4(ceil(B / 4)) + (head 1: round4(2 B A)), round4(n) = n rounded up to 4 floats: the
 * pieces of mobody_ens_evaluate_workspace in their places, the Gaussian policy's output behind them.
 * (Declared as a tagged struct plus its typedef, as MobodyEnsEval.) */
struct MobodyEnsEvalPolicy {
  int32_t struct_bytes, uncertainty_mode;
  const float *dyn_blob, *dyn_planes, *mopo_blob, *mopo_blob_T, *policy_blob, *policy_blob_T;
  int32_t precision, S, A, task;
  const float* init_obs;            /* [B][S]; read only when resume == 0 */
  int64_t B;
  int32_t H, n_elites;
  const int32_t* elites;            /* HOST array */
  uint32_t seed, call0;
  const int64_t* call_dev;          /* nullable */
  float max_action, discount;       /* discount in (0, 1] */
  int32_t use_trg, resume;
  float* obs_state;                 /* [B][S] current observation */
  uint8_t* alive;                   /* [B] */
  float *ret, *pen_sum, *disc;      /* [B] each */
  int32_t* length;                  /* [B] */
  int32_t head, member_mode;        /* 0 / 1 each */
  int32_t* member;                  /* [B]; member_mode 1 only (else nullable) */
  float* workspace;
};
typedef struct MobodyEnsEvalPolicy MobodyEnsEvalPolicy;
int64_t mobody_ens_evaluate_policy_workspace(const MobodyEnsEvalPolicy* a);
int mobody_ens_evaluate_policy(const MobodyEnsEvalPolicy* a, void* stream);

/* mobody_eval_summary: the figures of a finished row state, by member group.  Row b belongs to group b % G (G = 1: the overall
 * figures only).  out [G + 1][4] = (mean return, mean length, mean penalty sum, alive share) per group, the last row the same four
 * figures over all rows; nan_flag[0] = 1 when a ret or pen_sum is NaN, 0 otherwise.  One launch, k_eval_summary: ONE workgroup of
 * 256 threads and no atomics (k_fqe_value's pattern).  Thread t adds rows t, t + 256, ... in ascending order into per-group
 * accumulators and, in the same order, into accumulators over all rows; a fixed tree joins the 256 partial results, so two runs give
 * the same bits.  Lengths and alive counts are summed as 64-bit integers and are exact; each mean is one division by the group's row
 * count (the two integer means in fp64, rounded to fp32 once).  A NaN row makes its group's figure and the overall one NaN and
 * leaves the other groups' bits alone.  An empty group (B <= its index) gets four NaNs and does not raise the flag.
 * MOBODY_E_ARG before the first runtime call, the field named: G outside 1..7, B < 1, any null pointer.  No workspace (0 floats). */
int mobody_eval_summary(const float* ret, const float* pen_sum, const int32_t* length, const uint8_t* alive, int64_t B, int G,
                        float* out, int32_t* nan_flag, void* stream);

/* ---- The analytic off-dynamics control task, stepped on the device (mobody_amd/task.py holds the specification) ------
 * A ground truth for the evaluators: a small analytic control task with the observation / action shapes and the termination
 * predicates of the environments above, in a source and a shifted target variant.  MobodyTaskParams is the task a call runs (the
 * three entries share it).  With z = s - mu, u_j = gain[j] * clamp(a_j / max_action, -1, 1), v = z[S-1], d_i = sum_j bmat[i][j] u_j
 * (j ascending):
 *   i not in {0, 1, S-1}:  z'_i     = z_i + dt (-f z_i + g d_i + c sin(z_{i-1}))
 *   forward speed:         z'_{S-1} = v   + dt (-f v + g fwd),  fwd = mean(u_1..u_{A-1}), or u_0 when A == 1
 *   angle:                 z'_1     = z_1 + dt (lam grav z_1 + g u_0 - k v)
 *   height:                z'_0     = z_0 + dt (-f z_0 - h grav z_1^2)
 *   noise:                 z'_i    += sigma * n_i; n = noise[b][i], or (noise == NULL) element b S + i of the unit-normal stream
 *                          (seed, MOBODY_TASK_STREAM_NOISE, call + call_dev[0]), what mobody_rng_normal writes there; sigma == 0: none
 *   next = z' + mu;  reward = z'_{S-1} + alive_bonus - ctrl_cost * mean_j(u_j^2);  terminal = the predicate `task` on next
 * All of it fp32, every product and sum rounded on its own (no contraction), the sums in ascending j: two calls give the same bits.
 * mu [S], gain [A] and bmat [S][A] are DEVICE tables the host forms once (no device cos).  S in [3, 256], A in [1, 64]. */
enum { MOBODY_TASK_STREAM_NOISE = 4,   /* process noise [B][S] */
       MOBODY_TASK_STREAM_ACTION = 5,  /* the built-in controllers' action noise [B][A] */
       MOBODY_TASK_STREAM_START = 6 }; /* start states: element b S + i at call id e = the episode's index in its lane */
enum { MOBODY_TASK_CTRL_RANDOM = 0,    /* a_j uniform in [-1, 1): 2 u - 1 of word (b A + j) & 3 of the stream's counter (b A + j) >> 2 */
       MOBODY_TASK_CTRL_FEEDBACK = 1 };/* a_0 = -6 z_1 + 0.15 v, every other a_j = push; + eps_a * unit normal; clipped to [-1, 1] */
struct MobodyTaskParams {
  int32_t S, A, task, reserved;            /* task: MOBODY_TERM_*; reserved 0 */
  const float *mu, *gain, *bmat;           /* device [S], [A], [S][A] */
  float f, grav, dt, g, c, lam, k, h, sigma, alive_bonus, ctrl_cost, max_action;
};
typedef struct MobodyTaskParams MobodyTaskParams;

/* mobody_task_step: one launch, k_task_step, over B rows.  k_dyn_sample's geometry: a workgroup owns 256 / S whole rows staged in
 * LDS, one thread per (row, dim) element; one thread per row then forms the reward and the predicate.  No flags, tickets or
 * atomics.  alive (nullable, uint8 [B]): a dead row is computed like any other and its terminal is written 0.  obs / next_obs may
 * be the same array.  MOBODY_E_ARG before the first runtime call, the field named: struct_bytes, S, A, task (pen needs S > 26),
 * max_action <= 0, B < 0, any null pointer among mu, gain, bmat, obs, act, next_obs, reward, terminal.  B == 0 returns 0. */
struct MobodyTaskStep {
  int32_t struct_bytes, reserved;
  MobodyTaskParams p;
  const float *obs, *act;           /* [B][S], [B][A] */
  int64_t B;
  const float* noise;               /* [B][S], or NULL: the device generator */
  const uint8_t* alive;             /* [B], nullable */
  uint32_t seed, call;
  const int64_t* call_dev;          /* nullable device word added to `call` */
  float *next_obs, *reward;         /* [B][S], [B] */
  uint8_t* terminal;                /* [B] */
};
typedef struct MobodyTaskStep MobodyTaskStep;
int mobody_task_step(const MobodyTaskStep* a, void* stream);

/* mobody_task_evaluate: the TRUE return of a policy in the task, with the row-state contract of mobody_ens_evaluate_policy (resume,
 * obs_state, alive, ret, disc, length, discount, call0, call_dev, H); pen_sum is initialised to zero and never written again, so
 * mobody_eval_summary serves the row state unchanged.  head 0 / 1: the two policy forms of mobody_ens_evaluate_policy; head 2: the
 * built-in controller (ctrl, ctrl_push, ctrl_eps; no policy blob is read).  Per step: the policy forward (heads 0, 1); k_fqe_action
 * (head 1); k_task_advance, which forms the head-2 action, advances the task with the device generator at call id call0 + t +
 * call_dev[0] and does k_eval_account's accounting on the row state (ret = fma(disc, reward, ret), length, disc, alive &= !terminal,
 * obs_state = next) -- 2 / 3 / 1 launches per step at heads 0 / 1 / 2, one more (k_eval_init) when resume == 0.  Heads 0 and 1 have
 * the bits of mobody_mlp3_forward (out_mode 1; the slice [:, :A] at head 1), mobody_task_step under the carried mask and the
 * accounting.  A captured chunk replays with resume = 1.  MOBODY_E_ARG before the first runtime call, the field named: what
 * mobody_task_step refuses of the task, head outside {0, 1, 2}, ctrl outside {0, 1} (head 2), 2 A > 128 (head 1), resume, discount
 * outside (0, 1], H < 0, precision (an unknown id, or any id but f32 without policy_blob_T), any null pointer.  B == 0 returns 0.
 * workspace: mobody_task_evaluate_workspace(a) floats = round4(B A) + (head 1: round4(2 B A)); -1 for a bad block. */
struct MobodyTaskEval {
  int32_t struct_bytes, precision;
  MobodyTaskParams p;
  const float *policy_blob, *policy_blob_T;
  const float* init_obs;            /* [B][S]; read only when resume == 0 */
  int64_t B;
  int32_t H, head;
  int32_t ctrl, resume;
  float ctrl_push, ctrl_eps;
  uint32_t seed, call0;
  const int64_t* call_dev;          /* nullable */
  float discount, reserved;
  float* obs_state;                 /* [B][S] */
  uint8_t* alive;                   /* [B] */
  float *ret, *pen_sum, *disc;      /* [B] each */
  int32_t* length;                  /* [B] */
  float* workspace;
};
typedef struct MobodyTaskEval MobodyTaskEval;
int64_t mobody_task_evaluate_workspace(const MobodyTaskEval* a);
int mobody_task_evaluate(const MobodyTaskEval* a, void* stream);

/* mobody_task_collect: a dataset from `lanes` parallel lanes, each stepped L times by a built-in controller; one launch per step
 * (k_task_collect: controller, advance, record, reset) after one that sets the lanes' first start states.  Step t of lane b writes
 * row b L + t of observations [lanes L][S], actions [lanes L][A], next_observations, rewards [lanes L] and terminals (uint8).  A lane
 * restarts after a terminal step (terminals = 1) and after its time_limit-th step of an episode (terminals = 0 unless the predicate
 * holds too).  The e-th start state of lane b is mu + init_std * element b S + i of the unit-normal stream (seed,
 * MOBODY_TASK_STREAM_START, e).  Lane b < split runs controller 0 of (ctrl, ctrl_push, ctrl_eps), the others controller 1.  Step t
 * draws at call id call0 + t.  MOBODY_E_ARG before the first runtime call, the field named: what mobody_task_step refuses of the
 * task, lanes < 0, L < 0, time_limit < 1, split outside [0, lanes], ctrl outside {0, 1}, any null pointer.  lanes == 0 or L == 0
 * returns 0.  workspace: mobody_task_collect_workspace(a) floats = round4(lanes S) + 2 round4(lanes). */
struct MobodyTaskCollect {
  int32_t struct_bytes, reserved;
  MobodyTaskParams p;
  int64_t lanes, split;
  int32_t L, time_limit;
  int32_t ctrl[2];
  float ctrl_push[2], ctrl_eps[2];
  float init_std;
  uint32_t seed, call0, reserved1;
  float *observations, *actions, *next_observations, *rewards;
  uint8_t* terminals;
  float* workspace;
};
typedef struct MobodyTaskCollect MobodyTaskCollect;
int64_t mobody_task_collect_workspace(const MobodyTaskCollect* a);
int mobody_task_collect(const MobodyTaskCollect* a, void* stream);

/* mobody_task_interact: ONE interaction of the current policy with the task on `lanes` parallel lanes, recorded straight into a
 * replay ring (the driver's online modes 1 and 2, lines 675-770 of the reference's train_mobody.py).  Three launches, no host
 * read, no flags, tickets or atomics:
 *   1. the packed 3-layer forward on lane_obs, in `precision` with the net's T blob: head 0 = mobody_mlp_layout(S, A, 1), out_mode 1
 *      (pi(s)); head 1 = mobody_mlp_layout(S, 2 A, 1), raw (mu | logstd)
 *   2. k_task_interact (k_task's geometry: a workgroup owns 256 / S whole lanes).  With c = the interaction count count[0]:
 *        head 0: base = pi;  head 1 (select_action(test=False) of the reference's iql.py, lines 74-89 and 160-166):
 *                base = max_action * tanh(mu + exp(clamp(logstd, -20, 2)) * n1),  n1 = element b A + j of (seed, MOBODY_TASK_STREAM_POLICY, c)
 *        expl != 0: a = clamp(base + (expl * max_action) * n2, -max_action, max_action), n2 = the same element of (seed,
 *                MOBODY_TASK_STREAM_EXPLORE, c) (its mode-2 loop, lines 733-735); expl == 0: nothing is drawn and a = base
 *        step:   mobody_task_step's arithmetic on (lane_obs, a), process noise from (seed, MOBODY_TASK_STREAM_NOISE, call0 + c)
 *        lane:   t = lane_t + 1; stored done = predicate && t < time_limit; the episode ends when the predicate holds or
 *                t == time_limit (the mode-1 loop, lines 684-709).  On an end done_count += 1, ret_sum += lane_ret + reward, len_sum += t,
 *                lane_t = lane_ret = 0, lane_ep += 1 and lane_obs = mu + init_std * element b S + i of (seed,
 *                MOBODY_TASK_STREAM_START, lane_ep) (mobody_task_collect's rule); otherwise lane_t = t, lane_ret += reward,
 *                lane_obs = next.  The accumulators are per LANE: the host adds them in lane order when it reads them.
 *        record: lane b writes (state, a, next, reward, not_done = 1 - done) into row (ptr + b) mod cap of `ring`, ptr = ptr_size[0],
 *                and zeroes the padding of a row-interleaved ring's row as mobody_ring_append does.  ptr_size and count are only read.
 *   3. k_task_commit, one thread: ptr = (ptr + lanes) mod cap, size = min(size + lanes, cap), count += 1.
 * Every product and sum is an fp32 operation of its own in the order written; head 0 has the bits of mobody_mlp3_forward,
 * mobody_rng_normal, mobody_task_step and mobody_ring_append composed.  A captured call replays (nothing it bakes in changes).
 * MOBODY_E_ARG before the first runtime call, the field named: struct_bytes, what mobody_task_step refuses of the task, head outside
 * {0, 1}, 2 A > 128 (head 1), lanes < 0, lanes > cap, time_limit < 1, expl < 0, precision (an unknown id, or any id but f32 without
 * policy_blob_T), any null pointer (those of the view included).  lanes == 0 returns 0 and writes nothing.
 * workspace: mobody_task_interact_workspace(a) floats = round4(lanes A) (head 1: round4(2 lanes A)); -1 for a bad block. */
enum { MOBODY_TASK_STREAM_POLICY = 11,   /* the Gaussian policy's action sample [lanes][A], call id = the interaction count */
       MOBODY_TASK_STREAM_EXPLORE = 12 };/* exploration noise [lanes][A], call id = the interaction count */
struct MobodyTaskInteract {
  int32_t struct_bytes, precision;
  MobodyTaskParams p;
  const float *policy_blob, *policy_blob_T;
  int64_t lanes, cap;
  int32_t head, time_limit;
  float expl, init_std;
  uint32_t seed, call0;
  const MobodyBufferView* ring;     /* HOST struct of device pointers, `cap` rows */
  int64_t* ptr_size;                /* device int64[2] = {ptr, size} of the ring */
  int64_t* count;                   /* device word: interactions so far */
  float* lane_obs;                  /* [lanes][S]: the lanes' current states */
  int32_t *lane_t, *lane_ep;        /* [lanes]: steps into the episode, episode index */
  float* lane_ret;                  /* [lanes]: the running episode return */
  int32_t* done_count;              /* [lanes]: finished episodes */
  float* ret_sum;                   /* [lanes]: sum of their returns */
  int32_t* len_sum;                 /* [lanes]: sum of their lengths */
  float* workspace;
};
typedef struct MobodyTaskInteract MobodyTaskInteract;
int64_t mobody_task_interact_workspace(const MobodyTaskInteract* a);
int mobody_task_interact(const MobodyTaskInteract* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOBODY_HIP_H */
