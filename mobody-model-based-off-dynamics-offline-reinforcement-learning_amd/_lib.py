"""ctypes binding of libmobody_hip.so -- the only way product code reaches the GPU kernels.

Mirrors include/mobody_hip.h one to one.  Loading fails loudly (ImportError) when the
library has not been built: there is deliberately no CPU or PyTorch fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmobody_hip.so")

i32, i64, u32, f32 = C.c_int32, C.c_int64, C.c_uint32, C.c_float
vp = C.c_void_p


class MobodyLayer(C.Structure):
    _fields_ = [("in_dim", i32), ("out_dim", i32), ("Kp", i32), ("Np", i32), ("w_off", i64), ("b_off", i64)]


DL_NAMES = ["zs1", "zs2", "zs3", "za_src1", "za_src2", "za_trg1", "za_trg2", "transition1", "transition2",
            "transition3", "reward_model1", "reward_model2", "reward_model3"]


class MobodyDynLayout(C.Structure):
    _fields_ = [("S", i32), ("A", i32), ("E", i32), ("_pad", i32), ("layer", MobodyLayer * len(DL_NAMES)),
                ("total_floats", i64)]


class MobodyMlpLayout(C.Structure):
    _fields_ = [("in_dim", i32), ("out_dim", i32), ("members", i32), ("Kp1", i32), ("Np3", i32), ("Np1t", i32),
                ("w1", i64), ("b1", i64), ("w2", i64), ("b2", i64), ("w3", i64), ("b3", i64),
                ("member_floats", i64), ("total_floats", i64), ("w3t", i64), ("w2t", i64), ("w1t", i64),
                ("t_member_floats", i64), ("t_total_floats", i64), ("w2p", i64), ("w2tp", i64)]


class MobodyPretrainLayout(C.Structure):
    _fields_ = [("S", i32), ("A", i32), ("za_in", i32), ("_pad", i32), ("enc", MobodyMlpLayout), ("tr", MobodyMlpLayout),
                ("rw", MobodyMlpLayout), ("off_enc", i64), ("off_tr", i64), ("off_rw", i64), ("off_za_src", i64),
                ("off_za_trg", i64), ("za_w1", i64), ("za_b1", i64), ("za_w2", i64), ("za_b2", i64),
                ("za_member_floats", i64), ("total_floats", i64), ("t_off_enc", i64), ("t_off_tr", i64),
                ("t_off_rw", i64), ("t_total_floats", i64)]


class MobodyPretrainMopoLayout(C.Structure):
    _fields_ = [("S", i32), ("A", i32), ("_pad0", i32), ("_pad1", i32), ("dyn", MobodyMlpLayout), ("rw", MobodyMlpLayout),
                ("off_dyn", i64), ("off_rw", i64), ("total_floats", i64), ("t_off_dyn", i64), ("t_off_rw", i64),
                ("t_total_floats", i64)]


class MobodyBufferView(C.Structure):
    _fields_ = [("state", vp), ("action", vp), ("next_state", vp), ("reward", vp), ("not_done", vp), ("pitch", i64)]


class MobodyTrainDims(C.Structure):
    _fields_ = [("S", i32), ("A", i32), ("N", i64), ("Nt", i64), ("N_global", i64), ("Nt_global", i64)]


class MobodyHyper(C.Structure):
    _fields_ = [("gamma", f32), ("tau", f32), ("max_action", f32), ("weight", f32), ("bc_coef", f32),
                ("q_weighted", i32), ("scale_q", i32), ("precision", i32)]


class MobodyGatherRng(C.Structure):
    _fields_ = [("bufs", C.POINTER(MobodyBufferView)), ("counts", C.POINTER(i64)), ("nbuf", C.c_int), ("seeds", C.POINTER(u32)),
                ("call_offsets", C.POINTER(i64)), ("counter", vp), ("sizes", C.POINTER(vp)), ("bump", C.POINTER(vp)),
                ("nbump", C.c_int)]


class MobodyEnsStep(C.Structure):
    _fields_ = [("struct_bytes", i32), ("uncertainty_mode", i32), ("dyn_blob", vp), ("dyn_planes", vp), ("mopo_blob", vp),
                ("mopo_blob_T", vp), ("precision", i32), ("S", i32), ("A", i32), ("task", i32), ("obs", vp), ("act", vp),
                ("B", i64), ("noise", vp), ("elite_idx", vp), ("alive", vp), ("elites", C.POINTER(i32)), ("n_elites", i32),
                ("seed", u32), ("call", u32), ("use_penalty", i32), ("call_dev", vp), ("penalty_coef", f32), ("use_trg", i32),
                ("next_obs", vp), ("reward", vp), ("terminal", vp), ("penalty", vp), ("raw_reward", vp), ("mean_out", vp),
                ("workspace", vp)]


class MobodyEnsRollout(C.Structure):
    _fields_ = [("struct_bytes", i32), ("uncertainty_mode", i32), ("dyn_blob", vp), ("dyn_planes", vp), ("mopo_blob", vp),
                ("mopo_blob_T", vp), ("actor_blob", vp), ("actor_blob_T", vp), ("precision", i32), ("S", i32), ("A", i32),
                ("task", i32), ("init_obs", vp), ("B", i64), ("H", i32), ("n_elites", i32), ("elites", C.POINTER(i32)),
                ("seed", u32), ("call0", u32), ("call_dev", vp), ("max_action", f32), ("penalty_coef", f32),
                ("env_filter", f32), ("use_penalty", i32), ("use_trg", i32), ("filter_bad_rollout", i32),
                ("ring", C.POINTER(MobodyBufferView)), ("cap", i64), ("ptr_size", vp), ("workspace", vp)]


class MobodyEnsEval(C.Structure):
    _fields_ = [("struct_bytes", i32), ("uncertainty_mode", i32), ("dyn_blob", vp), ("dyn_planes", vp), ("mopo_blob", vp),
                ("mopo_blob_T", vp), ("actor_blob", vp), ("actor_blob_T", vp), ("precision", i32), ("S", i32), ("A", i32),
                ("task", i32), ("init_obs", vp), ("B", i64), ("H", i32), ("n_elites", i32), ("elites", C.POINTER(i32)),
                ("seed", u32), ("call0", u32), ("call_dev", vp), ("max_action", f32), ("discount", f32), ("use_trg", i32),
                ("resume", i32), ("obs_state", vp), ("alive", vp), ("ret", vp), ("pen_sum", vp), ("disc", vp), ("length", vp),
                ("workspace", vp)]


class MobodyEnsEvalPolicy(C.Structure):
    _fields_ = [("struct_bytes", i32), ("uncertainty_mode", i32), ("dyn_blob", vp), ("dyn_planes", vp), ("mopo_blob", vp),
                ("mopo_blob_T", vp), ("policy_blob", vp), ("policy_blob_T", vp), ("precision", i32), ("S", i32), ("A", i32),
                ("task", i32), ("init_obs", vp), ("B", i64), ("H", i32), ("n_elites", i32), ("elites", C.POINTER(i32)),
                ("seed", u32), ("call0", u32), ("call_dev", vp), ("max_action", f32), ("discount", f32), ("use_trg", i32),
                ("resume", i32), ("obs_state", vp), ("alive", vp), ("ret", vp), ("pen_sum", vp), ("disc", vp), ("length", vp),
                ("head", i32), ("member_mode", i32), ("member", vp), ("workspace", vp)]


class MobodyEnsReplay(C.Structure):
    _fields_ = [("struct_bytes", i32), ("uncertainty_mode", i32), ("dyn_blob", vp), ("dyn_planes", vp), ("mopo_blob", vp),
                ("mopo_blob_T", vp), ("precision", i32), ("S", i32), ("A", i32), ("task", i32),
                ("data", C.POINTER(MobodyBufferView)), ("data_rows", i64), ("row0", vp), ("B", i64), ("H", i32),
                ("reset_every", i32), ("n_elites", i32), ("elites", C.POINTER(i32)), ("seed", u32), ("call0", u32),
                ("call_dev", vp), ("use_trg", i32), ("obs_state", vp), ("act_state", vp), ("obs_err", vp), ("rew_err", vp),
                ("penalty", vp), ("term_model", vp), ("workspace", vp)]


# Argument blocks of the train step and of the pre-training step: one field per argument, in the header's order.  Float and
# counter pointers are c_void_p (torch data_ptr()); what keeps two of them apart is the field NAME the caller writes.
class MobodyCritic(C.Structure):
    _fields_ = [("struct_bytes", i32), ("phase", i32), ("d", MobodyTrainDims), ("h", MobodyHyper), ("actor_blob", vp),
                ("actor_blob_T", vp), ("q_blob", vp), ("q_blob_T", vp), ("qtarg_blob", vp), ("qtarg_blob_T", vp), ("state", vp),
                ("action", vp), ("next_state", vp), ("reward", vp), ("not_done", vp), ("q_next", vp), ("grad_q", vp), ("m", vp), ("v", vp),
                ("t", i64), ("t_dev", vp), ("lr", f32), ("policy_forward", i32), ("loss_out", vp), ("workspace", vp),
                ("bump", vp), ("gather", C.POINTER(MobodyGatherRng))]


class MobodyActor(C.Structure):
    _fields_ = [("struct_bytes", i32), ("policy_ready", i32), ("d", MobodyTrainDims), ("h", MobodyHyper), ("actor_blob", vp),
                ("actor_blob_T", vp), ("q_blob", vp), ("q_blob_T", vp), ("state", vp), ("action", vp), ("stats", vp),
                ("workspace", vp), ("v_true", vp), ("grad_actor", vp), ("m", vp), ("v", vp), ("t", i64), ("t_dev", vp), ("lr", f32),
                ("loss_out", vp)]


class MobodyIql(C.Structure):
    _fields_ = [("struct_bytes", i32), ("reserved", i32), ("d", MobodyTrainDims), ("h", MobodyHyper), ("lam", f32), ("temp", f32),
                ("T_max", i64), ("v_blob", vp), ("v_blob_T", vp), ("q_blob", vp), ("q_blob_T", vp), ("qtarg_blob", vp),
                ("qtarg_blob_T", vp), ("pi_blob", vp), ("pi_blob_T", vp), ("state", vp), ("action", vp), ("next_state", vp),
                ("reward", vp), ("not_done", vp), ("adv", vp), ("grad", vp), ("m", vp), ("v", vp), ("t", i64), ("t_dev", vp),
                ("lr", f32), ("bump", vp), ("loss_out", vp), ("log_out", vp), ("workspace", vp)]


class MobodyDara(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("d", MobodyTrainDims), ("n_src", i64), ("sa_blob", vp), ("sa_blob_T", vp),
                ("sas_blob", vp), ("sas_blob_T", vp), ("state", vp), ("action", vp), ("next_state", vp), ("reward", vp),
                ("noise_sas", vp), ("noise_sa", vp), ("noise_std", f32), ("eta", f32), ("seed", u32), ("call", u32), ("call_dev", vp),
                ("call_offset", i64), ("grad_sa", vp), ("grad_sas", vp), ("m_sa", vp), ("v_sa", vp), ("m_sas", vp), ("v_sas", vp),
                ("t", i64), ("t_dev", vp), ("lr", f32), ("reserved", i32), ("delta_out", vp), ("loss_out", vp), ("log_out", vp),
                ("workspace", vp)]


class MobodyIgdf(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("d", MobodyTrainDims), ("n", i64), ("k", i64), ("Z", i32),
                ("importance_weight", f32), ("sa_blob", vp), ("sa_blob_T", vp), ("ss_blob", vp), ("ss_blob_T", vp), ("state", vp),
                ("action", vp), ("next_state", vp), ("reward", vp), ("not_done", vp), ("out_state", vp), ("out_action", vp),
                ("out_next_state", vp), ("out_reward", vp), ("out_not_done", vp), ("row_weight", vp), ("score_out", vp),
                ("kept_out", vp), ("grad_sa", vp), ("grad_ss", vp), ("m_sa", vp), ("v_sa", vp), ("m_ss", vp), ("v_ss", vp),
                ("t", i64), ("t_dev", vp), ("bump", vp), ("lr", f32), ("reserved", i32), ("loss_out", vp), ("workspace", vp)]


class MobodyAdam(C.Structure):
    _fields_ = [("struct_bytes", i32), ("in_dim", i32), ("out_dim", i32), ("members", i32), ("blob", vp), ("blob_T", vp),
                ("grad", vp), ("m", vp), ("v", vp), ("target", vp), ("target_T", vp), ("t", i64), ("t_dev", vp), ("lr", f32), ("tau", f32),
                ("grad_scale", f32), ("precision", i32)]


class MobodyPretrain(C.Structure):
    _fields_ = [("struct_bytes", i32), ("S", i32), ("A", i32), ("use_trg", i32), ("b", i64), ("b_global", i64),
                ("encoder_loss_coef", f32), ("transition_coef", f32), ("reward_coef", f32), ("precision", i32), ("blob", vp),
                ("blob_T", vp), ("xenc", vp), ("act", vp), ("rew", vp), ("noise6", vp), ("noise7", vp), ("seed", u32),
                ("call", u32), ("call_dev", vp), ("grad", vp), ("m", vp), ("v", vp), ("t_main", i64), ("t_za", i64), ("t_dev", vp),
                ("lr", f32), ("loss_out", vp), ("loss_acc", vp), ("workspace", vp)]


class MobodyPretrainMopo(C.Structure):
    _fields_ = [("struct_bytes", i32), ("S", i32), ("A", i32), ("use_trg", i32), ("b", i64), ("b_global", i64),
                ("encoder_loss_coef", f32), ("precision", i32), ("blob", vp), ("blob_T", vp), ("xenc", vp), ("act", vp),
                ("rew", vp), ("noise", vp), ("seed", u32), ("call", u32), ("call_dev", vp), ("grad", vp), ("m", vp), ("v", vp), ("t", i64),
                ("t_dev", vp), ("lr", f32), ("loss_out", vp), ("loss_acc", vp), ("workspace", vp)]


class MobodyWideLayout(C.Structure):
    _fields_ = [("in_dim", i32), ("hidden", i32), ("out_dim", i32), ("members", i32), ("Kp1", i32), ("Hp", i32), ("Np3", i32),
                ("_pad", i32), ("w1", i64), ("b1", i64), ("w2", i64), ("b2", i64), ("w3", i64), ("b3", i64),
                ("member_floats", i64), ("total_floats", i64)]


class MobodyWideFwd(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("layout", MobodyWideLayout), ("blob", vp), ("src0", vp), ("src1", vp),
                ("src2", vp), ("src_width0", i32), ("src_width1", i32), ("src_width2", i32), ("x_shared", i32),
                ("src_member_stride0", i64), ("src_member_stride1", i64), ("src_member_stride2", i64), ("src_rows0", i64),
                ("src_rows1", i64), ("src_rows2", i64), ("rows", i64),
                ("out_mode", i32), ("max_action", f32), ("out", vp), ("save_x", vp), ("save_h1", vp), ("save_h2", vp),
                ("workspace", vp)]


class MobodyWideBwd(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("layout", MobodyWideLayout), ("blob", vp), ("dz3", vp), ("x", vp),
                ("h1", vp), ("h2", vp), ("x_shared", i32), ("reserved", i32), ("rows", i64), ("grad", vp), ("dx", vp),
                ("dx_col0", i32), ("dx_col1", i32), ("workspace", vp)]


class MobodyWideAdam(C.Structure):
    _fields_ = [("struct_bytes", i32), ("reserved", i32), ("blob", vp), ("grad", vp), ("m", vp), ("v", vp), ("n", i64), ("t", i64),
                ("t_dev", vp), ("lr", f32), ("reserved1", i32)]


class MobodyBosaVae(C.Structure):
    _fields_ = [("struct_bytes", i32), ("kind", i32), ("S", i32), ("A", i32), ("hidden", i32), ("members", i32), ("precision", i32),
                ("num_samples", i32), ("B", i64), ("beta", f32), ("max_action", f32), ("blob", vp), ("state", vp), ("action", vp),
                ("next_state", vp), ("eps", vp), ("seed", u32), ("call", u32), ("call_dev", vp), ("grad", vp), ("m", vp), ("v", vp),
                ("t", i64), ("t_dev", vp), ("lr", f32), ("log_eps", f32), ("loss_out", vp), ("ll", vp), ("min_ll", vp), ("mask", vp),
                ("mask_mean", vp), ("w_out", vp), ("workspace", vp)]


class MobodyBosaTarget(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("S", i32), ("A", i32), ("N", i64), ("actor_blob", vp), ("actor_blob_T", vp),
                ("q_blob", vp), ("q_blob_T", vp), ("next_state", vp), ("noise", vp), ("seed", u32), ("call", u32), ("call_dev", vp),
                ("expl_noise", f32), ("noise_clip", f32), ("max_action", f32), ("reserved", i32), ("q_next", vp), ("workspace", vp)]


class MobodyBosaStage2(C.Structure):
    _fields_ = [("struct_bytes", i32), ("A", i32), ("N", i64), ("mask", vp), ("row_weight", vp), ("dll", vp), ("dpi", vp),
                ("dpi_scale", f32), ("cons_coef", f32), ("lamda", f32), ("nbump", i32), ("mask_mean", vp), ("closs", vp), ("ll", vp),
                ("aloss", vp), ("words", vp), ("bump", vp), ("bump_inc", i64 * 4)]


class MobodyFqeTarget(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("head", i32), ("S", i32), ("A", i32), ("reserved", i32), ("N", i64),
                ("policy_blob", vp), ("policy_blob_T", vp), ("q_blob", vp), ("q_blob_T", vp), ("next_state", vp), ("max_action", f32),
                ("reserved1", i32), ("action_out", vp), ("q_next", vp), ("workspace", vp)]


class MobodyFqeValue(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("head", i32), ("S", i32), ("A", i32), ("reserved", i32), ("B", i64),
                ("policy_blob", vp), ("policy_blob_T", vp), ("q_blob", vp), ("q_blob_T", vp), ("state", vp), ("max_action", f32),
                ("reserved1", i32), ("q_out", vp), ("out", vp), ("nan_flag", vp), ("workspace", vp)]


class MobodyTaskParams(C.Structure):
    _fields_ = [("S", i32), ("A", i32), ("task", i32), ("reserved", i32), ("mu", vp), ("gain", vp), ("bmat", vp), ("f", f32),
                ("grav", f32), ("dt", f32), ("g", f32), ("c", f32), ("lam", f32), ("k", f32), ("h", f32), ("sigma", f32),
                ("alive_bonus", f32), ("ctrl_cost", f32), ("max_action", f32)]


class MobodyTaskStep(C.Structure):
    _fields_ = [("struct_bytes", i32), ("reserved", i32), ("p", MobodyTaskParams), ("obs", vp), ("act", vp), ("B", i64), ("noise", vp),
                ("alive", vp), ("seed", u32), ("call", u32), ("call_dev", vp), ("next_obs", vp), ("reward", vp), ("terminal", vp)]


class MobodyTaskEval(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("p", MobodyTaskParams), ("policy_blob", vp), ("policy_blob_T", vp),
                ("init_obs", vp), ("B", i64), ("H", i32), ("head", i32), ("ctrl", i32), ("resume", i32), ("ctrl_push", f32),
                ("ctrl_eps", f32), ("seed", u32), ("call0", u32), ("call_dev", vp), ("discount", f32), ("reserved", f32),
                ("obs_state", vp), ("alive", vp), ("ret", vp), ("pen_sum", vp), ("disc", vp), ("length", vp), ("workspace", vp)]


class MobodyTaskCollect(C.Structure):
    _fields_ = [("struct_bytes", i32), ("reserved", i32), ("p", MobodyTaskParams), ("lanes", i64), ("split", i64), ("L", i32),
                ("time_limit", i32), ("ctrl", i32 * 2), ("ctrl_push", f32 * 2), ("ctrl_eps", f32 * 2), ("init_std", f32), ("seed", u32),
                ("call0", u32), ("reserved1", u32), ("observations", vp), ("actions", vp), ("next_observations", vp), ("rewards", vp),
                ("terminals", vp), ("workspace", vp)]


WIDE_OUT_MODES = {"raw": 0, "tanh": 1}
BOSA_KINDS = {"policy": 0, "dynamics": 1}
BOSA_STREAMS = {"policy": 6, "dynamics": 7, "policy_ll": 8, "dynamics_ll": 9, "target_noise": 10}    # MOBODY_BOSA_STREAM_*


class MobodyTaskInteract(C.Structure):
    _fields_ = [("struct_bytes", i32), ("precision", i32), ("p", MobodyTaskParams), ("policy_blob", vp), ("policy_blob_T", vp),
                ("lanes", i64), ("cap", i64), ("head", i32), ("time_limit", i32), ("expl", f32), ("init_std", f32), ("seed", u32),
                ("call0", u32), ("ring", C.POINTER(MobodyBufferView)), ("ptr_size", vp), ("count", vp), ("lane_obs", vp),
                ("lane_t", vp), ("lane_ep", vp), ("lane_ret", vp), ("done_count", vp), ("ret_sum", vp), ("len_sum", vp),
                ("workspace", vp)]


def block(cls, **fields):
    """An argument block with struct_bytes set and `fields` by name (everything else zero / NULL)."""
    return cls(struct_bytes=BLOCK_BYTES[cls], **fields)


BLOCK_BYTES = {cls: C.sizeof(cls) for cls in (MobodyCritic, MobodyActor, MobodyIql, MobodyDara, MobodyIgdf, MobodyAdam, MobodyPretrain, MobodyPretrainMopo,
                                             MobodyWideFwd, MobodyWideBwd, MobodyWideAdam, MobodyBosaVae, MobodyBosaTarget, MobodyBosaStage2, MobodyEnsStep, MobodyEnsRollout,
                                             MobodyEnsEval, MobodyEnsEvalPolicy, MobodyEnsReplay, MobodyFqeTarget, MobodyFqeValue,
                                             MobodyTaskStep, MobodyTaskEval, MobodyTaskCollect, MobodyTaskInteract)}


PRECISIONS = {"f32": 0, "bf16": 1, "bf16x2": 2, "bf16x3": 3, "f16x2": 4}


# MOBODYEnsembleDynamics(uncertainty_mode=...) -> MOBODY_UNC_* (mobody_dynamics.py:241-252)
UNCERTAINTY_MODES = {"pairwise-diff": 0, "aleatoric": 1, "ensemble_std": 2}

TERM_IDS = {"never": 0, "halfcheetah": 1, "hopper": 2, "ant": 3, "walker2d": 4, "humanoid": 5, "pen": 6}

# device health words (include/mobody_hip.h)
HEALTH_WORDS, HEALTH_F16_RANGE, HEALTH_NONFINITE = 8, 1, 2

# name -> (restype, argtypes); must list every symbol include/mobody_hip.h declares
PROTOTYPES = {
    "mobody_last_error": (C.c_char_p, []),
    "mobody_abi_version": (C.c_int, []),
    "mobody_dyn_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(MobodyDynLayout)]),
    "mobody_mlp_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(MobodyMlpLayout)]),
    "mobody_prof_begin": (C.c_int, [C.c_int]),
    "mobody_prof_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(i64), C.c_int]),
    "mobody_health_bind": (C.c_int, [vp]),
    "mobody_health_clear": (C.c_int, [vp]),
    "mobody_rng_normal": (C.c_int, [u32, u32, u32, i64, vp, vp]),
    "mobody_rng_index": (C.c_int, [u32, u32, u32, i64, u32, vp, vp]),
    "mobody_dyn_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, i64, C.c_int, vp, vp]),
    "mobody_dyn_planes_floats": (i64, []),
    "mobody_dyn_planes": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp]),
    "mobody_dyn_step_workspace": (i64, [C.c_int, C.c_int, i64]),
    "mobody_dyn_step": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, i64, vp, vp, vp, C.POINTER(i32), C.c_int,
                                  u32, u32, vp, f32, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mobody_mopo_step": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, i64, vp, vp, vp, C.POINTER(i32), C.c_int,
                                   u32, u32, f32, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mobody_ens_step": (C.c_int, [C.POINTER(MobodyEnsStep), vp]),
    "mobody_ens_rollout_workspace": (i64, [C.POINTER(MobodyEnsRollout)]),
    "mobody_ens_rollout": (C.c_int, [C.POINTER(MobodyEnsRollout), vp]),
    "mobody_ens_evaluate_workspace": (i64, [C.POINTER(MobodyEnsEval)]),
    "mobody_ens_evaluate": (C.c_int, [C.POINTER(MobodyEnsEval), vp]),
    "mobody_ens_evaluate_policy_workspace": (i64, [C.POINTER(MobodyEnsEvalPolicy)]),
    "mobody_ens_evaluate_policy": (C.c_int, [C.POINTER(MobodyEnsEvalPolicy), vp]),
    "mobody_eval_summary": (C.c_int, [vp, vp, vp, vp, i64, C.c_int, vp, vp, vp]),
    "mobody_task_step": (C.c_int, [C.POINTER(MobodyTaskStep), vp]),
    "mobody_task_evaluate_workspace": (i64, [C.POINTER(MobodyTaskEval)]),
    "mobody_task_evaluate": (C.c_int, [C.POINTER(MobodyTaskEval), vp]),
    "mobody_task_collect_workspace": (i64, [C.POINTER(MobodyTaskCollect)]),
    "mobody_task_collect": (C.c_int, [C.POINTER(MobodyTaskCollect), vp]),
    "mobody_task_interact_workspace": (i64, [C.POINTER(MobodyTaskInteract)]),
    "mobody_task_interact": (C.c_int, [C.POINTER(MobodyTaskInteract), vp]),
    "mobody_ens_replay_workspace": (i64, [C.POINTER(MobodyEnsReplay)]),
    "mobody_ens_replay": (C.c_int, [C.POINTER(MobodyEnsReplay), vp]),
    "mobody_rollout_workspace": (i64, [C.c_int, C.c_int, i64]),
    "mobody_rollout": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp, i64, C.c_int, C.POINTER(i32), C.c_int, u32, u32, f32,
                                 C.c_int, C.c_int, f32, C.c_int, C.POINTER(MobodyBufferView), i64, vp, vp, vp]),
    "mobody_termination": (C.c_int, [C.c_int, vp, i64, C.c_int, vp, vp]),
    "mobody_rollout_mask": (C.c_int, [vp, vp, vp, f32, C.c_int, i64, vp, vp, vp]),
    "mobody_sample_indices": (C.c_int, [u32, u32, vp, i64, i64, vp, vp, vp]),
    "mobody_counter_add": (C.c_int, [vp, C.c_int, i64, vp]),
    "mobody_mlp3_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, i64, C.c_int, f32, vp,
                                      vp, vp, vp, vp]),
    "mobody_gather_batch": (C.c_int, [C.POINTER(MobodyBufferView), C.POINTER(vp), C.POINTER(i64), C.c_int, C.c_int,
                                      C.c_int, vp, vp, vp, vp, vp, vp]),
    "mobody_gather_batch_rng": (C.c_int, [C.POINTER(MobodyBufferView), C.POINTER(i64), C.c_int, C.c_int, C.c_int,
                                          C.POINTER(u32), C.POINTER(i64), vp, C.POINTER(vp), vp, vp, vp, vp, vp, C.POINTER(vp), C.c_int,
                                          vp]),
    "mobody_ring_append": (C.c_int, [C.POINTER(MobodyBufferView), i64, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, i64, vp,
                                     vp]),
    "mobody_ring_pitch": (i64, [C.c_int, C.c_int]),
    "mobody_train_workspace": (i64, [C.POINTER(MobodyTrainDims)]),
    "mobody_critic": (C.c_int, [C.POINTER(MobodyCritic), vp]),
    "mobody_actor_forward": (C.c_int, [C.POINTER(MobodyActor), vp]),
    "mobody_actor_backward": (C.c_int, [C.POINTER(MobodyActor), vp]),
    "mobody_td3bc_actor_forward": (C.c_int, [C.POINTER(MobodyActor), vp]),
    "mobody_td3bc_actor_backward": (C.c_int, [C.POINTER(MobodyActor), vp]),
    "mobody_bosa_actor_forward": (C.c_int, [C.POINTER(MobodyActor), vp, vp]),
    "mobody_bosa_actor_backward": (C.c_int, [C.POINTER(MobodyActor), vp, vp]),
    "mobody_iql_workspace": (i64, [C.POINTER(MobodyTrainDims)]),
    "mobody_iql_value": (C.c_int, [C.POINTER(MobodyIql), vp]),
    "mobody_iql_critic": (C.c_int, [C.POINTER(MobodyIql), vp]),
    "mobody_iql_actor": (C.c_int, [C.POINTER(MobodyIql), vp]),
    "mobody_dara_workspace": (i64, [C.POINTER(MobodyTrainDims)]),
    "mobody_dara_classifier": (C.c_int, [C.POINTER(MobodyDara), vp]),
    "mobody_dara_relabel": (C.c_int, [C.POINTER(MobodyDara), vp]),
    "mobody_igdf_workspace": (i64, [C.POINTER(MobodyTrainDims), i64, i32]),
    "mobody_igdf_contrast": (C.c_int, [vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp]),
    "mobody_igdf_select": (C.c_int, [vp, i64, i64, f32, vp, vp, vp]),
    "mobody_igdf_info": (C.c_int, [C.POINTER(MobodyIgdf), vp]),
    "mobody_igdf_filter": (C.c_int, [C.POINTER(MobodyIgdf), vp]),
    "mobody_igdf_critic": (C.c_int, [C.POINTER(MobodyIql), vp, vp]),
    "mobody_bosa_critic": (C.c_int, [C.POINTER(MobodyCritic), vp, vp, f32, i64, vp]),
    "mobody_adam_polyak": (C.c_int, [C.POINTER(MobodyAdam), vp]),
    "mobody_value_loss_grad": (C.c_int, [vp, vp, i64, i64, vp, vp, vp, vp]),
    "mobody_par_penalty": (C.c_int, [vp, vp, vp, f32, i64, C.c_int, vp]),
    "mobody_mlp3_backward_workspace": (i64, [C.c_int, C.c_int, C.c_int, i64]),
    "mobody_mlp3_backward": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, i64, vp, vp, vp]),
    "mobody_dara_inputs": (C.c_int, [vp, vp, vp, i64, C.c_int, C.c_int, f32, vp, vp, u32, u32, vp, vp, vp]),
    "mobody_dara_loss_grad": (C.c_int, [vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]),
    "mobody_dara_penalty": (C.c_int, [vp, vp, i64, f32, vp, vp, vp]),
    "mobody_mlp_transpose": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "mobody_pretrain_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(MobodyPretrainLayout)]),
    "mobody_pretrain_transpose": (C.c_int, [C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "mobody_pretrain_workspace": (i64, [C.c_int, C.c_int, i64]),
    "mobody_pretrain_gather": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, vp, i64, C.c_int, C.c_int, vp, vp, vp, vp]),
    "mobody_pretrain": (C.c_int, [C.POINTER(MobodyPretrain), vp]),
    "mobody_pretrain_adam": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, i64, i64, f32, f32, C.c_int, C.c_int, i64, vp]),
    "mobody_pretrain_za_adam": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, i64, f32, f32, vp]),
    "mobody_pretrain_mopo_layout": (C.c_int, [C.c_int, C.c_int, C.POINTER(MobodyPretrainMopoLayout)]),
    "mobody_pretrain_mopo_transpose": (C.c_int, [C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "mobody_pretrain_mopo_workspace": (i64, [C.c_int, C.c_int, i64]),
    "mobody_pretrain_mopo": (C.c_int, [C.POINTER(MobodyPretrainMopo), vp]),
    "mobody_pretrain_mopo_adam": (C.c_int, [C.c_int, C.c_int, vp, vp, vp, vp, vp, i64, f32, f32, C.c_int, vp]),
    "mobody_dyn_validate_mopo": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, i64, vp, vp, vp]),
    "mobody_dyn_validate_workspace": (i64, [C.c_int, C.c_int, i64]),
    "mobody_dyn_validate": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, i64, C.c_int, vp, vp, vp]),
    "mobody_wide_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MobodyWideLayout)]),
    "mobody_wide_mlp3_forward_workspace": (i64, [C.POINTER(MobodyWideLayout), i64]),
    "mobody_wide_mlp3_forward": (C.c_int, [C.POINTER(MobodyWideFwd), vp]),
    "mobody_wide_mlp3_backward_workspace": (i64, [C.POINTER(MobodyWideLayout), i64]),
    "mobody_wide_mlp3_backward": (C.c_int, [C.POINTER(MobodyWideBwd), vp]),
    "mobody_wide_mlp3_input_grad": (C.c_int, [C.POINTER(MobodyWideBwd), vp]),
    "mobody_wide_adam": (C.c_int, [C.POINTER(MobodyWideAdam), vp]),
    "mobody_bosa_workspace": (i64, [C.POINTER(MobodyBosaVae)]),
    "mobody_bosa_reparam": (C.c_int, [vp, vp, vp, i64, i32, f32, vp, vp, vp, vp, vp]),
    "mobody_bosa_vae": (C.c_int, [C.POINTER(MobodyBosaVae), vp]),
    "mobody_bosa_loglik": (C.c_int, [C.POINTER(MobodyBosaVae), vp]),
    "mobody_bosa_loglik_grad_workspace": (i64, [C.POINTER(MobodyBosaVae)]),
    "mobody_bosa_loglik_grad": (C.c_int, [C.POINTER(MobodyBosaVae), vp, vp]),
    "mobody_bosa_target_workspace": (i64, [C.POINTER(MobodyBosaTarget)]),
    "mobody_bosa_target": (C.c_int, [C.POINTER(MobodyBosaTarget), vp]),
    "mobody_bosa_stage2_rows": (C.c_int, [C.POINTER(MobodyBosaStage2), vp]),
    "mobody_bosa_stage2_words": (C.c_int, [C.POINTER(MobodyBosaStage2), vp]),
    "mobody_fqe_target_workspace": (i64, [C.POINTER(MobodyFqeTarget)]),
    "mobody_fqe_target": (C.c_int, [C.POINTER(MobodyFqeTarget), vp]),
    "mobody_fqe_value_workspace": (i64, [C.POINTER(MobodyFqeValue)]),
    "mobody_fqe_value": (C.c_int, [C.POINTER(MobodyFqeValue), vp]),
}

_lib = None


def load():
    """Load the shared library once; raise ImportError (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch ships its own HIP runtime; it has to be in the process BEFORE this library is mapped so that both bind
    # to the same runtime instance (the reverse order left the kernels with "no ROCm-capable device is detected").
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python {os.path.join(_HERE, 'csrc', 'build.py')}` "
            "(or __graft_entry__.build()). There is no CPU fallback for the MOBODY hot path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.mobody_abi_version() != 7:
        raise ImportError("libmobody_hip.so ABI version mismatch")
    _lib = lib
    return lib


class MobodyError(RuntimeError):
    pass


def check(rc, what=""):
    if rc != 0:
        msg = load().mobody_last_error().decode(errors="replace")
        raise MobodyError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device pointer of a contiguous torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C ABI needs contiguous tensors"
    return t.data_ptr()


_dev_index = None


def cur_stream():
    """Raw hipStream_t of torch's current stream (also the capture stream inside torch.cuda.graph).  Uses the
    raw-handle accessor: torch.cuda.current_stream() builds a Stream object and costs ~8 us per call, which at ~8
    calls per train() step was a fifth of the eager host overhead."""
    global _dev_index
    import torch
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_dev_index)


def dyn_layout(S, A):
    L = MobodyDynLayout()
    check(load().mobody_dyn_layout(S, A, C.byref(L)), "mobody_dyn_layout")
    return L


def mlp_layout(in_dim, out_dim, members):
    L = MobodyMlpLayout()
    check(load().mobody_mlp_layout(in_dim, out_dim, members, C.byref(L)), "mobody_mlp_layout")
    return L


def pretrain_layout(S, A):
    L = MobodyPretrainLayout()
    check(load().mobody_pretrain_layout(S, A, C.byref(L)), "mobody_pretrain_layout")
    return L


def pretrain_mopo_layout(S, A):
    L = MobodyPretrainMopoLayout()
    check(load().mobody_pretrain_mopo_layout(S, A, C.byref(L)), "mobody_pretrain_mopo_layout")
    return L


def wide_layout(in_dim, hidden, out_dim, members=1):
    L = MobodyWideLayout()
    check(load().mobody_wide_layout(in_dim, hidden, out_dim, members, C.byref(L)), "mobody_wide_layout")
    return L
