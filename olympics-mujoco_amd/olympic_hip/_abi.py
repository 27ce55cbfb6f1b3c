"""ctypes mirror of include/olympic_hip.h: constants, structs and the argument lists of
every exported entry point.  Declarations only - no library is loaded here (that is
_ffi.py for the HIP library).  tests/test_abi.py checks this table against the header.
"""
import ctypes as C

OLY_OK = 0
OLY_EINVAL, OLY_ENOTCONF, OLY_EHIP, OLY_ENOMEM, OLY_ERANGE, OLY_ENODEV = -1, -2, -3, -4, -5, -6
OLY_MAX_OBS, OLY_MAX_ACT, OLY_MAX_FALL, OLY_MAX_SEQ, OLY_MAX_PERIOD = 128, 64, 16, 20, 256

REWARD_NONE, REWARD_TARGET_VELOCITY, REWARD_X_POS = 0, 1, 2
OUT_OBS_F64, OUT_CTRL_F64 = 1, 2
MODE_STANDING, MODE_FORWARD, MODE_BACKWARD, MODE_LATERAL = 1, 2, 3, 4
SCAN_RETURN, SCAN_GAE = 0, 1
SCAN_REW_F64 = 0x100
OLY_MAX_STAT_PARTS = 64
FLAG_ABSORBING, FLAG_LAST = 1, 2

i32p = C.POINTER(C.c_int32)
f64p = C.POINTER(C.c_double)
vp = C.c_void_p
PHYSICS_FN = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), vp)


class IlModel(C.Structure):
    _fields_ = [
        ("nq", C.c_int32), ("nv", C.c_int32), ("n_pos", C.c_int32), ("n_vel", C.c_int32),
        ("n_drop", C.c_int32), ("n_grf", C.c_int32), ("n_act", C.c_int32), ("nu", C.c_int32),
        ("qpos_adr", i32p), ("qvel_adr", i32p), ("act_to_ctrl", i32p),
        ("act_mean", f64p), ("act_delta", f64p), ("ctrl_lo", f64p), ("ctrl_hi", f64p),
        ("n_fall", C.c_int32), ("fall_idx", i32p), ("fall_lo", f64p), ("fall_hi", f64p),
        ("use_absorbing_states", C.c_int32), ("reward_type", C.c_int32),
        ("reward_idx", C.c_int32), ("target_velocity", C.c_double),
    ]


class A3Model(C.Structure):
    _fields_ = [
        ("nq", C.c_int32), ("nv", C.c_int32), ("nu", C.c_int32), ("period", C.c_int32),
        ("delay_frames", C.c_int32), ("target_radius", C.c_double), ("mass", C.c_double),
        ("goal_height_ref", C.c_double), ("goal_speed_ref", C.c_double),
        ("clock_lut", f64p), ("motor_offset", f64p), ("gear", f64p),
    ]


A3_INPUT_FIELDS = ["qpos", "qvel", "act_len", "act_vel", "lf_pos", "rf_pos", "lf_vel", "rf_vel",
                   "root_pos", "root_quat", "head_pos", "grf_l", "grf_r", "min_z", "n_r", "n_l", "bad"]
A3_STATE_FIELDS = ["phase", "t1", "t2", "reached_frames", "target_reached", "mode", "seq_len",
                   "sequence", "goal"]


class A3Inputs(C.Structure):
    _fields_ = [(n, vp) for n in A3_INPUT_FIELDS]


class A3State(C.Structure):
    _fields_ = [(n, vp) for n in A3_STATE_FIELDS]


A3_BLOCK_F64 = ["qpos", "qvel", "act_len", "act_vel", "lf_pos", "rf_pos", "lf_vel", "rf_vel", "root_pos", "root_quat",
                "head_pos"]
A3_BLOCK_TAIL = ["ncon", "geom1", "geom2", "force6", "cpos_z"]


class A3Blocks(C.Structure):
    """oly_a3_blocks: [K,N,...] device blocks of K consecutive physics readbacks."""
    _fields_ = [("K", C.c_int32), ("C", C.c_int32)] + [(n, vp) for n in A3_BLOCK_F64 + A3_BLOCK_TAIL]


class ContactRecord(C.Structure):
    """oly_contact_record (64 bytes): one used contact slot of the compact (CSR) contact form."""
    _fields_ = [("geom1", C.c_int32), ("geom2", C.c_int32), ("force6", C.c_double * 6), ("pos_z", C.c_double)]


class A3ResetRecord(C.Structure):
    """oly_a3_reset_record: one pre-drawn WalkingTask.reset (656 bytes)."""
    _fields_ = [("mode", C.c_int32), ("phase", C.c_int32), ("seq_len", C.c_int32), ("pad", C.c_int32),
                ("seq", (C.c_double * 4) * 20)]


class A3Rollout(C.Structure):
    """oly_a3_rollout: policy outputs, rollout-buffer rows, side list, reset pool, device counters."""
    _fields_ = [("T", C.c_int32), ("max_traj_len", C.c_int32), ("deterministic", C.c_int32), ("pad0", C.c_int32),
                ("mu", vp), ("value", vp), ("scale", vp), ("eps", vp), ("state", vp), ("pd_target", vp),
                ("buf_states", vp), ("buf_actions", vp), ("buf_rewards", vp), ("buf_values", vp), ("buf_flags", vp),
                ("buf_rew6", vp), ("traj_len", vp),
                ("side_slots", C.c_int32), ("pad1", C.c_int32), ("side_obs", vp), ("side_t", vp), ("side_count", vp),
                ("pool_depth", C.c_int32), ("pad2", C.c_int32), ("pool", vp), ("pool_count", vp),
                ("ctr", vp), ("buf_mu", vp)]


VSTEP_RESET_ALL = 1

# oly_a3_readback: per-env slots of the pinned staging (11 double arrays, ncon/geom1/geom2 int32, force6, cpos_z)
A3_READBACK_FIELDS = (("qpos", C.c_double), ("qvel", C.c_double), ("act_len", C.c_double), ("act_vel", C.c_double),
                      ("lf_pos", C.c_double), ("rf_pos", C.c_double), ("lf_vel", C.c_double), ("rf_vel", C.c_double),
                      ("root_pos", C.c_double), ("root_quat", C.c_double), ("head_pos", C.c_double),
                      ("ncon", C.c_int32), ("geom1", C.c_int32), ("geom2", C.c_int32), ("force6", C.c_double),
                      ("cpos_z", C.c_double))


class A3Readback(C.Structure):
    _fields_ = [(n, C.POINTER(t)) for n, t in A3_READBACK_FIELDS]


class IlContacts(C.Structure):
    _fields_ = [("W", C.c_int), ("C", C.c_int), ("ncon", C.POINTER(C.c_int32)), ("ncon_stride", C.c_long),
                ("geom1", C.POINTER(C.c_int32)), ("geom2", C.POINTER(C.c_int32)), ("geom_stride", C.c_long),
                ("force6", C.POINTER(C.c_double)), ("force_stride", C.c_long)]


PHYSICS_CONTACTS_FN = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(IlContacts), vp)
A3_PHYSICS_FN = C.CFUNCTYPE(None, C.c_int, C.POINTER(C.c_double), C.POINTER(A3Readback), vp)


# name -> (restype, argtypes); device/host pointers are void*.
STD_SCALAR, STD_PER_DIM, STD_FULL = 0, 1, 2
ABI_VERSION = 8          # OLY_ABI_VERSION of include/olympic_hip.h this table mirrors


class AdamNet(C.Structure):
    """oly_adam_net: one network's flat optimiser buffers."""
    _fields_ = [("param", vp), ("grad", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("packed", vp), ("in_mean", vp),
                ("in_std", vp), ("out_dim", C.c_int32), ("pad", C.c_int32)]


class PPOAdam(C.Structure):
    """oly_ppo_adam (K14's optimiser half): clip_grad_norm_ + Adam.step + re-pack for actor and critic."""
    _fields_ = [("in_dim", C.c_int32), ("step", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("max_grad_norm", C.c_float), ("norm_ready", C.c_int32), ("net", AdamNet * 2), ("ws", vp)]


class PPOUpdate(C.Structure):
    """oly_ppo_update (K14): one PPO minibatch update's gradient call."""
    _fields_ = [("B", C.c_int32), ("in_dim", C.c_int32), ("act_dim", C.c_int32),
                ("parts_actor", C.c_int32), ("parts_critic", C.c_int32),
                ("normalize_actor", C.c_int32), ("normalize_critic", C.c_int32), ("pad0", C.c_int32),
                ("obs", vp), ("mir_obs", vp), ("action", vp), ("adv", vp), ("ret", vp), ("old_mu", vp), ("idx", vp),
                ("packed_actor", vp), ("packed_critic", vp),
                ("sd", vp), ("log_sd", vp), ("old_sd", vp), ("old_log_sd", vp),
                ("act_src", vp), ("act_sign", vp),
                ("clip", C.c_float), ("vf_coeff", C.c_float), ("mirror_coeff", C.c_float), ("pad1", C.c_int32),
                ("grad_actor", vp), ("grad_critic", vp), ("scal_out", vp), ("ws", vp), ("ws_floats", C.c_int64), ("gnorm_ws", vp)]

ACT_IDENTITY, ACT_TANH = 0, 1


class ILCriticFit(C.Structure):
    """oly_il_critic_fit (K16): the imitation critic's fit state for oly_il_critic_fit_epoch."""
    _fields_ = [("in_dim", C.c_int32), ("step", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("x", vp), ("v_target", vp), ("colstats", vp),
                ("param", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("packed", vp), ("ws", vp),
                ("ws_floats", C.c_int64), ("loss_out", vp)]


class DiscFit(C.Structure):
    """oly_disc_fit (K15): the VAIL discriminator's fit state for oly_disc_fit_epoch."""
    _fields_ = [("in_dim", C.c_int32), ("n_plcy", C.c_int32), ("step", C.c_int32), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("weight_decay", C.c_float),
                ("info_constraint", C.c_float), ("lr_beta", C.c_float), ("x", vp), ("targets", vp), ("eps", vp),
                ("colstats", vp), ("param", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("packed", vp), ("beta", vp),
                ("ws", vp), ("ws_floats", C.c_int64), ("loss_out", vp), ("bce_out", vp), ("kl_out", vp),
                ("beta_out", vp)]


class GailDiscFit(C.Structure):
    """oly_gail_disc_fit (K18): GAIL's discriminator fit state for oly_gail_disc_fit_epoch."""
    _fields_ = [("in_dim", C.c_int32), ("n_plcy", C.c_int32), ("step", C.c_int32), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("weight_decay", C.c_float),
                ("entcoeff", C.c_float), ("x", vp), ("targets", vp), ("colstats", vp), ("param", vp), ("exp_avg", vp),
                ("exp_avg_sq", vp), ("packed", vp), ("ws", vp), ("ws_floats", C.c_int64), ("loss_out", vp),
                ("bce_out", vp), ("ent_out", vp)]


class DiscPair(C.Structure):
    """oly_disc_pair: the second part (next states or actions) of a paired discriminator input."""
    _fields_ = [("x2", vp), ("mask2", vp), ("stride2", C.c_int32), ("d2", C.c_int32), ("standardise", C.c_int32),
                ("pad", C.c_int32)]


class GailDiscLog(C.Structure):
    """oly_gail_disc_log_args (K19): GAIL's discriminator diagnostics for oly_gail_disc_log."""
    _fields_ = [("in_dim", C.c_int32), ("n_rows", C.c_int32), ("n_plcy", C.c_int32), ("entcoeff", C.c_float), ("x", vp),
                ("targets", vp), ("colstats", vp), ("packed", vp), ("ws", vp), ("ws_floats", C.c_int64), ("out", vp)]


class DiscLog(C.Structure):
    """oly_disc_log_args (K19): the VAIL discriminator's diagnostics for oly_disc_log."""
    _fields_ = [("in_dim", C.c_int32), ("n_rows", C.c_int32), ("n_plcy", C.c_int32), ("entcoeff", C.c_float),
                ("info_constraint", C.c_float), ("lr_beta", C.c_float), ("x", vp), ("targets", vp), ("eps", vp),
                ("beta", vp), ("colstats", vp), ("packed", vp), ("ws", vp), ("ws_floats", C.c_int64), ("out", vp)]


# out [OLY_DISC_LOG_SCALARS] of oly_gail_disc_log / oly_disc_log: the reference's tags in the order of its add_scalar
# calls (gail_TRPO.py:227-249, vail_TRPO.py:30-32); GAIL fills the first nine
OLY_DISC_LOG_SCALARS = 12
DISC_LOG_TAGS = ("DiscrimLoss", "D_Generator_Accuracy", "D_Out_Generator", "D_Expert_Accuracy", "D_Out_Expert",
                 "Bernoulli Ent.", "Neg. Bernoulli Ent. Loss (incl. in DiscrimLoss)", "Generator_loss", "Expert_Loss",
                 "Bottleneck_Loss", "Beta", "Bottleneck_Loss_times_Beta")

OLY_TRPO_ACCEPT_OR, OLY_TRPO_ACCEPT_AND, OLY_TRPO_SCALARS = 0, 1, 8


class IterLog(C.Structure):
    """oly_iter_log_args (K20): the agent's iteration diagnostics (_logging_sw) for oly_iter_log."""
    _fields_ = [("n", C.c_int32), ("in_dim", C.c_int32), ("act_dim", C.c_int32), ("T", C.c_int32), ("N", C.c_int32),
                ("rew_f64", C.c_int32), ("x", vp), ("v_target", vp), ("mu_old", vp), ("log_sigma_old", vp),
                ("log_sigma", vp), ("critic_packed", vp), ("policy_packed", vp), ("rew_env", vp), ("rew", vp), ("last", vp),
                ("colstats", vp), ("ws", vp), ("ws_floats", C.c_int64), ("out", vp)]


# out [OLY_ITER_LOG_SCALARS] of oly_iter_log: the reference's tags in the order of its add_scalar calls
# (gail_TRPO.py:267-272), then the mean episode length before rounding and the number of completed episodes
OLY_EPISODE_STATS, OLY_ITER_LOG_SCALARS = 8, 8
ITER_LOG_TAGS = ("EpTrueRewMean", "EpRewMean", "EpLenMean", "vf_loss", "entropy", "kl")


class ILAct(C.Structure):
    """oly_il_act_args (K21): one acting step (statistics update, mean network, Gaussian sample, controls)."""
    _fields_ = [("n", C.c_int32), ("in_dim", C.c_int32), ("act_dim", C.c_int32), ("update_stats", C.c_int32), ("x", vp),
                ("colstats", vp), ("packed", vp), ("log_sigma", vp), ("eps", vp), ("action", vp), ("mu", vp), ("ctrl", vp),
                ("out_flags", C.c_int32), ("pad", C.c_int32)]


class ILReset(C.Structure):
    """oly_il_reset_args (K22): the reset of the environments whose episode ended, in one launch."""
    _fields_ = [("n", C.c_int32), ("out_flags", C.c_int32), ("mask", vp), ("traj_no", vp), ("step", vp), ("cur_traj", vp),
                ("cur_step", vp), ("origin", vp), ("sample", vp), ("qpos", vp), ("qvel", vp), ("qpos_slot", vp),
                ("qvel_slot", vp), ("obs_in", vp), ("obs_out", vp), ("prev", vp), ("episode_steps", vp)]


class TRPOStep(C.Structure):
    """oly_trpo_step_args (K17): one TRPO policy step, or the gradient / FVP pieces."""
    _fields_ = [("n", C.c_int32), ("in_dim", C.c_int32), ("hidden1", C.c_int32), ("hidden2", C.c_int32),
                ("out_dim", C.c_int32), ("last_act", C.c_int32), ("n_epochs_cg", C.c_int32),
                ("n_epochs_line_search", C.c_int32), ("accept_rule", C.c_int32), ("max_kl", C.c_float),
                ("ent_coeff", C.c_float), ("cg_damping", C.c_float), ("cg_residual_tol", C.c_float),
                ("obs", vp), ("act", vp), ("adv", vp), ("colstats", vp), ("theta", vp), ("packed", vp), ("ws", vp),
                ("ws_floats", C.c_int64), ("stepdir_out", vp), ("full_step_out", vp), ("scal_out", vp)]


class BCPair(C.Structure):
    """oly_bc_pair (K24): the two indexed tables and raw actions of a paired fit, the block oly_bc_fit.pair points to."""
    _fields_ = [("d1", C.c_int32), ("d2", C.c_int32), ("stride1", C.c_int32), ("stride2", C.c_int32), ("x2", vp),
                ("actions", vp), ("central", vp), ("delta", vp)]


class BCFit(C.Structure):
    """oly_bc_fit (K24): the behavioural-cloning fit state for oly_bc_fit_steps."""
    _fields_ = [("in_dim", C.c_int32), ("act_dim", C.c_int32), ("batch", C.c_int32), ("n_rows", C.c_int32),
                ("step", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float),
                ("nll_eps", C.c_float), ("pad", C.c_int32), ("states", vp), ("targets", vp), ("idx", vp),
                ("colstats", vp), ("param", vp), ("m", vp), ("v", vp), ("packed", vp), ("ws", vp),
                ("ws_floats", C.c_int64), ("out", vp), ("pair", C.POINTER(BCPair))]


OLY_BC_MAX_BATCH, OLY_BC_MAX_ACT = 4096, 16
# out [n_steps, 3] of oly_bc_fit_steps: the reference's tags (behavioral_cloning.py:85,88,94)
BC_LOG_TAGS = ("GaussianNLLLoss", "Squashed Gaussian Entropy", "MSELoss (between mean & target actions)")
# column 3 of oly_bc_fit_steps_log's out [n_steps, 4] (behavioral_cloning.py:92)
BC_LOG_TAG_EMPIRICAL = "Squashed Gaussian Entropy (Empirical)"


class BCFitLog(C.Structure):
    """oly_bc_fit_log (K24 + K25): oly_bc_fit with the sampled second forward of logging()."""
    _fields_ = [("fit", BCFit), ("logging_iter", C.c_int32), ("iter0", C.c_int32), ("eps", vp)]


class SGAct(C.Structure):
    """oly_sg_act_args (K25): the squashed-Gaussian policy's act and log-probability in one call."""
    _fields_ = [("n", C.c_int32), ("in_dim", C.c_int32), ("act_dim", C.c_int32), ("update_stats", C.c_int32), ("x", vp),
                ("colstats", vp), ("packed", vp), ("log_std_min", C.c_float), ("log_std_max", C.c_float), ("central", vp),
                ("delta", vp), ("eps", vp), ("action", vp), ("log_prob", vp), ("mu", vp), ("log_sigma", vp), ("ctrl", vp),
                ("out_flags", C.c_int32), ("pad", C.c_int32), ("x2", vp), ("d2", C.c_int32), ("stride1", C.c_int32),
                ("stride2", C.c_int32), ("n_rows", C.c_int32), ("idx", vp), ("clip_lo", vp), ("clip_hi", vp)]


class LSIQ(C.Structure):
    """oly_lsiq (K26): LSIQ's own parameters, the block oly_iq_q.lsiq points to; the h_* tail is read for the H update
    (algo "lsiq_h") alone."""
    _fields_ = [("lossQ_type", C.c_int32), ("loss_mode_exp", C.c_int32), ("Q_exp_loss", C.c_int32),
                ("target_clipping", C.c_int32), ("Q_min", C.c_float), ("Q_max", C.c_float), ("h_loss", C.c_int32),
                ("h_cost", C.c_int32), ("h_clip_expert", C.c_int32), ("h_pad", C.c_int32), ("h_tau_up", C.c_double),
                ("h_tau_down", C.c_double), ("h_max_state", vp), ("h_q_t", vp), ("h_v_t", vp)]


class IQQ(C.Structure):
    """oly_iq_q (K26): one soft-Q critic update of IQ-Learn / SQIL / LSIQ for oly_iq_q_update."""
    _fields_ = [("in_dim", C.c_int32), ("act_dim", C.c_int32), ("batch", C.c_int32), ("n_policy", C.c_int32),
                ("algo", C.c_int32), ("plcy_loss_mode", C.c_int32), ("regularizer_mode", C.c_int32),
                ("treat_absorbing", C.c_int32), ("use_target", C.c_int32), ("update_target", C.c_int32),
                ("step", C.c_int32), ("pad", C.c_int32), ("gamma", C.c_float), ("alpha", C.c_float),
                ("reg_mult", C.c_float), ("R_min", C.c_float), ("R_max", C.c_float),
                ("gradient_penalty_lambda", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("weight_decay", C.c_float), ("pad2", C.c_float), ("tau", C.c_double), ("obs", vp),
                ("act", vp), ("next_obs", vp), ("absorbing", vp), ("a_next", vp), ("logp_next", vp), ("a_pi", vp),
                ("logp_pi", vp), ("colstats", vp), ("target_colstats", vp), ("param", vp), ("m", vp), ("v", vp),
                ("packed", vp), ("target_param", vp), ("target_packed", vp), ("packed_floats", C.c_int64),
                ("target_packed_floats", C.c_int64), ("ws", vp), ("ws_floats", C.c_int64), ("out", vp),
                ("lsiq", C.POINTER(LSIQ))]


class IQV0(C.Structure):
    """oly_iq_v0 (K26): plcy_loss_mode v0's own policy draw on the expert rows, and the all-expert flag."""
    _fields_ = [("a_v0", vp), ("logp_v0", vp), ("all_expert", C.c_int32), ("pad", C.c_int32)]


OLY_IQ_Q_EXT = 0x69717630       # oly_iq_q.pad of an oly_iq_q_ext's head


class IQQExt(C.Structure):
    """oly_iq_q_ext (K26): oly_iq_q with the trailing pointer to oly_iq_v0; q.pad = OLY_IQ_Q_EXT says so."""
    _fields_ = [("q", IQQ), ("v0", C.POINTER(IQV0))]


class IQPi(C.Structure):
    """oly_iq_pi (K27): one policy update of IQ-Learn / SQIL for oly_iq_pi_update."""
    _fields_ = [("in_dim", C.c_int32), ("act_dim", C.c_int32), ("batch", C.c_int32), ("step", C.c_int32),
                ("alpha", C.c_float), ("log_std_min", C.c_float), ("log_std_max", C.c_float), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float), ("weight_decay", C.c_float),
                ("x", vp), ("eps", vp), ("central", vp), ("delta", vp), ("colstats", vp), ("param", vp), ("m", vp),
                ("v", vp), ("packed", vp), ("packed_floats", C.c_int64), ("critic_packed", vp),
                ("critic_packed_floats", C.c_int64), ("critic_param", vp), ("critic_colstats", vp), ("ws", vp),
                ("ws_floats", C.c_int64), ("action", vp), ("log_prob", vp), ("out", vp), ("h_packed", vp),
                ("h_packed_floats", C.c_int64), ("h_param", vp), ("h_colstats", vp), ("h_ws", vp), ("h_ws_floats", C.c_int64)]


class IQAlpha(C.Structure):
    """oly_iq_alpha (K27): one _update_alpha for oly_iq_alpha_update."""
    _fields_ = [("n", C.c_int32), ("step", C.c_int32), ("target_entropy", C.c_float), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("pad", C.c_float), ("log_prob", vp),
                ("state", vp)]


# out [4] of oly_iq_pi_update (iq_sac.py:441-443); slots 2 and 3 are the means of log_prob and of Q(x | a_new)
IQ_PI_TAGS = ("Actor/Loss", "Gradients/Norm2 Gradient Q wrt. Pi-parameters", "mean(log_prob)", "mean(Q)")

IQ_ALGO = {"iq": 0, "sqil": 1, "lsiq": 2, "lsiq_h": 3}
IQ_PLCY_LOSS_MODES = {"value": 0, "value_expert": 1, "value_policy": 2, "q_old_policy": 3, "v0": 4}
SQIL_PLCY_LOSS_MODES = {"plcy": 0, "value": 1, "value_plcy": 2}
IQ_REGULARIZER_MODES = {"exp_and_plcy": 0, "exp": 1, "plcy": 2, "off": 3}
# LSIQ (lsiq.py:11-23): plcy_loss_mode by lossQ_type (OLY_LSIQ_* / OLY_LSIQ_SQ_*), and the enumerants of oly_lsiq
LSIQ_PLCY_LOSS_MODES = {"value": 0, "value_expert": 1, "value_policy": 2, "q_old_policy": 3, "v0": 4,
                        "value_q_old_policy": 5, "off": 6}
LSIQ_SQIL_LIKE_MODES = {"value": 0, "value_plcy": 1, "q_old_policy": 2}
LSIQ_LOSSQ_TYPES = {"iq_like": 0, "sqil_like": 1}
LSIQ_LOSS_MODES_EXP = {"fix": 0, "bootstrap": 1}
LSIQ_Q_EXP_LOSSES = {None: 0, "MSE": 1, "Huber": 2}
LSIQ_H_LOSSES = {"MSE": 1, "Huber": 2}      # oly_lsiq.h_loss (LSIQ_HC's H_loss_mode), OLY_LSIQ_LOSS_*
# out [16] of oly_iq_q_update with algo "lsiq_h": the reference's seven tags (lsiq_h.py:94-100), then the gradient's norm
# and the running maximum of -log pi, which the reference does not log; slots 9-15 are 0
LSIQ_H_TAGS = ("H function/Loss", "H function/H", "H function/H plcy", "H function/H expert", "H function/H_step",
               "H function/H_step plcy", "H function/H_step expert", "Gradients/Norm2 Gradient LossH wrt. H-parameters",
               "H function/max_H_policy")
# out [16] of oly_iq_q_update: the reference's tags (iq_sac.py:426-428, 494, 535, 624-643); SQIL logs slot 0 as IQ-Loss/LossQ
IQ_Q_TAGS = ("IQ-Loss/Loss1", "IQ-Loss/Loss2", "IQ-Loss/Chi2 Loss", "V for policy on all states",
             "Action-Value/Q for expert", "Action-Value/Q^2 for expert", "Action-Value/Q for policy",
             "Action-Value/Q^2 for policy", "Action-Value/Reward", "Action-Value/Reward_Expert",
             "Action-Value/Reward_Policy", "Targets/expert data", "Targets/policy data",
             "Action-Value/Q Absorbing state exp", "Action-Value/Q Absorbing state plcy",
             "Gradients/Norm2 Gradient LossQ wrt. Q-parameters")


SIGNATURES = {
    "oly_strerror": (C.c_char_p, [C.c_int]),
    "oly_last_error": (C.c_char_p, [vp]),
    "oly_version": (C.c_char_p, []),
    "oly_abi_version": (C.c_int, []),
    "oly_create": (C.c_int, [C.POINTER(vp), C.c_int]),
    "oly_destroy": (None, [vp]),
    "oly_il_configure": (C.c_int, [vp, C.POINTER(IlModel)]),
    "oly_il_obs_dim": (C.c_int, [vp]),
    "oly_il_step": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                              C.c_int, vp]),
    "oly_il_ctrl": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp]),
    "oly_batcher_create": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_double, vp, vp]),
    "oly_batcher_destroy": (None, [vp]),
    "oly_batcher_qpos": (C.POINTER(C.c_double), [vp]),
    "oly_batcher_qvel": (C.POINTER(C.c_double), [vp]),
    "oly_batcher_prev": (vp, [vp]),
    "oly_batcher_set_prev": (C.c_int, [vp, vp, vp]),
    "oly_batcher_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "oly_batcher_last_timing": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "oly_batcher_set_mapped": (C.c_int, [vp, C.c_int]),
    "oly_batcher_enable_contacts": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "oly_batcher_enable_contacts_packed": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "oly_il_grf_window": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "oly_a3_batcher_create": (C.c_int, [C.POINTER(vp), vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "oly_a3_batcher_destroy": (None, [vp]),
    "oly_a3_batcher_slots": (C.c_int, [vp, C.c_int, C.POINTER(A3Readback)]),
    "oly_a3_batcher_upload": (C.c_int, [vp, vp]),
    "oly_a3_batcher_step": (C.c_int, [vp, vp, C.POINTER(A3State), vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "oly_a3_batcher_last_timing": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "oly_a3_batcher_set_mapped": (C.c_int, [vp, C.c_int]),
    "oly_a3_batcher_set_compact": (C.c_int, [vp, C.c_int]),
    "oly_traj_upload": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    "oly_traj_reset": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "oly_traj_next": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "oly_traj_euler": (C.c_int, [vp, C.c_int, C.c_int, C.c_double, vp, vp, vp]),
    "oly_expert_rows": (C.c_int64, [vp]),
    "oly_expert_gather": (C.c_int, [vp, C.c_int64, vp, C.c_int, vp, vp, vp, vp]),
    "oly_expert_dataset": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp]),
    "oly_contact_configure": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]),
    "oly_contact_reduce": (C.c_int, [vp, C.c_int, C.c_int] + [vp] * 13 + [vp]),
    "oly_contact_reduce_csr": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64] + [vp] * 7),
    "oly_a3_configure": (C.c_int, [vp, C.POINTER(A3Model)]),
    "oly_a3_step": (C.c_int, [vp, C.c_int, C.POINTER(A3Inputs), C.POINTER(A3State), vp, vp, vp, vp,
                              C.c_int, vp]),
    "oly_a3_vec_ctr_len": (C.c_int, [C.c_int]),
    "oly_a3_vec_step": (C.c_int, [vp, C.c_int, C.POINTER(A3Blocks), C.POINTER(A3State), C.POINTER(A3Rollout), C.c_int, vp]),
    "oly_a3_pd_target": (C.c_int, [vp, C.c_int, vp, vp, vp]),
    "oly_a3_pd_torque": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "oly_mlp_packed_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_mlp_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "oly_a3_rollout_persistent": (C.c_int, [vp, C.c_int, C.POINTER(A3Blocks), C.POINTER(A3State), C.POINTER(A3Rollout), C.c_int,
                                            vp, C.c_int, vp, C.c_int, vp, vp, vp]),
    "oly_mlp_forward2": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
    "oly_return_scan": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                  vp, vp, vp, vp, vp, vp, vp]),
    "oly_return_scan_stats": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                        vp, vp, vp, vp, vp, vp, vp, vp]),
    "oly_adv_stats": (C.c_int, [vp, C.c_int64, vp, vp, vp]),
    "oly_adv_normalize_parts": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_double, vp]),
    "oly_adv_normalize": (C.c_int, [vp, C.c_int64, vp, vp, C.c_int, C.c_double, vp]),
    "oly_col_stats": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "oly_disc_standardize": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    "oly_disc_reparam": (C.c_int, [vp, C.c_int64, vp, vp, vp, vp, vp]),
    "oly_disc_reward": (C.c_int, [vp, C.c_int64, vp, vp, vp]),
    "oly_disc_packed_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_disc_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 12),
    "oly_disc_forward": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int] + [vp] * 12),
    "oly_disc_reward_step": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp, C.c_int] + [vp] * 8),
    "oly_grf_configure": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp]),
    "oly_il_ground_forces": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "oly_rollout_cuts": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "oly_obs_filter": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, vp, vp]),
    "oly_signed_perm": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "oly_mirror_loss": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "oly_ppo_loss": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp,
                               C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    "oly_ppo_update_grad_floats": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "oly_ppo_update_ws_floats": (C.c_int64, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "oly_ppo_update_grads": (C.c_int, [vp, C.POINTER(PPOUpdate), vp]),
    "oly_ppo_adam_step": (C.c_int, [vp, C.POINTER(PPOAdam), vp]),
    "oly_ppo_update_epoch": (C.c_int, [vp, C.POINTER(PPOUpdate), C.POINTER(PPOAdam), vp, C.c_int, vp, vp]),
    "oly_ilmlp_packed_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_ilmlp_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 8),
    "oly_ilmlp_forward": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int] + [vp] * 7),
    "oly_il_critic_fit_ws_floats": (C.c_int64, [C.c_int, C.c_int]),
    "oly_il_critic_fit_epoch": (C.c_int, [vp, C.POINTER(ILCriticFit), vp, C.c_int, C.c_int, vp]),
    "oly_disc_fit_ws_floats": (C.c_int64, [C.c_int, C.c_int]),
    "oly_disc_fit_epoch": (C.c_int, [vp, C.POINTER(DiscFit), vp, C.c_int, C.c_int, vp]),
    "oly_gail_disc_forward": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int] + [vp] * 9),
    "oly_gail_reward_step": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, C.c_int] + [vp] * 5),
    "oly_gail_disc_fit_ws_floats": (C.c_int64, [C.c_int, C.c_int]),
    "oly_gail_disc_fit_epoch": (C.c_int, [vp, C.POINTER(GailDiscFit), vp, C.c_int, C.c_int, vp]),
    "oly_disc_forward_pair": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.POINTER(DiscPair)] + [vp] * 9),
    "oly_disc_reward_step_pair": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.POINTER(DiscPair), vp, vp, C.c_int]
                                  + [vp] * 8),
    "oly_disc_fit_pair_ws_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_disc_fit_epoch_pair": (C.c_int, [vp, C.POINTER(DiscFit), C.POINTER(DiscPair), vp, C.c_int, C.c_int, vp]),
    "oly_gail_disc_forward_pair": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.POINTER(DiscPair)] + [vp] * 6),
    "oly_gail_reward_step_pair": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.POINTER(DiscPair), vp, vp, C.c_int]
                                  + [vp] * 5),
    "oly_gail_disc_fit_pair_ws_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_gail_disc_fit_epoch_pair": (C.c_int, [vp, C.POINTER(GailDiscFit), C.POINTER(DiscPair), vp, C.c_int, C.c_int, vp]),
    "oly_gail_disc_log_ws_floats": (C.c_int64, [C.c_int]),
    "oly_disc_log_ws_floats": (C.c_int64, [C.c_int]),
    "oly_gail_disc_log": (C.c_int, [vp, C.POINTER(GailDiscLog), C.POINTER(DiscPair), vp]),
    "oly_disc_log": (C.c_int, [vp, C.POINTER(DiscLog), C.POINTER(DiscPair), vp]),
    "oly_trpo_param_count": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_trpo_ws_floats": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "oly_trpo_old_offsets": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "oly_episode_stats": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, vp, vp]),
    "oly_iter_log_ws_floats": (C.c_int64, [C.c_int]),
    "oly_iter_log": (C.c_int, [vp, C.POINTER(IterLog), vp]),
    "oly_il_act": (C.c_int, [vp, C.POINTER(ILAct), vp]),
    "oly_il_reset_where": (C.c_int, [vp, C.POINTER(ILReset), vp]),
    "oly_a3_reset_draw": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_uint64, vp, vp, C.c_double, C.c_int, vp]),
    "oly_bc_fit_ws": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_bc_targets": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp, vp, vp, vp]),
    "oly_bc_fit_steps": (C.c_int, [vp, C.POINTER(BCFit), C.c_int, vp]),
    "oly_bc_fit_log_ws": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_bc_fit_steps_log": (C.c_int, [vp, C.POINTER(BCFitLog), C.c_int, vp]),
    "oly_sg_act": (C.c_int, [vp, C.POINTER(SGAct), vp]),
    "oly_iq_q_ws": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_iq_q_ws_values": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_iq_q_update": (C.c_int, [vp, C.POINTER(IQQ), vp]),
    "oly_iq_pi_ws": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_iq_pi_ws_values": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "oly_iq_pi_update": (C.c_int, [vp, C.POINTER(IQPi), vp]),
    "oly_iq_alpha_update": (C.c_int, [vp, C.POINTER(IQAlpha), vp]),
    "oly_trpo_grad": (C.c_int, [vp, C.POINTER(TRPOStep), C.c_int, vp, vp, vp, vp]),
    "oly_trpo_fvp": (C.c_int, [vp, C.POINTER(TRPOStep), C.c_int, vp, vp, vp, vp, vp]),
    "oly_trpo_step": (C.c_int, [vp, C.POINTER(TRPOStep), vp]),
    "oly_event_create": (C.c_int, [C.POINTER(vp)]),
    "oly_event_destroy": (C.c_int, [vp]),
    "oly_event_record": (C.c_int, [vp, vp]),
    "oly_event_sync": (C.c_int, [vp]),
    "oly_event_elapsed_ms": (C.c_int, [vp, vp, C.POINTER(C.c_float)]),
    "oly_stream_sync": (C.c_int, [vp]),
}
