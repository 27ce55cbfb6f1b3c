"""Which test runs each entry point of include/olympic_hip.h, from oly_ilmlp_packed_floats down to oly_iq_q_update, on
fenced and poisoned operands (tests/fences.py).  No tests here: tests/test_il_fence_ledger_cpu.py holds the table to the
header without a GPU, so an entry point added to the header fails there until it is fenced or exempted with a reason.

COVERED: entry point -> (test file, test function).  EXEMPT: entry point -> one line saying why it needs no fence."""
IL, K10, IQ = "test_gpu_il_fences.py", "test_gpu_fences.py", "test_gpu_iq_q.py"

COVERED = {
    # K16
    "oly_ilmlp_pack": (IL, "test_k16_ilmlp_pack_and_forward"),
    "oly_ilmlp_forward": (IL, "test_k16_ilmlp_pack_and_forward"),
    "oly_il_critic_fit_epoch": (IL, "test_k16_il_critic_fit_epoch"),
    # K15
    "oly_disc_fit_epoch": (IL, "test_k15_disc_fit_epoch"),
    "oly_disc_fit_epoch_pair": (IL, "test_k15_disc_fit_epoch_pair"),
    # K18
    "oly_gail_disc_forward": (IL, "test_k18_gail_reward_step_and_forward"),
    "oly_gail_reward_step": (IL, "test_k18_gail_reward_step_and_forward"),
    "oly_gail_disc_forward_pair": (IL, "test_k18_gail_reward_step_and_forward_pair"),
    "oly_gail_reward_step_pair": (IL, "test_k18_gail_reward_step_and_forward_pair"),
    "oly_gail_disc_fit_epoch": (IL, "test_k18_gail_disc_fit_epoch"),
    "oly_gail_disc_fit_epoch_pair": (IL, "test_k18_gail_disc_fit_epoch_pair"),
    # K19
    "oly_gail_disc_log": (IL, "test_k19_disc_log"),
    "oly_disc_log": (IL, "test_k19_disc_log"),
    # K17
    "oly_trpo_grad": (IL, "test_k17_trpo_grad_and_fvp"),
    "oly_trpo_fvp": (IL, "test_k17_trpo_grad_and_fvp"),
    "oly_trpo_step": (IL, "test_k17_trpo_step"),
    # K20
    "oly_episode_stats": (IL, "test_k20_episode_stats"),
    "oly_iter_log": (IL, "test_k20_iter_log"),
    # K21, K22
    "oly_il_act": (IL, "test_k21_il_act"),
    "oly_il_reset_where": (IL, "test_k22_il_reset_where"),
    # K23, K24
    "oly_a3_reset_draw": (K10, "test_k23_reset_draw"),
    "oly_bc_targets": (K10, "test_k24_targets"),
    "oly_bc_fit_steps": (K10, "test_k24_fit"),
    "oly_bc_fit_steps_log": (K10, "test_k24_logged_fit"),
    # K25
    "oly_sg_act": (IL, "test_k25_sg_act"),
    # K26
    "oly_iq_q_update": (IQ, "test_fenced_operands_and_stores"),
}

_SIZE = "a size query on integers: it takes no device pointer"
EXEMPT = {
    "oly_ilmlp_packed_floats": _SIZE,
    "oly_il_critic_fit_ws_floats": _SIZE,
    "oly_disc_fit_ws_floats": _SIZE,
    "oly_disc_fit_pair_ws_floats": _SIZE,
    "oly_gail_disc_fit_ws_floats": _SIZE,
    "oly_gail_disc_fit_pair_ws_floats": _SIZE,
    "oly_gail_disc_log_ws_floats": _SIZE,
    "oly_disc_log_ws_floats": _SIZE,
    "oly_trpo_param_count": _SIZE,
    "oly_trpo_ws_floats": _SIZE,
    "oly_trpo_old_offsets": "two offsets into the workspace computed on the host and written to host integers: no device pointer",
    "oly_iter_log_ws_floats": _SIZE,
    "oly_bc_fit_ws": _SIZE,
    "oly_bc_fit_log_ws": _SIZE,
    "oly_iq_q_ws": _SIZE,
    "oly_iq_q_ws_values": _SIZE,
}
