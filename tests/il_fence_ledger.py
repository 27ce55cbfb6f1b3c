"""Which test runs each entry point of include/olympic_hip.h, every function it declares with an int or int64_t result,
on fenced and poisoned operands (tests/fences.py).  No tests here: tests/test_il_fence_ledger_cpu.py holds the table to
the header without a GPU, so an entry point added to the header fails there until it is fenced or exempted with a reason.

COVERED: entry point -> (test file, test function).  EXEMPT: entry point -> one line saying why it needs no fence."""
IL, K10, IQ = "test_gpu_il_fences.py", "test_gpu_fences.py", "test_gpu_iq_q.py"
ENV, IQ_PI = "test_gpu_env_fences.py", "test_gpu_iq_pi.py"

COVERED = {
    # K1 / K5 and the imitation-learning host batcher
    "oly_il_step": (ENV, "test_k1_il_step"),
    "oly_il_ctrl": (ENV, "test_k1_il_ctrl"),
    "oly_batcher_set_prev": (ENV, "test_host_batcher_step"),
    "oly_batcher_step": (ENV, "test_host_batcher_step"),
    # K4 and the expert data
    "oly_traj_reset": (ENV, "test_k4_traj_reset_next_euler"),
    "oly_traj_next": (ENV, "test_k4_traj_reset_next_euler"),
    "oly_traj_euler": (ENV, "test_k4_traj_reset_next_euler"),
    "oly_expert_gather": (ENV, "test_expert_gather_and_dataset"),
    "oly_expert_dataset": (ENV, "test_expert_gather_and_dataset"),
    # K3
    "oly_contact_reduce": (ENV, "test_k3_contact_reduce_and_csr"),
    "oly_contact_reduce_csr": (ENV, "test_k3_contact_reduce_and_csr"),
    "oly_il_ground_forces": (ENV, "test_k3_il_ground_forces_and_window"),
    "oly_il_grf_window": (ENV, "test_k3_il_ground_forces_and_window"),
    # K2 / K5 and the reinforcement-learning host batcher
    "oly_a3_step": (ENV, "test_k2_a3_step"),
    "oly_a3_pd_target": (ENV, "test_k5_a3_pd"),
    "oly_a3_pd_torque": (ENV, "test_k5_a3_pd"),
    "oly_a3_batcher_upload": (ENV, "test_a3_host_batcher_step"),
    "oly_a3_batcher_step": (ENV, "test_a3_host_batcher_step"),
    # K10, K13
    "oly_a3_vec_step": (K10, "test_k10_vec_step"),
    "oly_a3_rollout_persistent": (K10, "test_k13_persistent_rollout"),
    # K11
    "oly_mlp_pack": (K10, "test_k11_pack_and_forward"),
    "oly_mlp_forward2": (K10, "test_k11_pack_and_forward"),
    # K6
    "oly_return_scan": (ENV, "test_k6_return_scan_small"),
    "oly_return_scan_stats": (ENV, "test_k6_return_scan_small"),
    "oly_rollout_cuts": (ENV, "test_rollout_cuts"),
    # K7
    "oly_adv_stats": (ENV, "test_k7_adv_stats_and_normalize"),
    "oly_adv_normalize": (ENV, "test_k7_adv_stats_and_normalize"),
    "oly_adv_normalize_parts": (ENV, "test_k7_adv_stats_and_normalize"),
    "oly_col_stats": (ENV, "test_k7_col_stats"),
    # K8
    "oly_disc_standardize": (ENV, "test_k8_disc_standardize"),
    "oly_disc_reparam": (ENV, "test_k8_disc_reparam"),
    "oly_disc_reward": (ENV, "test_k8_disc_reward"),
    "oly_obs_filter": (ENV, "test_k8_obs_filter"),
    # K12
    "oly_disc_pack": (K10, "test_k12_disc_forward"),
    "oly_disc_forward": (K10, "test_k12_disc_forward"),
    "oly_disc_reward_step": (K10, "test_k12_disc_reward_step"),
    "oly_disc_forward_pair": (ENV, "test_k12_disc_reward_step_and_forward_pair"),
    "oly_disc_reward_step_pair": (ENV, "test_k12_disc_reward_step_and_forward_pair"),
    # K9
    "oly_signed_perm": (ENV, "test_k9_mirror_loss_and_signed_perm"),
    "oly_mirror_loss": (ENV, "test_k9_mirror_loss_and_signed_perm"),
    "oly_ppo_loss": (ENV, "test_k9_ppo_loss"),
    # K14
    "oly_ppo_update_grads": (K10, "test_k14_update_grads_ragged_and_gathered"),
    "oly_ppo_adam_step": (K10, "test_k14_adam_step"),
    "oly_ppo_update_epoch": (K10, "test_k14_update_epoch"),
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
    # K27
    "oly_iq_pi_update": (IQ_PI, "test_fenced_operands_and_stores"),
    "oly_iq_alpha_update": (IQ_PI, "test_fenced_operands_and_stores"),
}

_SIZE = "a size query on integers: it takes no device pointer"
_HOST = "it takes host pointers only and copies them to memory the context owns: no caller device pointer"
_HANDLE = "it creates, configures or queries a handle on the host: no caller device pointer"
_EVENT = "an event or stream utility of the runtime: it takes no device pointer"
EXEMPT = {
    "oly_abi_version": "it returns a constant: no pointer at all",
    "oly_create": _HANDLE,
    "oly_il_configure": _HOST,
    "oly_il_obs_dim": _SIZE,
    "oly_batcher_create": _HANDLE,
    "oly_batcher_last_timing": "three host doubles of the last step's timing: no device pointer",
    "oly_batcher_set_mapped": _HANDLE,
    "oly_batcher_enable_contacts": _HANDLE,
    "oly_batcher_enable_contacts_packed": _HANDLE,
    "oly_traj_upload": _HOST,
    "oly_expert_rows": _SIZE,
    "oly_contact_configure": _HOST,
    "oly_grf_configure": _HOST,
    "oly_a3_configure": _HOST,
    "oly_a3_vec_ctr_len": _SIZE,
    "oly_a3_batcher_create": _HANDLE,
    "oly_a3_batcher_slots": "it hands out the host addresses of one environment's pinned staging rows: no device pointer",
    "oly_a3_batcher_last_timing": "three host doubles of the last step's timing: no device pointer",
    "oly_a3_batcher_set_mapped": _HANDLE,
    "oly_a3_batcher_set_compact": _HANDLE,
    "oly_mlp_packed_floats": _SIZE,
    "oly_disc_packed_floats": _SIZE,
    "oly_ppo_update_grad_floats": _SIZE,
    "oly_ppo_update_ws_floats": "a plan query: sizes computed on the host and written to host integers, no device pointer",
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
    "oly_iq_pi_ws": _SIZE,
    "oly_iq_pi_ws_values": _SIZE,
    "oly_event_create": _EVENT,
    "oly_event_destroy": _EVENT,
    "oly_event_record": _EVENT,
    "oly_event_sync": _EVENT,
    "oly_event_elapsed_ms": _EVENT,
    "oly_stream_sync": _EVENT,
}
