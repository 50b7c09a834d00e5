"""ctypes binding of librgstep.so (the gfx950 HIP stepper behind the C ABI of include/rgstep.h).

There is no CPU fallback: if the library is missing or no MI355X is visible the product raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGSTEP_LIB") or os.path.join(_HERE, "csrc", "librgstep.so")   # (RGSTEP_LIB: A/B builds of the same ABI, tools/ only)

RG_F_QPOS, RG_F_QVEL, RG_F_CTRL, RG_F_PID, RG_F_WARMSTART, RG_F_TIME, RG_F_STATUS, RG_F_STATS, RG_F_DEBUG, RG_F_COST, RG_F_PAIRLB, RG_F_ENVPRM = range(12)
RB_F_MOCAP, RB_F_EQ_DATA, RB_F_EQ_ACTIVE, RB_F_SENSORDATA = 12, 13, 14, 15
RG_STATUS_BAD_STATE, RG_STATUS_CON_FULL, RG_STATUS_CAND_FULL, RG_STATUS_ROW_FULL, RG_STATUS_BAD_FACTOR, RG_STATUS_BAD_ACTION = 1, 2, 4, 8, 16, 32


class StepArgs(ctypes.Structure):
    """`rg_step_args` of include/rgstep.h."""

    _fields_ = [("action_dev", ctypes.c_void_p), ("goal_quat_dev", ctypes.c_void_p), ("obs_dev", ctypes.c_void_p), ("goal_dist_dev", ctypes.c_void_p),
                ("active_dev", ctypes.c_void_p), ("hold_dev", ctypes.c_void_p), ("nticks_dev", ctypes.c_void_p), ("order_dev", ctypes.c_void_p),
                ("nsubsteps", ctypes.c_int), ("nforward_ticks", ctypes.c_int), ("flags", ctypes.c_int), ("stream", ctypes.c_void_p),
                ("config", ctypes.c_int), ("redo_dev", ctypes.c_void_p), ("preticks_dev", ctypes.c_void_p), ("xdata_dev", ctypes.c_void_p)]


RG_CFG_ROLLOUT, RG_CFG_LARGE = 0, 1
RG_CFG_ITEMS = 2   # rg_kernel_resources only: the substep-granular kernel of the rollout capacities
RG_POST_NDRAW = 2 + 4 + 3 + 20


def _post_fields():
    p_, i_, f_, u_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint
    ptrs1 = ("t", "phase", "tries", "steps", "steps_since_last_goal", "successes_so_far", "goals_so_far", "consecutive",
             "prev_dist", "prev_valid", "is_successful", "goal_quat", "qpos_goal", "preticks", "reward",
             "done", "goal_reset", "trial_success", "sub_goal_ok", "env_crash", "resetting", "episode_started",
             "info_ssl", "nticks_next", "reset_mask", "live_mask", "goal_dist_before", "packed", "draws", "goal_override")
    return ([("goal_dist", p_), ("obs", p_), ("obs_dim", i_)] + [(n, p_) for n in ptrs1] + [("seed", u_), ("step", u_)]
            + [(n, p_) for n in ("parallel_quats", "qpos0", "zero_ctrl", "ctrl_lo", "ctrl_hi")]
            + [(n, f_) for n in ("success_threshold", "success_reward", "wiggle_std", "cube_body_z")]
            + [(n, i_) for n in ("max_timesteps_per_goal", "successes_needed", "use_goal_distance_reward", "pipelined", "reset_initial_steps",
                                 "n_random_initial_steps", "max_pose_resets", "cube_pos_col", "cube_quat_col", "stop_on_fall")])


class PostArgs(ctypes.Structure):
    """`rg_post_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = _post_fields()


RB_POST_NDRAW, RB_GOAL_WORDS, RB_RESET_NDRAW = 5, 16, 3 + 4 + 50 + 6 + 2 + 1 + 20


class RbPostArgs(ctypes.Structure):
    """`rb_post_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = ([("obs", ctypes.c_void_p), ("obs_dim", ctypes.c_int)]
                + [(n, ctypes.c_void_p) for n in ("t", "steps", "steps_since_last_goal", "successes_so_far", "goals_so_far", "consecutive", "prev_dist", "prev_valid",
                                                  "is_successful", "goal", "reward", "goal_dist", "done", "goal_reset", "trial_success", "sub_goal_ok", "env_crash",
                                                  "info_ssl", "force_new_goal", "draws")]
                + [("seed", ctypes.c_uint), ("step", ctypes.c_uint), ("cube_tab", ctypes.c_void_p), ("face_up_quats", ctypes.c_void_p),
                   ("face_geom", ctypes.c_int * 6), ("tip_site", ctypes.c_int * 5), ("ref_site", ctypes.c_int * 3), ("center_site", ctypes.c_int)]
                + [(n, ctypes.c_int) for n in ("cube_pos_col", "cube_quat_col", "cube_block_col", "target_block_col", "hand_col", "n_hand")]
                + [(n, ctypes.c_float) for n in ("quat_threshold", "face_threshold", "success_reward", "p_face_flip", "round_target_face")]
                + [(n, ctypes.c_int) for n in ("directions", "max_timesteps_per_goal", "successes_needed", "use_goal_distance_reward", "stop_on_fall", "goal_mode", "pipelined")]
                + [(n, ctypes.c_void_p) for n in ("phase", "tries", "nticks_next", "hold_next", "resetting", "episode_started", "reset_draws", "qpos0", "ctrl_lo", "ctrl_hi")]
                + [("wiggle_std", ctypes.c_float)]
                + [(n, ctypes.c_int) for n in ("reset_initial_steps", "n_random_initial_steps", "max_pose_resets", "num_scramble_steps", "scramble_face_angles", "randomize_face_angles")])


class RbTcpArgs(ctypes.Structure):
    """`rb_tcp_args` of include/rgstep.h."""

    _fields_ = [("arm_qposadr", ctypes.c_int * 6), ("main_arm_qposadr", ctypes.c_int * 6), ("main_gripper_actuator", ctypes.c_int), ("tcp_body", ctypes.c_int),
                ("wrist_joint", ctypes.c_int), ("reset_controller_error", ctypes.c_int), ("max_position_change", ctypes.c_float), ("speed_roll", ctypes.c_float),
                ("speed_pitch", ctypes.c_float), ("joint_drift_threshold", ctypes.c_float), ("gripper_ctrl_lo", ctypes.c_float), ("gripper_ctrl_hi", ctypes.c_float),
                ("action_index", ctypes.c_void_p), ("bins", ctypes.c_void_p), ("nbins", ctypes.c_int), ("ema_alpha", ctypes.c_float),
                ("ema_value", ctypes.c_void_p), ("ema_t", ctypes.c_void_p), ("action_out", ctypes.c_void_p), ("hold", ctypes.c_void_p), ("scripted", ctypes.c_void_p), ("wrist_only", ctypes.c_int), ("self_world", ctypes.c_int), ("nforward_ticks", ctypes.c_int),
                ("nticks", ctypes.c_void_p), ("skip", ctypes.c_void_p)]


RA_MAXOBJ = 16


def _ra_post_fields():
    _p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    return ([("obs", _p), ("obs_dim", _i), ("num_objects", _i)]
            + [(n, _p) for n in ("t", "steps", "steps_since_last_goal", "successes_so_far", "consecutive", "prev_nsucc", "prev_valid", "goal", "goal_rot", "qpos_goal", "static_obs",
                                 "reward", "goal_dist", "done", "goal_reset", "trial_success", "sub_goal_ok", "env_crash", "objects_off_table", "info_ssl")]
            + [("obj_body", _i * RA_MAXOBJ), ("tcp_body", _i), ("arm_qposadr", _i * 6), ("grip_qposadr", _i), ("grip_dofadr", _i), ("grip_act", _i), ("finger_geom", _i * 2),
               ("table_plane_geom", _i), ("force_adr", _i), ("torque_adr", _i), ("gripper_geom_mask", ctypes.c_ulonglong), ("table_min", _f * 2), ("table_max", _f * 2)]
            + [(n, _f) for n in ("table_height", "pos_threshold", "rot_threshold", "goal_pos_offset", "goal_rot_weight", "goal_reward_per_object", "success_reward",
                                 "penalty_table_collision", "penalty_objects_off_table", "penalty_safety_stop", "safety_stop_force")]
            + [(n, _i) for n in ("max_timesteps_per_goal", "successes_needed", "use_goal_distance_reward")]
            + [("solver_qpos", _p), ("solver_ctrl", _p), ("solver_nq", _i), ("solver_nu", _i), ("solver_grip_qposadr", _i), ("solver_grip_act", _i), ("frozen", _p), ("reward_clip", _f)]
            + [("goal_kind", _i), ("grip_site", _i), ("goal_dist_extra", _p)]
            + [("obj_group", _p)]
            + [("parallel_quats", _p), ("parallel_quats_180", _p), ("rot_dist_type", _i)]
            + [("num_active", _p), ("max_timesteps_per_goal_per_obj", _i)]
            + [("icp_rel", _p)]
            + [("mask_obs", _i), ("soft_mask", _i), ("mask_margin", _f), ("area_height", _f), ("area_offset", _f * 2), ("area_size", _f * 2), ("table_pos", _f * 3),
               ("table_size", _f * 3), ("used_table_portion", _f), ("seed", ctypes.c_uint), ("step", ctypes.c_uint), ("goal_in_area", _p)]
            + [("rel_dist", _p), ("rel_threshold", _f)])


class RaPostArgs(ctypes.Structure):
    """`ra_post_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = _ra_post_fields()


class RaIcpArgs(ctypes.Structure):
    """`ra_icp_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = [("icp_rel", ctypes.c_void_p), ("goal", ctypes.c_void_p), ("num_objects", ctypes.c_int), ("obj_body", ctypes.c_int * RA_MAXOBJ),
                ("src", ctypes.c_void_p), ("src_stride", ctypes.c_int), ("src_num", ctypes.c_void_p), ("tgt", ctypes.c_void_p), ("tgt_total", ctypes.c_int),
                ("tgt_adr", ctypes.c_void_p), ("tgt_num", ctypes.c_void_p), ("error_threshold", ctypes.c_float), ("obj_group", ctypes.c_void_p),
                ("num_active", ctypes.c_void_p), ("frozen", ctypes.c_void_p)]


def _ra_recipe_fields():
    _p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    return ([("num_objects", _i), ("action_dim", _i)]
            + [(n, _p) for n in ("stage", "left", "yaw", "done", "goal_reset", "hold", "hold_ctrl", "solver_active", "nticks", "scripted", "frozen", "resetting", "episode_started",
                                 "reobserve", "ended", "stabilised", "placement_failed", "t", "steps", "steps_since_last_goal", "successes_so_far", "consecutive", "prev_valid",
                                 "ema_t", "ema_value", "action_ema", "goal", "goal_rot", "qpos_goal", "static_obs")]
            + [("obj_qposadr", _i * RA_MAXOBJ), ("arm_qposadr", _i * 6), ("solver_arm_qposadr", _i * 6), ("arm_start", _f * 6), ("obj_center", (_f * 3) * RA_MAXOBJ),
               ("obj_half", (_f * 3) * RA_MAXOBJ), ("area_offset", _f * 2), ("area_size", _f * 2), ("table_pos", _f * 3), ("table_size", _f * 3), ("stabilize_steps", _i),
               ("n_random_initial_steps", _i), ("settle_steps", _i), ("seed", ctypes.c_uint), ("step", ctypes.c_uint)]
            + [("goal_kind", _i), ("height_range", _f * 2), ("object_size", _f), ("fixed_order", _i), ("target_height", _f), ("det_points", (_f * 3) * 2), ("goal_index", _p)]
            + [("obj_group", _p), ("group_mode", _i), ("sample_lam", _f * 2)]
            + [("goal_distance_ratio", _p), ("goal_distance_min", _f), ("pickup_proba", _f), ("stacking_proba", _f)]
            + [("randomize_goal_rot", _i), ("domino_distance_mul", _f)]
            + [("fixed_xy", (_f * 2) * RA_MAXOBJ), ("fixed_yaw", _f * RA_MAXOBJ)]
            + [("num_active", _p), ("num_objects_next", _p), ("used_table_portion", _f), ("park_pose", (_f * 7) * RA_MAXOBJ)]
            + [("active", _p), ("sync_mode", _i)]
            + [("goal_in_area", _p), ("soft_mask", _i), ("mask_margin", _f), ("area_height", _f)]
            + [("scene_init", _p), ("scene_init_half", _p), ("scene_goal", _p), ("scene_goal_rot", _p), ("scene_num_goals", _p), ("num_scenes", _i), ("max_scene_goals", _i), ("scene_next", _p), ("scene", _p),
               ("goal_cursor", _p), ("advance_goals", _i)])


class RaRecipeArgs(ctypes.Structure):
    """`ra_recipe_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = _ra_recipe_fields()


# the codes of the rearrange env kernels, as include/rgstep.h defines them (tests/test_rearrange_codes.py compares the two)
RA_GOAL_OBJECT_STATE, RA_GOAL_PICKANDPLACE, RA_GOAL_STACK, RA_GOAL_REACH, RA_GOAL_DET_REACH, RA_GOAL_TRAIN, RA_GOAL_DOMINOS, RA_GOAL_ATTACHED, RA_GOAL_FIXED = range(9)
RA_ROT_FULL, RA_ROT_MOD90, RA_ROT_MOD180, RA_ROT_ICP = range(4)                                          # ra_post_args.rot_dist_type
RA_OBS_STEP, RA_OBS_EPISODE_START, RA_OBS_SKIP, RA_OBS_NEW_GOAL, RA_OBS_IN_RECIPE = range(5)            # ra_post_args.frozen, ra_recipe_args.frozen / reobserve
RA_STAGE_LIVE, RA_STAGE_STABILISE, RA_STAGE_RANDOM_ACTION, RA_STAGE_SETTLE = range(4)                   # ra_recipe_args.stage
RA_GROUPS_KEEP, RA_GROUPS_SAMPLE = 0, 1                                                                  # ra_recipe_args.group_mode
RA_SYNC_PIPELINED, RA_SYNC_FORCED_END, RA_SYNC_REGOAL_ONLY = 0, 1, 2      # ra_recipe_args.sync_mode
RA_ROWS_RESTORE, RA_ROWS_PARK = 1, 2                # ra_param_rows_args.stages


class RaParamRowsArgs(ctypes.Structure):
    """`ra_param_rows_args` of include/rgstep_sync_reset.h (field order and types must match; bind() checks the size)."""

    _fields_ = [("ended", ctypes.c_void_p), ("stabilised", ctypes.c_void_p), ("episode_started", ctypes.c_void_p), ("active", ctypes.c_void_p),
                ("block_default", ctypes.c_void_p), ("num_objects", ctypes.c_int), ("obj_dofadr", ctypes.c_int * RA_MAXOBJ), ("obj_body", ctypes.c_int * RA_MAXOBJ),
                ("stabilize_damping", ctypes.c_float), ("num_active", ctypes.c_void_p), ("park_damping", ctypes.c_float), ("stages", ctypes.c_int)]


# the wrapper stack's two launches (include/rgstep.h rg_wrap_*): the packed row's keys in RG_WK_* order ("_delta": the block of the RandomizedBodyWrapper family's entries)
RG_WRAP_U_POOL, RG_WRAP_N_POOL = 32, 128
RG_WRAP_KEYS = ["cube_pos", "cube_quat", "qpos", "qvel", "hand_angle", "fingertip_pos", "goal_pos", "goal_quat", "qpos_goal", "is_goal_achieved", "fell_down", "action_history",
                "action_delay", "_delta", "noisy_cube_pos", "noisy_cube_quat", "noisy_fingertip_pos", "noisy_hand_angle", "action_ema", "achieved_goal_pos", "relative_goal_pos",
                "noisy_achieved_goal_pos", "noisy_relative_goal_pos", "achieved_goal_quat", "relative_goal_quat", "noisy_achieved_goal_quat", "noisy_relative_goal_quat",
                "relative_goal", "noisy_relative_goal", "achieved_goal", "noisy_achieved_goal", "goal", "previous_action", "reward"]


class WrapDims(ctypes.Structure):
    """`rg_wrap_dims` of include/rgstep.h."""

    _fields_ = [(n, ctypes.c_int) for n in ("nq", "nv", "nu", "nh", "ntip", "ndelta", "randomize", "relative_goal")]


class WrapLay(ctypes.Structure):
    """`rg_wrap_lay` of include/rgstep.h."""

    _fields_ = ([(n, ctypes.c_int) for n in ("fwidth", "iwidth", "W", "s_prev", "s_ema", "s_alpha", "s_aema", "s_hist", "s_slack", "s_cdown", "s_cup", "s_anmult", "s_anadd", "s_addb",
                                             "s_mulb", "s_ts", "s_wind", "s_occl", "s_ffbuf", "s_ffleft", "s_cfleft", "s_cfbuf", "s_delta", "i_emat", "i_steps", "i_drops", "i_first",
                                             "i_delay", "n_action", "n_wind")]
                + [("n_noise", ctypes.c_int * 4)] + [(n, ctypes.c_int) for n in ("u_ts", "u_wind", "u_axis", "u_ff", "u_cf")] + [("key", ctypes.c_int * len(RG_WRAP_KEYS))])


def _wrap_fields():
    p_, i_, f_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    return ([("B", i_), ("device", i_), ("dims", WrapDims), ("lay", WrapLay), ("fstate", p_), ("istate", p_), ("u", p_), ("n", p_), ("e", p_),
             ("action_index", p_), ("bins", p_), ("nbins", i_), ("action_out", p_), ("qpos", p_), ("qpos_stride", i_), ("hand_q", p_), ("pos_to_ctrl", p_),
             ("prm", p_), ("prm_stride", i_)]
            + [(n, i_) for n in ("p_ctrlrange", "p_timestep", "p_xfrc_cube", "p_mass_cube", "relative_action", "nsubsteps", "fixed_wrist", "wrist_act", "wrist_qadr")]
            + [("wrist_lo", f_), ("wrist_hi", f_), ("obs", p_), ("obs_stride", i_), ("goal_pos", p_), ("goal_quat", p_), ("qpos_goal", p_), ("is_goal_achieved", p_),
               ("contact", p_), ("contact_stride", i_), ("ncon_slots", i_), ("ncon", p_), ("ncon_stride", i_), ("env_reward", p_), ("env_done", p_), ("successes_so_far", p_),
               ("out", p_), ("reward_out", p_), ("done_out", p_), ("fell_out", p_), ("info_out", p_), ("occ_geom", f_ * 5), ("n_occ", i_)]
            + [(n, f_) for n in ("timestep0", "cube_body_z", "fall_z", "occ_cutoff", "ff_p", "cf_p", "freeze_scale", "drop_reward", "clip")]
            + [("min_episode_length", i_), ("unc", f_ * 4)])


class WrapArgs(ctypes.Structure):
    """`rg_wrap_args` of include/rgstep.h (field order and types must match; bind() checks the size)."""

    _fields_ = _wrap_fields()


EXPORTS = [
    "rg_model_create", "rg_model_free", "rg_model_dims", "rg_batch_create", "rg_batch_free", "rg_batch_set_env",
    "rg_batch_copy", "rg_batch_reset", "rg_batch_step", "rg_obs_dim", "rg_debug_size", "rg_lds_bytes", "rg_sync",
    "rg_last_error", "rg_batch_mpr_pair", "rg_batch_copy_rows", "rg_batch_step_ex", "rg_batch_field_ptr", "rg_model_create_on", "rg_model_npair",
    "rg_lds_bytes_cfg", "rg_env_post_step", "rg_post_args_size", "rg_batch_enable_env_params", "rg_prm_layout", "rg_xdata_layout", "rg_batch_set_constants", "rg_batch_items_info",
    "rb_model_create", "rb_model_free", "rb_model_info", "rb_scratch_offset", "rb_batch_create", "rb_batch_free", "rb_batch_reset", "rb_batch_set_env",
    "rb_batch_field_ptr", "rb_batch_step", "rb_batch_step_ex", "rb_env_post_step", "rb_post_args_size", "rb_cube_ops", "rb_batch_step_tcp", "ra_env_post_step", "ra_post_args_size",
    "rg_blob_entry", "rg_model_blob_keys", "rb_model_blob_keys", "rg_compile_mjcf", "rb_compile_mjcf", "rg_compile_mjcf_blob", "rg_blob_free",
    "rb_model_enable_env_params", "rb_prm_layout", "rb_batch_set_action_limits", "ra_env_recipe_step", "ra_recipe_args_size", "rb_tcp_args_size", "rb_multi_begin", "rb_multi_launch",
    "rg_wrap_layout", "rg_wrap_pre_step", "rg_wrap_post_step", "rg_wrap_args_size", "rg_items_per_cu", "rg_kernel_resources",
]
EXPORTS_SETCONST = ["rb_batch_set_constants"]      # include/rgstep_setconst.h (EXPORTS is what include/rgstep.h itself declares)
EXPORTS_ICP = ["ra_env_icp", "ra_icp_args_size"]      # include/rgstep_icp.h
EXPORTS_SYNC_RESET = ["ra_env_param_rows", "ra_param_rows_args_size"]      # include/rgstep_sync_reset.h



class NativeError(RuntimeError):
    pass


def bind(path):
    """Load a build of the C ABI and declare its signatures."""
    if not os.path.exists(path):
        raise NativeError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path
        )
    L = ctypes.CDLL(path)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.rg_model_create.restype = vp
    L.rg_model_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ci]
    L.rg_model_free.argtypes = [vp]
    L.rg_model_create_on.restype = vp
    L.rg_model_create_on.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ci, ctypes.c_char_p, ci]
    L.rg_model_npair.argtypes = [vp]
    L.rg_batch_step_ex.argtypes = [vp, ctypes.POINTER(StepArgs)]
    L.rg_batch_field_ptr.restype = vp
    L.rg_batch_field_ptr.argtypes = [vp, ci, ctypes.POINTER(ci)]
    L.rg_model_dims.argtypes = [vp, ctypes.POINTER(ci)]
    L.rg_batch_create.restype = vp
    L.rg_batch_create.argtypes = [vp, ci, ci]
    L.rg_batch_free.argtypes = [vp]
    L.rg_batch_set_env.argtypes = [vp, ctypes.POINTER(ci), ci, ctypes.POINTER(cf), cf]
    L.rg_batch_copy.argtypes = [vp, ci, vp, ci, ci]
    L.rg_batch_reset.argtypes = [vp]
    L.rg_batch_copy_rows.argtypes = [vp, ci, vp, vp, ci, ci, vp]
    L.rg_batch_step.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.rg_batch_mpr_pair.argtypes = [vp, ci, ci, cf, vp, vp]
    L.rg_obs_dim.argtypes = [vp]
    L.rg_debug_size.restype = ci
    L.rg_lds_bytes.restype = ci
    L.rg_lds_bytes_cfg.restype = ci
    L.rg_lds_bytes_cfg.argtypes = [ci]
    L.rg_items_per_cu.restype = ci
    L.rg_kernel_resources.argtypes = [ci, ctypes.POINTER(ci)]
    L.rg_batch_enable_env_params.argtypes = [vp]
    L.rg_prm_layout.argtypes = [ctypes.POINTER(ci), ci]
    L.rg_xdata_layout.argtypes = [ctypes.POINTER(ci), ci]
    L.rg_env_post_step.argtypes = [vp, ctypes.POINTER(PostArgs), vp]
    L.rg_post_args_size.restype = ci
    if L.rg_post_args_size() != ctypes.sizeof(PostArgs):
        raise NativeError("rg_post_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.rg_wrap_layout.argtypes = [ctypes.POINTER(WrapDims), ctypes.POINTER(WrapLay)]
    L.rg_wrap_pre_step.argtypes = [ctypes.POINTER(WrapArgs), vp]
    L.rg_wrap_post_step.argtypes = [ctypes.POINTER(WrapArgs), vp]
    L.rg_wrap_args_size.restype = ci
    if L.rg_wrap_args_size() != ctypes.sizeof(WrapArgs):
        raise NativeError("rg_wrap_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.rg_batch_set_constants.argtypes = [vp, vp, vp]
    L.rg_batch_items_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    L.rb_model_create.restype = vp
    L.rb_model_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ci]
    L.rb_model_free.argtypes = [vp]
    L.rb_model_info.argtypes = [vp, ctypes.POINTER(ci), ci]
    L.rg_blob_entry.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ci, ctypes.c_char_p, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_uint)]
    L.rg_model_blob_keys.argtypes = [vp, ctypes.c_char_p, ci]
    L.rb_model_blob_keys.argtypes = [vp, ctypes.c_char_p, ci]
    L.rg_compile_mjcf.restype = vp
    L.rg_compile_mjcf.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci]
    L.rb_compile_mjcf.restype = vp
    L.rb_compile_mjcf.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ci]
    L.rg_compile_mjcf_blob.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ci, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p, ci]
    L.rg_blob_free.argtypes = [vp]
    L.rb_model_enable_env_params.argtypes = [vp]
    L.rb_prm_layout.argtypes = [vp, ctypes.POINTER(ci), ci]
    L.rb_scratch_offset.argtypes = [vp, ci]
    L.rb_batch_create.restype = vp
    L.rb_batch_create.argtypes = [vp, ci]
    L.rb_batch_free.argtypes = [vp]
    L.rb_batch_reset.argtypes = [vp]
    L.rb_batch_set_env.argtypes = [vp, ci, ci, ci, ctypes.POINTER(cf)]
    L.rb_batch_set_action_limits.argtypes = [vp, cf, ctypes.c_uint]
    L.rb_batch_field_ptr.restype = vp
    L.rb_batch_field_ptr.argtypes = [vp, ci, ctypes.POINTER(ci)]
    L.rb_batch_step.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    L.rb_batch_step_ex.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, vp]
    L.rb_batch_step_tcp.argtypes = [vp, vp, vp, vp, ctypes.POINTER(RbTcpArgs), ci, ci, vp]
    L.rb_multi_launch.argtypes = [vp]
    L.rb_batch_set_constants.argtypes = [vp, vp, vp]
    L.rb_tcp_args_size.restype = ci
    if L.rb_tcp_args_size() != ctypes.sizeof(RbTcpArgs):
        raise NativeError("rb_tcp_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.ra_env_post_step.argtypes = [vp, vp, ctypes.POINTER(RaPostArgs), vp]
    L.ra_post_args_size.restype = ci
    if L.ra_post_args_size() != ctypes.sizeof(RaPostArgs):
        raise NativeError("ra_post_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.ra_env_icp.argtypes = [vp, ctypes.POINTER(RaIcpArgs), vp]
    L.ra_icp_args_size.restype = ci
    if L.ra_icp_args_size() != ctypes.sizeof(RaIcpArgs):
        raise NativeError("ra_icp_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.ra_env_recipe_step.argtypes = [vp, vp, ctypes.POINTER(RaRecipeArgs), vp]
    L.ra_recipe_args_size.restype = ci
    if L.ra_recipe_args_size() != ctypes.sizeof(RaRecipeArgs):
        raise NativeError("ra_recipe_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.ra_env_param_rows.argtypes = [vp, ctypes.POINTER(RaParamRowsArgs), vp]
    L.ra_param_rows_args_size.restype = ci
    if L.ra_param_rows_args_size() != ctypes.sizeof(RaParamRowsArgs):
        raise NativeError("ra_param_rows_args layout mismatch between include/rgstep_sync_reset.h and robogym_amd/_native.py")
    L.rb_env_post_step.argtypes = [vp, ctypes.POINTER(RbPostArgs), vp]
    L.rb_post_args_size.restype = ci
    if L.rb_post_args_size() != ctypes.sizeof(RbPostArgs):
        raise NativeError("rb_post_args layout mismatch between include/rgstep.h and robogym_amd/_native.py")
    L.rb_cube_ops.argtypes = [vp, ci, vp, vp, ci, vp, vp]
    L.rg_sync.argtypes = [vp]
    L.rg_last_error.restype = ctypes.c_char_p
    return L


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = bind(LIB_PATH)
    return _LIB


def check(L, rc, what):
    if rc != 0:
        raise NativeError("%s failed: %s" % (what, L.rg_last_error().decode()))


RG_FLAG_MPR_PLANE_DEPTH = 16   # rg_step_args.flags bit 4 (include/rgstep.h)
RG_FLAG_SENSORS = 32           # bit 5: evaluate data.sensordata (the last state-less forward runs in full)
RG_FLAG_SEPARATE_FORWARD_SUBSTITUTION = 64   # bit 6: test hook (include/rgstep.h)
RG_FLAG_SUBSTEP_ITEMS = 128    # bit 7: substep-granular dispatch of a rollout launch (rg_step_items_kernel)
RG_FLAG_CAPACITY_TEST_HOOK = 512   # bit 9: test hook (include/rgstep.h)
RG_FLAG_DESERT_QUEUE0 = 1024       # bit 10: test hook: the substep-granular dispatch leaves its queue 0 unserved (the fallback must complete those envs)
RG_STATUS_SCHED = 64
RG_FLAG_RESUME = 256           # bit 8: active_dev is a redo array: entry - 1 = first substep still to do

RB_PRM_NAMES = ["gravity", "dof_damping", "dof_armature", "dof_frictionloss", "dof_invweight0", "jnt_stiffness", "jnt_margin", "jnt_range", "body_pos", "body_mass", "body_inertia",
                "body_invweight0", "actuator_gainprm", "actuator_forcerange", "actuator_ctrlrange", "geom_pos", "geom_margin", "geom_gap", "geom_friction", "geom_solref", "geom_solimp",
                "tendon_range", "tendon_invweight0", "timestep", "xfrc_applied", "site_pos", "geom_scale"]      # rb_types.h RB_P_* order (rb_prm_layout)
PRM_NAMES = ["row", "gravity", "timestep", "dof_damping", "dof_armature", "dof_frictionloss", "dof_invweight0", "body_mass", "body_inertia", "body_invweight0",
             "jnt_range", "tendon_range", "tendon_invweight0", "actuator_gainprm", "actuator_ctrlrange", "actuator_forcerange", "geom_friction", "xfrc_applied", "site_pos", "geom_scale", "jnt_margin", "geom_solref", "geom_solimp"]


def prm_layout(L):
    """rg_prm_layout as a dict: 'row' -> floats per env, then field -> offset."""
    buf = (ctypes.c_int * 32)()
    n = L.rg_prm_layout(buf, 32)
    assert n == len(PRM_NAMES), "rg_prm_layout and robogym_amd/_native.py disagree"
    return {k: int(buf[i]) for i, k in enumerate(PRM_NAMES)}
