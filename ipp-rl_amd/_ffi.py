"""
ctypes binding of the C-ABI in include/ipp_engine.h (lib/libipp_hip.so, built by csrc/Makefile).

There is no CPU fallback: if the HIP library is missing or does not load, importing the engine fails
loudly (build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C ipp-rl_amd/csrc``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IPP_HIP_LIB") or os.path.join(_HERE, "lib", "libipp_hip.so")  # override: A/B builds only

IPP_DENSE, IPP_FACTOR = 0, 1
IPP_GRF_GEN_CONV, IPP_GRF_GEN_DFT, IPP_GRF_GEN_HARTLEY, IPP_GRF_GEN_FFT = 0, 1, 2, 3
IPP_PRIOR_MATERN32, IPP_PRIOR_MATERN12, IPP_PRIOR_MATERN52, IPP_PRIOR_RBF = 0, 1, 2, 3
IPP_COV_ONLY, IPP_PREDICT_ONLY, IPP_ADAPTIVE, IPP_USE_FLIGHT_TIME, IPP_GIVEN_OBSERVATION, IPP_UPDATE_PREV = 1, 2, 4, 8, 16, 32
IPP_BUDGET, IPP_RESET_ON_DONE = 64, 128
IPP_BUDGET_STREAM = 3 << 40
IPP_PRIOR_STREAM = 11 << 40  # Philox subsequence base of the per-episode priors (ipp_set_budget_prior, vec_env.start_prior)
IPP_CMA_STREAM = 9 << 40  # Philox subsequence base of the CMA-ES planner's normals (planning/vec_cmaes.py)
IPP_CMA_MAX_DIM, IPP_CMA_MAX_LAMBDA = 48, 64
# Philox subsequence bases of the self-play draws (ipp_selfplay_record / _commit, ipp_replay_gather)
IPP_SP_ACTION_STREAM, IPP_SP_INIT_STREAM, IPP_SP_TIE_STREAM, IPP_SP_ARGMAX_STREAM, IPP_REPLAY_STREAM = (4 << 40, 5 << 40, 6 << 40, 7 << 40,
                                                                                                       8 << 40)
IPP_PVNET_SGD_SCRATCH = 1024  # doubles of scratch that always suffice for ipp_pvnet_sgd_step (one per workgroup of its first launch)
IPP_REPLAY_SCAN_TILE = 2048  # ring rows per workgroup of ipp_replay_mass's prefix sum (its scratch: one double per tile)
IPP_FIELD_GRF, IPP_FIELD_HOTSPOT, IPP_FIELD_SPLIT = 0, 1, 2
STATUS_OK, STATUS_CHOL_FALLBACK, STATUS_NOT_PD, STATUS_RANK_FULL, STATUS_BAD_FOOTPRINT = 0, 1, 2, 3, 4
IPP_MAX_MEAS = 25
ABI_VERSION = 17
AB_MIN_ABI = 13  # oldest library tools/ab_kernels.py may load under IPP_AB_OLD_LIB (v14 added the ipp_arena_* calls, v15 the budget ledger calls, v16 the *_prior calls, v17 the field calls; ipp_feature_planes, ipp_mcts_plane_entries and the prioritised-replay calls (ipp_replay_priority_reset .. _update) were added later WITHOUT a bump -- tests pin 17 -- so an older v17 library lacks them and the A/B loader leaves them unbound; nothing else)
IPP_ARENA_HIPMALLOC, IPP_ARENA_VMM = 0, 1


class IppConfig(C.Structure):
    _fields_ = [
        ("x_dim", C.c_int32), ("y_dim", C.c_int32),
        ("resolution", C.c_double),
        ("tan_half_fov_x", C.c_double), ("tan_half_fov_y", C.c_double),
        ("rf_altitude", C.c_double),
        ("coeff_a", C.c_double), ("coeff_b", C.c_double),
        ("signal_variance", C.c_double), ("length_scale", C.c_double),
        ("max_v", C.c_double), ("max_a", C.c_double),
        ("value_threshold", C.c_double), ("interval_factor", C.c_double),
        ("cluster_radius", C.c_double),
        ("state_repr", C.c_int32), ("capacity", C.c_int32), ("rank_cap", C.c_int32), ("max_batch", C.c_int32),
        ("max_measurements", C.c_int32), ("tile_threads", C.c_int32), ("window_rows", C.c_int32), ("score_scratch", C.c_int32), ("node_capacity", C.c_int32), ("fixed_prior", C.c_int32),
    ]


class IppInfo(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_cells", C.c_int32), ("n_pad", C.c_int32), ("tile_threads", C.c_int32),
        ("n_tiles", C.c_int32), ("meas_cap", C.c_int32), ("fp_cap", C.c_int32), ("window_rows", C.c_int32),
        ("arena_bytes", C.c_uint64), ("cov_slot_bytes", C.c_uint64), ("step_lds_bytes", C.c_uint64),
        ("fused_step", C.c_int32), ("patch_layout", C.c_int32), ("patch_waves", C.c_int32), ("patch_big_min_items", C.c_int32),
        ("patch_split_min_items", C.c_int32), ("patch_two_wave_min_items", C.c_int32),
    ]


class IppFieldRecord(C.Structure):
    """ipp_field_record: cell (y, x) = inside if it lies in rect[0] or rect[1] ({y0, y1, x0, x1}, half-open), else outside."""
    _fields_ = [("inside", C.c_double), ("outside", C.c_double), ("rect", (C.c_int32 * 4) * 2)]


class IppPlaneSpec(C.Structure):
    _fields_ = [
        ("history", C.c_int32), ("use_fov", C.c_int32), ("use_costs", C.c_int32), ("adaptive", C.c_int32),
        ("use_flight_time", C.c_int32), ("reserved", C.c_int32), ("min_altitude", C.c_double), ("max_altitude", C.c_double),
    ]


class IppStepItem(C.Structure):
    _fields_ = [
        ("env", C.c_int32), ("dst", C.c_int32), ("rank_before", C.c_int32), ("status", C.c_int32),
        ("xl", C.c_int32), ("xr", C.c_int32), ("yu", C.c_int32), ("yd", C.c_int32),
        ("rf", C.c_int32), ("m", C.c_int32), ("f", C.c_int32), ("pad", C.c_int32),
        ("cost", C.c_double), ("noise_var", C.c_double),
        ("S", C.c_double * (IPP_MAX_MEAS * IPP_MAX_MEAS)),
        ("Linv", C.c_double * (IPP_MAX_MEAS * IPP_MAX_MEAS)),
        ("z", C.c_double * IPP_MAX_MEAS),
        ("y", C.c_double * IPP_MAX_MEAS),
    ]


_P = C.c_void_p


class IppMctsTables(C.Structure):
    """ipp_mcts_tables (include/ipp_engine.h): dimensions, search constants and the [dev] buffers of a device-side tree search."""
    _fields_ = [
        ("roots", C.c_int32), ("kmax", C.c_int32), ("nodes_per_root", C.c_int32), ("dev_per_root", C.c_int32),
        ("table_size", C.c_int32), ("max_depth", C.c_int32), ("wave", C.c_int32), ("horizon", C.c_int32),
        ("grid_w", C.c_int32), ("grid_h", C.c_int32), ("n_levels", C.c_int32), ("n_off", C.c_int32),
        ("num_actions", C.c_int32), ("use_flight_time", C.c_int32), ("tie_break", C.c_int32), ("device", C.c_int32),
        ("res", C.c_double), ("max_dist", C.c_double), ("gamma", C.c_double), ("puct_init", C.c_double),
        ("puct_base", C.c_double), ("fpf", C.c_double), ("vmax", C.c_double), ("amax", C.c_double),
        ("actions", _P), ("cell_action", _P), ("off_x", _P), ("off_y", _P),
        ("zkey", _P), ("uniform_ps", _P), ("t_idx", _P), ("t_ps", _P),
        ("t_nsa", _P), ("t_qsa", _P), ("t_num", _P), ("t_child", _P),
        ("n_k", _P), ("n_ns", _P), ("n_flags", _P), ("n_hash", _P),
        ("n_value", _P), ("n_devpath", _P), ("root_count", _P), ("dev_count", _P),
        ("h_keys", _P), ("h_vals", _P), ("p_node", _P), ("p_k", _P),
        ("p_cost", _P), ("p_len", _P), ("leaf", _P), ("pend_node", _P),
        ("pend_depth", _P), ("pend_sim", _P), ("pend_prev", _P), ("pend_budget", _P),
        ("pend_count", _P), ("rq_root", _P), ("rq_parent", _P), ("rq_k", _P),
        ("rq_child", _P), ("rq_newdev", _P), ("rq_cost", _P), ("rq_prev", _P),
        ("rq_action", _P), ("rq_count", _P), ("ts_paths", _P), ("ts_reward", _P),
        ("ts_status", _P), ("err", _P),
        ("puct_c", _P), ("sqrt_ns1", _P), ("ns_table_n", C.c_int64),
        ("root_base", C.c_int32), ("dev_base", C.c_int32), ("scratch_base", C.c_int32), ("reserved0", C.c_int32),
    ]


class IppSelfPlay(C.Structure):
    """ipp_selfplay (include/ipp_engine.h): the batch's self-play state and sample ring, [dev] pointers."""
    _fields_ = [
        ("num_envs", C.c_int32), ("slots", C.c_int32), ("kmax", C.c_int32), ("num_actions", C.c_int32),
        ("horizon", C.c_int32), ("temp_threshold", C.c_int32), ("temp_zero", C.c_int32), ("random_init", C.c_int32),
        ("device", C.c_int32), ("reserved", C.c_int32), ("gamma", C.c_double), ("seed", C.c_uint64), ("row_offset", C.c_int64),
        ("actions", _P), ("budget", _P), ("depth", _P), ("episode", _P), ("done", _P), ("prev", _P), ("reward", _P),
        ("ep_len", _P), ("forced", _P), ("tie_u", _P), ("episode_value", _P), ("action", _P), ("action_idx", _P),
        ("r_policy", _P), ("r_idx", _P), ("r_value", _P), ("r_reward", _P), ("r_flags", _P),
    ]


class IppSelfPlayIter(C.Structure):
    """ipp_selfplay_iter (include/ipp_engine.h): the cap, the per-env counters and the row tags of a self-play iteration, [dev] pointers."""
    _fields_ = [
        ("iteration", C.c_int32), ("episode_cap", C.c_int32),
        ("iter_episodes", _P), ("r_iter", _P), ("examples", _P), ("value_sum", _P),
    ]


class IppReplayCompact(C.Structure):
    """ipp_replay_compact (include/ipp_engine.h): the compact replay ring's rows and per-env archive bookkeeping, [dev] pointers."""
    _fields_ = [
        ("history", C.c_int32), ("archive_episodes", C.c_int32),
        ("r_entries", _P), ("r_mean", _P), ("r_episode", _P), ("episodes", _P), ("last_rank", _P), ("evicted", _P),
    ]


IPP_SLOT_COLUMNS, IPP_SLOT_MAPS = 1, 2
IPP_SLOT_OK, IPP_SLOT_BAD_ID, IPP_SLOT_RANK, IPP_SLOT_BAD_RECORD = 0, 1, 2, 3


class IppSlotLayout(C.Structure):
    """ipp_slot_layout (include/ipp_engine.h): what a packed slot record depends on; engines exchange slots iff every field is equal."""
    _fields_ = [
        ("format", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("N", C.c_int32), ("Npad", C.c_int32),
        ("pw", C.c_int32), ("ph", C.c_int32), ("pstride", C.c_int32), ("window_rows", C.c_int32), ("tile_cells", C.c_int32),
        ("prior_kind", C.c_int32), ("reserved", C.c_int32),
    ]


class IppIterTotals(C.Structure):
    """The 32-byte record of ipp_selfplay_iter_totals."""
    _fields_ = [("episodes_kept", C.c_int64), ("envs_at_cap", C.c_int64), ("examples", C.c_int64), ("value_sum", C.c_double)]


class IppPlay(C.Structure):
    """ipp_play (include/ipp_engine.h): the deployment planner's / arena's per-env decision and game bookkeeping, [dev] pointers."""
    _fields_ = [
        ("num_envs", C.c_int32), ("workers", C.c_int32), ("kmax", C.c_int32), ("num_actions", C.c_int32),
        ("games_per_env", C.c_int32), ("tie_rule", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
        ("gamma", C.c_double), ("seed", C.c_uint64), ("row_offset", C.c_int64),
        ("actions", _P), ("budget", _P), ("depth", _P), ("episode", _P), ("done", _P), ("prev", _P), ("reward", _P),
        ("ret", _P), ("steps", _P), ("games", _P), ("forced", _P), ("tie_u", _P), ("action", _P), ("action_idx", _P),
        ("game_value", _P), ("game_steps", _P), ("ensemble", _P),
    ]

class IppRollout(C.Structure):
    """ipp_rollout (include/ipp_engine.h): dimensions, policy constants and the [dev] buffers of n device rollouts."""
    _fields_ = [
        ("n", C.c_int32), ("kmax", C.c_int32), ("max_depth", C.c_int32), ("gcb", C.c_int32),
        ("grid_w", C.c_int32), ("grid_h", C.c_int32), ("n_levels", C.c_int32), ("half", C.c_int32),
        ("node_base", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32),
        ("resolution", C.c_double), ("radius", C.c_double), ("gamma", C.c_double), ("epsilon", C.c_double),
        ("vmax", C.c_double), ("amax", C.c_double),
        ("levels", _P), ("u", _P),
        ("root", _P), ("path", _P), ("plen", _P), ("cur", _P), ("charge_from", _P), ("budget", _P), ("depth_left", _P),
        ("value", _P), ("disc", _P), ("live", _P), ("flag", _P),
        ("cand", _P), ("reward", _P), ("cost", _P), ("status", _P), ("action", _P), ("new_id", _P),
        ("step_reward", _P), ("step_status", _P), ("pick_idx", _P),
    ]


IPP_ROLLOUT_RUNNING, IPP_ROLLOUT_END, IPP_ROLLOUT_NO_ACTION, IPP_ROLLOUT_RANK_FULL = 0, 1, 2, 3
IPP_ROLLOUT_ERR_FOOTPRINT, IPP_ROLLOUT_ERR_NAN, IPP_ROLLOUT_ERR_STEP = 4, 5, 6


class IppCtree(C.Structure):
    """ipp_ctree (include/ipp_engine.h): dimensions, the UCT constant and the [dev] tables of a device-side classic tree search."""
    _fields_ = [
        ("roots", C.c_int32), ("cap", C.c_int32), ("horizon", C.c_int32), ("thr_len", C.c_int32),
        ("tree_node_base", C.c_int32), ("device", C.c_int32), ("c", C.c_double),
        ("thr", _P), ("root_slot", _P), ("root_wp", _P), ("root_budget", _P), ("tie_u", _P),
        ("parent", _P), ("dev", _P), ("plen", _P), ("path", _P), ("action", _P), ("visits", _P), ("value_sum", _P), ("edge_reward", _P),
        ("count", _P), ("err", _P), ("t_len", _P), ("t_slot", _P), ("leaf_kind", _P), ("leaf_budget", _P), ("leaf_depth", _P),
    ]


class IppBaseline(C.Structure):
    """ipp_baseline (include/ipp_engine.h): kind, geometry, cost mode and the [dev] arrays of one baseline decision per env."""
    _fields_ = [
        ("n", C.c_int32), ("kind", C.c_int32), ("table_len", C.c_int32), ("grid_w", C.c_int32), ("grid_h", C.c_int32),
        ("n_levels", C.c_int32), ("adaptive", C.c_int32), ("use_flight_time", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
        ("resolution", C.c_double), ("step_size", C.c_double), ("max_v", C.c_double), ("max_a", C.c_double),
        ("low", C.c_double * 3), ("high", C.c_double * 3), ("seed", C.c_uint64), ("row_offset", C.c_int64),
        ("table", _P), ("levels", _P), ("uniforms", _P), ("prev", _P), ("budget", _P), ("episode", _P),
        ("cursor", _P), ("seen_episode", _P), ("decision", _P), ("start_budget", _P), ("action", _P), ("has", _P),
    ]


IPP_BASELINE_STREAM = 10 << 40  # Philox subsequence base of the random baselines' uniforms (planning/vec_baselines.py)
IPP_BASELINE_LAWNMOWER, IPP_BASELINE_SPIRAL, IPP_BASELINE_RANDOM_DISCRETE, IPP_BASELINE_RANDOM_CONTINUOUS = 0, 1, 2, 3
IPP_BASELINE_TRIALS = 101
IPP_CURVE_VALUES, IPP_CURVE_POINT = 8, 9

IPP_CTREE_TERMINAL, IPP_CTREE_ROLLOUT, IPP_CTREE_EXPAND = 0, 1, 2
IPP_CTREE_ERR_RANGE, IPP_CTREE_ERR_SELECT, IPP_CTREE_ERR_PICK, IPP_CTREE_ERR_STEP, IPP_CTREE_ERR_FULL, IPP_CTREE_ERR_ROLLOUT = 1, 2, 3, 4, 5, 6

# name -> (restype, argtypes); exactly the symbols include/ipp_engine.h declares
PROTOTYPES = {
    "ipp_abi_version": (C.c_int, []),
    "ipp_min_window_rows": (C.c_int, [_P, _P]),
    "ipp_last_error": (C.c_char_p, []),
    "ipp_engine_arena_bytes": (C.c_int, [C.POINTER(IppConfig), C.POINTER(C.c_uint64)]),
    "ipp_engine_create": (C.c_int, [C.POINTER(IppConfig), C.c_int, _P, C.c_uint64, C.POINTER(_P)]),
    "ipp_min_window_rows_prior": (C.c_int, [C.POINTER(IppConfig), C.c_int32, _P]),
    "ipp_engine_arena_bytes_prior": (C.c_int, [C.POINTER(IppConfig), C.c_int32, C.POINTER(C.c_uint64)]),
    "ipp_engine_create_prior": (C.c_int, [C.POINTER(IppConfig), C.c_int32, C.c_int, _P, C.c_uint64, C.POINTER(_P)]),
    "ipp_engine_destroy": (C.c_int, [_P]),
    "ipp_engine_info": (C.c_int, [_P, C.POINTER(IppInfo)]),
    "ipp_grf_generator": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ipp_reset": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    "ipp_reset_episode": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "ipp_score_actions": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_uint32, _P, _P, _P]),
    "ipp_score_actions_envs": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, _P]),
    "ipp_score_actions_envs_scratch_bytes": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    "ipp_state_plane": (C.c_int, [_P, C.c_int32, _P, C.c_uint32, _P, _P]),
    "ipp_feature_planes": (C.c_int, [_P, C.POINTER(IppPlaneSpec), _P, C.c_int32, _P, _P, _P, _P]),
    "ipp_mcts_plane_entries": (C.c_int, [C.POINTER(IppMctsTables), _P, _P, _P, _P, C.c_int32, C.c_double, C.c_int32, _P, _P, _P]),
    "ipp_tree_step": (C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, C.c_uint32, _P, _P, _P]),
    "ipp_tree_read_diag": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_mcts_select": (C.c_int, [C.POINTER(IppMctsTables), _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _P]),
    "ipp_mcts_steps": (C.c_int, [_P, C.POINTER(IppMctsTables), C.c_int32, C.c_int32, C.c_uint32, _P]),
    "ipp_mcts_expand": (C.c_int, [C.POINTER(IppMctsTables), _P, _P, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_uint64, _P]),
    "ipp_mcts_backup": (C.c_int, [C.POINTER(IppMctsTables), C.c_int32, _P]),
    "ipp_mcts_policy": (C.c_int, [C.POINTER(IppMctsTables), _P, C.c_double, C.c_int32, _P, _P, _P, _P]),
    "ipp_tree_score_actions": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, _P, C.c_uint32, _P, _P, _P]),
    # (added without an ABI bump: no struct changes layout, every existing call answers as before until it is set)
    "ipp_set_grf_rows": (C.c_int, [_P, C.c_int32]),
    "ipp_generate_grf": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "ipp_generate_grf_rows": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_uint64, C.c_uint64, _P, _P]),
    "ipp_generate_grf_groups": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_uint64, C.c_uint64, _P, _P]),
    "ipp_generate_grf_refill": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int64, C.c_uint64, C.c_uint64, _P]),
    "ipp_generate_field_groups": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_uint64, C.c_uint64, _P, _P]),
    "ipp_generate_field_refill": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int64, C.c_uint64, C.c_uint64, _P]),
    "ipp_fill_fields": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P]),
    "ipp_set_budget": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_double, C.c_int32, C.c_int32, C.c_uint64, C.c_int64]),
    "ipp_set_budget_prior": (C.c_int, [_P, C.c_int32]),
    "ipp_step": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, _P]),
    "ipp_step_autoreset": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "ipp_step_parts": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    "ipp_observe": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "ipp_set_uav": (C.c_int, [_P, C.c_double, C.c_double]),
    "ipp_set_adaptive": (C.c_int, [_P, C.c_double, C.c_double]),
    "ipp_set_item_order": (C.c_int, [_P, _P, C.c_int32]),
    "ipp_set_reset_prior": (C.c_int, [_P, _P]),
    "ipp_fork": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    # (slot export and import, csrc/k_slots.h: added without an ABI bump, nothing existing changes layout)
    "ipp_slots_layout": (C.c_int, [_P, C.POINTER(IppSlotLayout)]),
    "ipp_slots_plan": (C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, _P, _P]),
    "ipp_slots_export": (C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, _P, _P]),
    "ipp_slots_import": (C.c_int, [_P, _P, C.c_int32, C.c_uint32, _P, _P, _P, _P]),
    "ipp_read_mean": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_read_diag": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_read_gt": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_read_cov_dense": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_read_rank": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32), _P]),
    "ipp_read_ranks": (C.c_int, [_P, _P, _P]),
    "ipp_read_prior": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "ipp_write_mean": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_write_gt": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_write_cov_dense": (C.c_int, [_P, C.c_int32, _P, _P]),
    "ipp_metrics": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "ipp_fill_normal": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P]),
    "ipp_fill_normal_rows": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, C.c_uint64, C.c_uint64, _P]),
    "ipp_probe_stream_pair": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(C.c_double)]),
    "ipp_arena_alloc": (C.c_int, [C.c_int, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(_P)]),
    "ipp_arena_free": (C.c_int, [_P]),
    "ipp_arena_retired_bytes": (C.c_int, [C.POINTER(C.c_uint64)]),
    "ipp_arena_trim": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "ipp_arena_latency": (C.c_int, [C.c_int, _P, C.c_uint64, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    "ipp_arena_probe": (C.c_int, [C.c_int, _P, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    "ipp_debug_capture": (C.c_int, [_P, C.c_int32]),
    "ipp_debug_step_item": (C.c_int, [_P, C.c_int32, C.POINTER(IppStepItem), _P]),
    "ipp_streamed_bytes": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int32, _P]),
    "ipp_streamed_bytes_detail": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int32, _P]),
    "ipp_streamed_bytes_needed": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "ipp_profile_enable": (C.c_int, [_P, C.c_int32]),
    "ipp_profile_read": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
    "ipp_profile_read_busy": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
    "ipp_selfplay_record": (C.c_int, [C.POINTER(IppSelfPlay), C.c_int64, _P, _P, _P, _P, _P]),
    "ipp_selfplay_commit": (C.c_int, [C.POINTER(IppSelfPlay), C.c_int64, _P]),
    "ipp_replay_gather": (C.c_int, [C.POINTER(IppSelfPlay), C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_uint64, C.c_uint64,
                                    _P, _P, _P, _P, _P, _P, _P, _P]),
    "ipp_replay_priority_reset": (C.c_int, [C.POINTER(IppSelfPlay), _P, _P, _P]),
    "ipp_replay_mass": (C.c_int, [C.POINTER(IppSelfPlay), _P, C.c_double, _P, _P, C.c_uint64, _P]),
    "ipp_replay_draw_per": (C.c_int, [C.POINTER(IppSelfPlay), _P, _P, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_uint64, C.c_uint64,
                                      _P, _P, _P]),
    "ipp_replay_gather_rows": (C.c_int, [C.POINTER(IppSelfPlay), C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ipp_replay_priority_update": (C.c_int, [C.POINTER(IppSelfPlay), _P, _P, _P, C.c_int32, _P]),
    # (self-play iterations and the off-policy window, csrc/k_selfplay.h and csrc/k_learn.h: added without an ABI bump as well)
    "ipp_selfplay_commit_iter": (C.c_int, [C.POINTER(IppSelfPlay), C.c_int64, C.POINTER(IppSelfPlayIter), _P]),
    "ipp_selfplay_iter_totals": (C.c_int, [C.POINTER(IppSelfPlay), C.POINTER(IppSelfPlayIter), _P, _P]),
    "ipp_replay_priority_reset_window": (C.c_int, [C.POINTER(IppSelfPlay), _P, C.c_int32, C.c_int32, _P, _P, _P]),
    # (the compact replay ring, csrc/k_replay_compact.h: added without an ABI bump as well)
    "ipp_replay_record_compact": (C.c_int, [_P, C.POINTER(IppSelfPlay), C.POINTER(IppReplayCompact), C.c_int64, _P, _P]),
    "ipp_selfplay_archive": (C.c_int, [_P, C.POINTER(IppSelfPlay), C.POINTER(IppReplayCompact), _P]),
    "ipp_replay_compact_planes": (C.c_int, [_P, C.POINTER(IppSelfPlay), C.POINTER(IppReplayCompact), C.POINTER(IppPlaneSpec), C.c_int32,
                                            C.c_int32, _P, _P, _P, _P, _P, _P]),
    # (the deployment planner's and the arena's calls, csrc/k_play.h: added without an ABI bump, nothing existing changes layout)
    "ipp_play_pick": (C.c_int, [C.POINTER(IppPlay), _P, _P, _P, _P]),
    "ipp_play_tally": (C.c_int, [C.POINTER(IppPlay), _P]),
    "ipp_play_totals": (C.c_int, [C.POINTER(IppPlay), _P, _P]),
    # (ops: an array of ipp_pvnet_op, planning/mcts_zero/networks.py IppPvnetOp)
    "ipp_pvnet_create": (C.c_int, [_P, C.c_int32, _P, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "ipp_pvnet_set_weights": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "ipp_pvnet_forward": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, _P, _P]),
    "ipp_pvnet_destroy": (C.c_int, [_P]),
    # (the trainer's calls, csrc/k_train.h: added without an ABI bump, like the prioritised-replay calls)
    "ipp_pvnet_loss": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                 _P, _P, _P, _P, C.c_int32, _P]),
    "ipp_pvnet_sgd_step": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, _P, _P, C.c_uint64,
                                     C.c_int32, _P]),
    # (the batched CMA-ES planner's calls, csrc/k_cmaes.h: bare buffers, no handle; added without an ABI bump as well)
    "ipp_cma_state_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_uint64)]),
    "ipp_cma_init": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "ipp_cma_ask": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    "ipp_cma_plan": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                               C.c_int32, C.c_double, C.c_double, _P, _P, _P, _P, _P, C.c_int32, _P]),
    "ipp_cma_objective": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "ipp_cma_tell": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
    # (classic MCTS for a batch, csrc/k_rollout.h: added without an ABI bump as well)
    "ipp_tree_score_nodes": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, _P]),
    "ipp_tree_score_nodes_scratch_bytes": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    "ipp_rollout_candidates": (C.c_int, [C.POINTER(IppRollout), _P]),
    "ipp_rollout_pick": (C.c_int, [C.POINTER(IppRollout), C.c_int32, _P]),
    "ipp_rollout_advance": (C.c_int, [C.POINTER(IppRollout), _P]),
    "ipp_rollout_run": (C.c_int, [_P, C.POINTER(IppRollout), _P, C.c_uint64, _P]),
    # (the classic tree search's tables, csrc/k_ctree.h: added without an ABI bump as well)
    "ipp_ctree_descend": (C.c_int, [C.POINTER(IppCtree), C.POINTER(IppRollout), C.POINTER(IppRollout), _P]),
    "ipp_ctree_attach": (C.c_int, [C.POINTER(IppCtree), C.POINTER(IppRollout), C.POINTER(IppRollout), _P]),
    "ipp_ctree_backup": (C.c_int, [C.POINTER(IppCtree), C.POINTER(IppRollout), _P]),
    "ipp_ctree_best": (C.c_int, [C.POINTER(IppCtree), _P, _P, _P]),
    "ipp_ctree_search": (C.c_int, [_P, C.POINTER(IppCtree), C.POINTER(IppRollout), C.POINTER(IppRollout), _P, C.c_uint64, C.c_int32, C.c_int32,
                                   _P]),
    # (the baseline missions and the comparison curves, csrc/k_baselines.h and csrc/k_curves.h: added without an ABI bump as well)
    "ipp_baseline_act": (C.c_int, [C.POINTER(IppBaseline), _P]),
    "ipp_curve_record": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_double, C.c_double, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    "ipp_curve_extent": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "ipp_curve_resample": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_double, C.c_int32, _P, C.c_int32, _P]),
    "ipp_curve_reduce": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
}

_lib = None


class IppError(RuntimeError):
    pass


def load():
    """Load libipp_hip.so once; raise (never fall back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IppError(
            f"HIP engine library not found at {LIB_PATH}: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # The engine shares the HIP runtime of the process with PyTorch (device memory, streams).  PyTorch's wheel carries
    # its own libamdhip64: it has to be the first HIP runtime the process loads, otherwise the engine binds to
    # /opt/rocm's copy and the process ends up with two runtimes, one of which sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:  # symbol checks on a machine without torch
        pass
    lib = C.CDLL(LIB_PATH)
    # tools/ab_kernels.py may time an OLDER build of the library against this binding (IPP_AB_OLD_LIB=1): only a library whose
    # ABI is at least AB_MIN_ABI (struct layouts and call signatures unchanged since then; newer entry points may be absent
    # and are then not bound) and only when the library is not the in-tree product build -- never a general switch
    lib.ipp_abi_version.restype, lib.ipp_abi_version.argtypes = C.c_int, []
    abi = lib.ipp_abi_version()
    ab_old = bool(os.environ.get("IPP_AB_OLD_LIB")) and bool(os.environ.get("IPP_HIP_LIB")) and AB_MIN_ABI <= abi <= ABI_VERSION
    if abi != ABI_VERSION and not ab_old:
        raise IppError(f"libipp_hip.so ABI {abi} != binding ABI {ABI_VERSION}: rebuild")
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        except AttributeError:
            if ab_old:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise IppError(f"ipp engine error {rc}: {load().ipp_last_error().decode(errors='replace')}")
