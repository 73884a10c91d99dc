"""ctypes binding of the C ABI in ``include/lsm_rollout.h``, ``include/lsm_learner.h``,
``include/lsm_recurrent.h``, ``include/lsm_minibatch_edges.h``, ``include/lsm_gnn.h``,
``include/lsm_policy.h``, ``include/lsm_evaluate.h``, ``include/lsm_loss.h``, ``include/lsm_backward.h``,
``include/lsm_gnn_backward.h``, ``include/lsm_gnn_backward_large.h``, ``include/lsm_gnn_embed_backward.h``,
``include/lsm_optim.h`` and
``include/lsm_train_info.h`` (``liblsm_rollout.so``).

This is the Python stub a maintainer of the reference would add (see
INTEGRATION.md): plain pointers and sizes only, no torch types cross the ABI.
The library is built in-tree by ``lsm.build`` (``hipcc --offload-arch=gfx950``);
if it is missing the import fails loudly -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSM_LIB") or os.path.join(os.path.dirname(_HERE), "csrc", "liblsm_rollout.so")

LSM_DOUBLE_INTEGRATOR, LSM_AIRTAXI = 0, 1
LSM_ACTIONS_INDEX_I32, LSM_ACTIONS_ONEHOT_F32, LSM_ACTIONS_ONEHOT_F64 = 0, 1, 2
(OUT_OBS, OUT_NODE_OBS, OUT_ADJ, OUT_REWARD, OUT_DONE, OUT_RESET_FLAG, OUT_EP_INFO, OUT_INFO,
 OUT_EDGES, OUT_STATE, OUT_DEBUG_STAMPS, OUT_ADJ_MASK, OUT_SHARE_OBS, OUT_MASKS, OUT_ACTIVE_MASKS,
 OUT_COLLISION_FORCE, OUT_DEPARTED, OUT_ADJ_NNZ) = range(18)
NUM_OUT = 18
LSM_SCENARIO_TRAIN, LSM_SCENARIO_LAYOUT, LSM_SCENARIO_DEPARTURES = 0, 1, 2
LSM_RNG_MT19937, LSM_RNG_PHILOX = 0, 1
ADJ_REFERENCE, ADJ_COMPACT = 0, 1
# lsm_config.reward_terms bits: RewardBinaryConfig's optional reward terms (multiagent/config.py:78-83)
REWARD_BITS = {"safety_violation": 1, "potential_conflict": 2, "diff_from_filtered_action": 4, "hj_value": 8}
INFO_FIELDS = ("individual_reward", "min_relative_distance", "Dist_to_goal", "Time_req_to_goal",
               "Num_agent_collisions", "Distance_mean", "Distance_variance", "Dists_traveled",
               "Time_mean", "Time_stddev", "Min_time_to_goal", "Safety filtered", "Safety violated",
               "deconflicting_agent_index", "action_diff", "reached_goal", "position_x", "position_y")

# Every symbol include/lsm_rollout.h declares (checked by tests/test_capi.py).
EXPORTED = ("lsm_create", "lsm_destroy", "lsm_last_error", "lsm_set_value_table", "lsm_set_ttr_table",
            "lsm_bind_output", "lsm_output_bytes", "lsm_reset", "lsm_step", "lsm_num_entities",
            "lsm_node_features", "lsm_obs_dim", "lsm_host_mt_uniforms", "lsm_host_scenario",
            "lsm_set_agent_state", "lsm_edges_workspace_bytes", "lsm_edges_count", "lsm_edges_emit", "lsm_edges_emit_dev",
            "lsm_edges_last_error", "lsm_bind_output_ring", "lsm_select_ring", "lsm_buffer_insert",
            "lsm_buffer_last_error", "lsm_host_rk45_di", "lsm_host_glibc_pow", "lsm_action_errors",
            "lsm_kernel_name", "lsm_reset_layout", "lsm_layout_doubles", "lsm_host_philox_uniforms",
            "lsm_host_philox4x32", "lsm_episode_summary", "lsm_build_id", "lsm_test_set_mt_stage",
            "lsm_create_select", "lsm_edges_scan_emit", "lsm_test_read_value_bounds", "lsm_kernel_name_for")
# Every symbol include/lsm_learner.h declares (checked by tests/test_learner_capi.py).
EXPORTED_LEARNER = ("lsm_buffer_compute_returns", "lsm_host_compute_returns",
                    "lsm_buffer_advantages_workspace_bytes", "lsm_buffer_advantages", "lsm_returns_last_error",
                    "lsm_buffer_gather", "lsm_gather_last_error")
LSM_GATHER_ROWS, LSM_GATHER_COMPACT_ADJ = 0, 1
LSM_GATHER_MAX_FIELDS = 16
# Every symbol include/lsm_recurrent.h declares (checked by tests/test_recurrent_capi.py).
EXPORTED_RECURRENT = ("lsm_buffer_gather_chunks", "lsm_host_gather_chunks", "lsm_buffer_copy_rows",
                      "lsm_recurrent_last_error")
LSM_CHUNK_ROWS, LSM_CHUNK_COMPACT_ADJ, LSM_CHUNK_FIRST_ROW = 0, 1, 2
LSM_CHUNK_MAX_FIELDS = 16
LSM_COPY_MAX = 8
# Every symbol include/lsm_minibatch_edges.h declares (checked by tests/test_mb_edges_capi.py).
EXPORTED_MB_EDGES = ("lsm_mb_edges_workspace_bytes", "lsm_mb_edges_count", "lsm_mb_edges_emit", "lsm_host_mb_edges",
                     "lsm_mb_edges_last_error")
LSM_MB_INDICES, LSM_MB_CHUNKS = 0, 1
# Every symbol include/lsm_gnn.h declares (checked by tests/test_gnn_capi.py).
EXPORTED_GNN = ("lsm_gnn_weights_floats", "lsm_gnn_forward", "lsm_host_gnn_forward", "lsm_gnn_last_error",
                "lsm_gnn_plan")
LSM_GNN_NODE, LSM_GNN_GLOBAL_MEAN, LSM_GNN_GLOBAL_MAX, LSM_GNN_GLOBAL_ADD = 0, 1, 2, 3
# Every symbol include/lsm_policy.h declares (checked by tests/test_policy_capi.py).
EXPORTED_POLICY = ("lsm_head_weights_floats", "lsm_head_forward", "lsm_host_head_forward", "lsm_policy_last_error",
                   "lsm_head_plan")
LSM_HEAD_ACTOR, LSM_HEAD_CRITIC = 0, 1
LSM_HEAD_PLAN_FORWARD, LSM_HEAD_PLAN_EVALUATE, LSM_HEAD_PLAN_BACKWARD = 0, 1, 2
LSM_HEAD_PLAN_MAX_JOBS = 17
# Every symbol include/lsm_evaluate.h declares (checked by tests/test_evaluate_capi.py).
EXPORTED_EVALUATE = ("lsm_head_evaluate_scratch_bytes", "lsm_head_evaluate", "lsm_host_head_evaluate")
# Every symbol include/lsm_loss.h declares (checked by tests/test_loss_capi.py).
EXPORTED_LOSS = ("lsm_ppo_loss_scratch_bytes", "lsm_ppo_loss", "lsm_host_ppo_loss", "lsm_loss_last_error")
LSM_LOSS_GROUP = 256
# Every symbol include/lsm_backward.h declares (checked by tests/test_heads_backward_capi.py).
EXPORTED_BACKWARD = ("lsm_head_backward_workspace_bytes", "lsm_head_backward", "lsm_host_head_backward")
LSM_BWD_SLAB = 2048
# Every symbol include/lsm_gnn_backward.h declares (checked by tests/test_gnn_backward_capi.py).
EXPORTED_GNN_BACKWARD = ("lsm_gnn_backward_workspace_bytes", "lsm_gnn_backward", "lsm_host_gnn_backward",
                         "lsm_gnn_backward_plan", "lsm_gnn_backward_last_error")
LSM_GNN_BWD_SLAB = 256
# Every symbol include/lsm_gnn_backward_large.h declares (checked by tests/test_gnn_backward_large_capi.py).
EXPORTED_GNN_BACKWARD_LARGE = ("lsm_gnn_backward_large_workspace_bytes", "lsm_gnn_backward_large",
                               "lsm_host_gnn_backward_large", "lsm_gnn_backward_large_plan",
                               "lsm_gnn_backward_large_last_error")
# Every symbol include/lsm_gnn_embed_backward.h declares (checked by tests/test_gnn_embed_backward_capi.py); its
# slabs are LSM_GNN_BWD_SLAB graphs.
EXPORTED_GNN_EMBED_BACKWARD = ("lsm_gnn_embed_floats", "lsm_gnn_embed_backward_workspace_bytes",
                               "lsm_gnn_embed_backward", "lsm_host_gnn_embed_backward",
                               "lsm_gnn_embed_backward_plan", "lsm_gnn_embed_backward_last_error")
# Every symbol include/lsm_optim.h declares (checked by tests/test_optim_capi.py).
EXPORTED_OPTIM = ("lsm_optim_workspace_bytes", "lsm_optim_step", "lsm_host_optim_step", "lsm_optim_last_error")
LSM_OPT_MAX_GROUPS, LSM_OPT_MAX_SEGMENTS, LSM_OPT_CHUNK, LSM_OPT_LANES = 4, 8, 1024, 256
# Every symbol include/lsm_train_info.h declares (checked by tests/test_train_info_capi.py).
EXPORTED_TRAIN_INFO = ("lsm_train_info_add", "lsm_train_info_mean", "lsm_host_train_info_add",
                       "lsm_host_train_info_mean", "lsm_train_info_last_error")
LSM_TRAIN_INFO_SLOTS, LSM_TRAIN_INFO_MEANS, LSM_TRAIN_INFO_STATE_WORDS, LSM_TRAIN_INFO_LANES = 8, 6, 18, 64
# the slots' names, in the header's order
TRAIN_INFO_SLOTS = ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio",
                    "actor_skipped", "critic_skipped")


class LsmConfig(C.Structure):
    _fields_ = [("dynamics", C.c_int32), ("num_envs", C.c_int32), ("num_agents", C.c_int32),
                ("num_landmarks", C.c_int32), ("episode_length", C.c_int32),
                ("use_safety_filter", C.c_int32), ("use_masking", C.c_int32),
                ("auto_reset", C.c_int32), ("emit_edges", C.c_int32), ("adj_layout", C.c_int32),
                ("world_size", C.c_double), ("seed", C.c_int64), ("env_offset", C.c_int64),
                ("collision_forces", C.c_int32), ("scenario", C.c_int32), ("rng", C.c_int32),
                ("num_internal_step", C.c_int32), ("reward_terms", C.c_int32), ("collaborative", C.c_int32)]


class LsmKernelSelect(C.Structure):
    """lsm_kernel_select: kernel choice for parity tests and A/B runs (the library reads no
    environment variables). ``kernel_select(**overrides)`` fills the defaults."""
    _fields_ = [(n, C.c_int32) for n in ("workgroup_per_env", "lanes_per_env", "team", "generic", "lean",
                                         "filter_search", "bounds_shift")]


KERNEL_SELECT_DEFAULTS = dict(workgroup_per_env=0, lanes_per_env=0, team=-1, generic=0, lean=-1, filter_search=-1,
                              bounds_shift=0)


def kernel_select(**overrides) -> LsmKernelSelect:
    bad = set(overrides) - set(KERNEL_SELECT_DEFAULTS)
    if bad:
        raise ValueError("unknown kernel_select fields: %s" % sorted(bad))
    return LsmKernelSelect(**dict(KERNEL_SELECT_DEFAULTS, **overrides))


class LsmCurriculum(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "curriculum_ratio", "sloped", "stair", "ratio_airtaxi", "ratio_scenario",
        "goal_heading_error_thresh", "goal_speed_error_thresh", "min_dist_thresh",
        "separation_distance", "engagement_distance", "world_use_safety_filter", "stair_is_int")]


class LsmReturnsConfig(C.Structure):
    _fields_ = [("gamma", C.c_double), ("gae_lambda", C.c_double), ("use_gae", C.c_int32),
                ("use_proper_time_limits", C.c_int32)]


class LsmGatherField(C.Structure):
    """lsm_gather_field (include/lsm_learner.h)."""
    _fields_ = [("kind", C.c_int32), ("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64),
                ("masks", C.c_void_p), ("E", C.c_int32), ("N", C.c_int32)]


class LsmChunkField(C.Structure):
    """lsm_chunk_field (include/lsm_recurrent.h)."""
    _fields_ = [("kind", C.c_int32), ("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64),
                ("masks", C.c_void_p), ("E", C.c_int32), ("N", C.c_int32)]


class LsmRowCopy(C.Structure):
    """lsm_row_copy (include/lsm_recurrent.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int64), ("zero_on_done", C.c_int32)]


class LsmMbGraphs(C.Structure):
    """lsm_mb_graphs (include/lsm_minibatch_edges.h), passed by value."""
    _fields_ = [("adj", C.c_void_p), ("masks", C.c_void_p), ("E", C.c_int32), ("N", C.c_int32), ("rows", C.c_int64),
                ("kind", C.c_int32), ("ids", C.c_void_p), ("count", C.c_int64), ("L", C.c_int64), ("T", C.c_int64),
                ("M", C.c_int64)]


class LsmGnnConfig(C.Structure):
    """lsm_gnn_config (include/lsm_gnn.h), passed by value."""
    _fields_ = [(n, C.c_int32) for n in ("F", "num_embeddings", "embedding_size", "embed_hidden", "embed_layer_N",
                                         "embed_relu", "layer_norm", "C", "H", "concat", "layer_N", "relu", "aggr",
                                         "ego_only")]


class LsmGnnLaunchPlan(C.Structure):
    """lsm_gnn_launch_plan (include/lsm_gnn.h): what lsm_gnn_plan fills."""
    _fields_ = [(n, C.c_int32) for n in ("TS", "G", "adj_lds", "fast", "SA", "SK")] + [("lds_bytes", C.c_int64)]


class LsmGnnBwdIo(C.Structure):
    """lsm_gnn_bwd_io (include/lsm_gnn_backward.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("node_obs", "adj", "masks", "agent_id", "dout", "dweights", "dh0",
                                          "workspace", "bad")]


class LsmGnnBwdLaunchPlan(C.Structure):
    """lsm_gnn_bwd_launch_plan (include/lsm_gnn_backward.h): what lsm_gnn_backward_plan fills."""
    _fields_ = ([(n, C.c_int32) for n in ("TS", "G", "fast", "adj_lds", "acc_lds", "SA", "SK", "ST")] +
                [(n, C.c_int64) for n in ("lds_bytes", "slabs", "ws_bytes")])


class LsmGnnBwdLargeLaunchPlan(C.Structure):
    """lsm_gnn_bwd_large_launch_plan (include/lsm_gnn_backward_large.h): what lsm_gnn_backward_large_plan fills."""
    _fields_ = ([(n, C.c_int32) for n in ("TS", "G", "fast", "adj_lds", "acc_lds", "SA", "SK", "ST", "spill",
                                          "spilled_floats")] +
                [(n, C.c_int64) for n in ("lds_bytes", "slabs", "ws_bytes", "scratch_bytes")])


class LsmGnnEmbedBwdIo(C.Structure):
    """lsm_gnn_embed_bwd_io (include/lsm_gnn_embed_backward.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("node_obs", "adj", "masks", "dh0", "dembed", "workspace", "bad")]


class LsmGnnEmbedBwdLaunchPlan(C.Structure):
    """lsm_gnn_embed_bwd_launch_plan (include/lsm_gnn_embed_backward.h): what lsm_gnn_embed_backward_plan fills."""
    _fields_ = ([(n, C.c_int32) for n in ("TS", "G", "fast", "adj_lds", "acc_lds", "S", "per_graph", "entries")] +
                [(n, C.c_int64) for n in ("lds_bytes", "slabs", "ws_bytes")])


class LsmHeadPlanJob(C.Structure):
    """lsm_head_plan_job (include/lsm_policy.h)."""
    _fields_ = [(n, C.c_int32) for n in ("nout", "nin", "ti_n", "tile0")]


class LsmHeadLaunchPlan(C.Structure):
    """lsm_head_launch_plan (include/lsm_policy.h): what lsm_head_plan fills."""
    _fields_ = ([(n, C.c_int32) for n in ("SX", "SA", "SH", "S0", "S1", "S2", "HP", "njobs", "ntiles")] +
                [("lds_bytes", C.c_int64 * 2), ("slabs", C.c_int64), ("ws_floats", C.c_int64), ("o_feat", C.c_int64),
                 ("o_ho", C.c_int64 * 2), ("job", LsmHeadPlanJob * LSM_HEAD_PLAN_MAX_JOBS)])


class LsmHeadConfig(C.Structure):
    """lsm_head_config (include/lsm_policy.h), passed by value."""
    _fields_ = [(n, C.c_int32) for n in ("in0", "in1", "hidden", "layer_N", "relu", "feature_norm", "recurrent_N",
                                         "kind", "num_actions")]


class LsmHeadIo(C.Structure):
    """lsm_head_io (include/lsm_policy.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("x0", "x1", "rnn_states", "masks", "u", "available_actions", "actions_i32",
                                          "actions_f32", "log_probs", "logits", "values", "features", "rnn_out",
                                          "bad")]


class LsmEvalIo(C.Structure):
    """lsm_eval_io (include/lsm_evaluate.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("x0", "x1", "rnn_states", "masks", "actions", "available_actions",
                                          "active_masks", "log_probs", "entropy", "dist_entropy", "logits", "values",
                                          "features", "rnn_out", "scratch", "bad")]


class LsmLossConfig(C.Structure):
    """lsm_loss_config (include/lsm_loss.h), passed by value."""
    _fields_ = ([("vn_beta", C.c_double)] +
                [(n, C.c_float) for n in ("clip_param", "huber_delta", "value_loss_coef", "entropy_coef")] +
                [(n, C.c_int32) for n in ("use_clipped_value_loss", "use_huber_loss", "use_value_active_masks",
                                          "use_policy_active_masks", "use_valuenorm", "num_actions")])


class LsmLossIo(C.Structure):
    """lsm_loss_io (include/lsm_loss.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("logits", "actions", "available_actions", "old_log_probs", "advantages",
                                          "active_masks", "values", "value_preds", "returns", "vn_state", "denorm",
                                          "dlogits", "dvalues", "imp_weights", "stats", "scratch", "bad")]


class LsmBwdIo(C.Structure):
    """lsm_bwd_io (include/lsm_backward.h): one call's tensors, passed by pointer."""
    _fields_ = [(n, C.c_void_p) for n in ("x0", "x1", "rnn_states", "masks", "available_actions", "dlogits",
                                          "dvalues", "dweights", "dx0", "dx1", "workspace")]


class LsmOptimSegment(C.Structure):
    """lsm_optim_segment (include/lsm_optim.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("weights", "grads", "exp_avg", "exp_avg_sq")] + [("n", C.c_int64)]


class LsmOptimGroup(C.Structure):
    """lsm_optim_group (include/lsm_optim.h): one parameter group of a call's table."""
    _fields_ = ([("segments", LsmOptimSegment * LSM_OPT_MAX_SEGMENTS)] +
                [(n, C.c_int32) for n in ("n_segments", "use_max_grad_norm", "skip_nonfinite", "reserved")] +
                [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm")] +
                [("state", C.c_void_p), ("info", C.c_void_p)])


class LsmTrainInfoSrc(C.Structure):
    """lsm_train_info_src (include/lsm_train_info.h), passed by value."""
    _fields_ = [("value", C.c_void_p * LSM_TRAIN_INFO_SLOTS)]


class LsmError(RuntimeError):
    pass


_lib = None


def load_library(path: str = LIB_PATH):
    """Load liblsm_rollout.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise LsmError("liblsm_rollout.so not built (%s); run __graft_entry__.build() or "
                       "python -m lsm.build -- there is no CPU fallback" % path)
    lib = C.CDLL(path)
    P, I32, I64, U32, D, SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_double, C.c_size_t
    sig = {
        "lsm_create": (I32, [C.POINTER(LsmConfig), C.POINTER(P)]),
        "lsm_create_select": (I32, [C.POINTER(LsmConfig), C.POINTER(LsmKernelSelect), C.POINTER(P)]),
        "lsm_destroy": (None, [P]),
        "lsm_last_error": (C.c_char_p, [P]),
        "lsm_set_value_table": (I32, [P, I32, P, P, P, P, P, P, D]),
        "lsm_set_ttr_table": (I32, [P, I32, P, P, P, P, P, D]),
        "lsm_bind_output": (I32, [P, I32, P, SZ]),
        "lsm_output_bytes": (SZ, [P, I32]),
        "lsm_reset": (I32, [P, C.POINTER(LsmCurriculum), P]),
        "lsm_step": (I32, [P, P, I32, C.POINTER(LsmCurriculum), P]),
        "lsm_num_entities": (I32, [P]),
        "lsm_node_features": (I32, [P]),
        "lsm_obs_dim": (I32, [P]),
        "lsm_host_mt_uniforms": (I32, [U32, I32, D, D, P]),
        "lsm_host_scenario": (I32, [C.POINTER(LsmConfig), C.POINTER(LsmCurriculum), U32, P, P]),
        "lsm_set_agent_state": (I32, [P, I32, P, P, P]),
        "lsm_edges_workspace_bytes": (SZ, [I64]),
        "lsm_edges_count": (I32, [P, P, I64, I32, I32, P, P, SZ, P]),
        "lsm_edges_emit": (I32, [P, P, I64, I32, I32, P, I64, P, P, P]),
        "lsm_edges_emit_dev": (I32, [P, P, I64, I32, I32, P, I64, P, P, P]),
        "lsm_edges_scan_emit": (I32, [P, P, I64, I32, I32, P, P, P, SZ, I64, P, P, P, P]),
        "lsm_edges_last_error": (C.c_char_p, []),
        "lsm_bind_output_ring": (I32, [P, I32, P, SZ, I32, I32]),
        "lsm_select_ring": (I32, [P, I32]),
        "lsm_buffer_insert": (I32, [P, P, I32, I32, I32, I32, P, P, P, P, P, P]),
        "lsm_buffer_last_error": (C.c_char_p, []),
        "lsm_host_rk45_di": (I32, [P, D, D, D, P]),
        "lsm_host_glibc_pow": (D, [D, D]),
        "lsm_action_errors": (I32, [P, P]),
        "lsm_kernel_name": (C.c_char_p, [P]),
        "lsm_kernel_name_for": (I32, [C.POINTER(LsmConfig), C.POINTER(LsmKernelSelect), C.c_char_p, SZ]),
        "lsm_reset_layout": (I32, [P, C.POINTER(LsmCurriculum), P, P]),
        "lsm_layout_doubles": (I32, [P]),
        "lsm_host_philox_uniforms": (I32, [U32, U32, I32, D, D, P]),
        "lsm_host_philox4x32": (I32, [P, P, P]),
        "lsm_episode_summary": (I32, [P, I32, P, P]),
        "lsm_build_id": (C.c_char_p, []),
        "lsm_test_set_mt_stage": (I32, [P, I32]),
        "lsm_test_read_value_bounds": (I32, [P, P, I32, P, P]),
        # include/lsm_learner.h
        "lsm_buffer_compute_returns": (I32, [P, P, P, P, P, P, P, I32, I64, C.POINTER(LsmReturnsConfig), P]),
        "lsm_host_compute_returns": (I32, [P, P, P, P, P, P, P, I32, I64, C.POINTER(LsmReturnsConfig)]),
        "lsm_buffer_advantages_workspace_bytes": (SZ, [I64]),
        "lsm_buffer_advantages": (I32, [P, P, P, P, I64, P, P, P, SZ, P]),
        "lsm_returns_last_error": (C.c_char_p, []),
        "lsm_buffer_gather": (I32, [C.POINTER(LsmGatherField), I32, P, I64, I64, P, P]),
        "lsm_gather_last_error": (C.c_char_p, []),
        # include/lsm_recurrent.h
        "lsm_buffer_gather_chunks": (I32, [C.POINTER(LsmChunkField), I32, P, I64, I64, I64, I64, P, P]),
        "lsm_host_gather_chunks": (I32, [C.POINTER(LsmChunkField), I32, P, I64, I64, I64, I64, P]),
        "lsm_buffer_copy_rows": (I32, [C.POINTER(LsmRowCopy), I32, P, I64, P]),
        "lsm_recurrent_last_error": (C.c_char_p, []),
        # include/lsm_minibatch_edges.h
        "lsm_mb_edges_workspace_bytes": (SZ, [I64]),
        "lsm_mb_edges_count": (I32, [LsmMbGraphs, P, P, SZ, P, P]),
        "lsm_mb_edges_emit": (I32, [LsmMbGraphs, P, I64, I64, P, P, P]),
        "lsm_host_mb_edges": (I32, [LsmMbGraphs, I64, P, P, P, P]),
        "lsm_mb_edges_last_error": (C.c_char_p, []),
        # include/lsm_gnn.h
        "lsm_gnn_weights_floats": (SZ, [LsmGnnConfig]),
        "lsm_gnn_forward": (I32, [LsmGnnConfig, P, P, P, P, I64, I32, I32, P, P, P, P]),
        "lsm_host_gnn_forward": (I32, [LsmGnnConfig, P, P, P, P, I64, I32, I32, P, P, P]),
        "lsm_gnn_last_error": (C.c_char_p, []),
        "lsm_gnn_plan": (I32, [LsmGnnConfig, I64, I32, I32, I32, C.POINTER(LsmGnnLaunchPlan)]),
        # include/lsm_policy.h
        "lsm_head_weights_floats": (SZ, [LsmHeadConfig]),
        "lsm_head_forward": (I32, [LsmHeadConfig, P, C.POINTER(LsmHeadIo), I64, P]),
        "lsm_host_head_forward": (I32, [LsmHeadConfig, P, C.POINTER(LsmHeadIo), I64]),
        "lsm_policy_last_error": (C.c_char_p, []),
        "lsm_head_plan": (I32, [LsmHeadConfig, I32, I64, I32, C.POINTER(LsmHeadLaunchPlan)]),
        # include/lsm_evaluate.h
        "lsm_head_evaluate_scratch_bytes": (SZ, [I64, I32]),
        "lsm_head_evaluate": (I32, [LsmHeadConfig, P, C.POINTER(LsmEvalIo), I64, I32, P]),
        "lsm_host_head_evaluate": (I32, [LsmHeadConfig, P, C.POINTER(LsmEvalIo), I64, I32]),
        # include/lsm_loss.h
        "lsm_ppo_loss_scratch_bytes": (SZ, [I64]),
        "lsm_ppo_loss": (I32, [LsmLossConfig, C.POINTER(LsmLossIo), I64, P]),
        "lsm_host_ppo_loss": (I32, [LsmLossConfig, C.POINTER(LsmLossIo), I64]),
        "lsm_loss_last_error": (C.c_char_p, []),
        # include/lsm_backward.h
        "lsm_head_backward_workspace_bytes": (SZ, [LsmHeadConfig, I64, I32]),
        "lsm_head_backward": (I32, [LsmHeadConfig, P, C.POINTER(LsmBwdIo), I64, I32, P]),
        "lsm_host_head_backward": (I32, [LsmHeadConfig, P, C.POINTER(LsmBwdIo), I64, I32]),
        # include/lsm_gnn_backward.h
        "lsm_gnn_backward_workspace_bytes": (SZ, [LsmGnnConfig, I64, I32]),
        "lsm_gnn_backward": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnBwdIo), I64, I32, I32, P]),
        "lsm_host_gnn_backward": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnBwdIo), I64, I32, I32]),
        "lsm_gnn_backward_plan": (I32, [LsmGnnConfig, I64, I32, I32, I32, C.POINTER(LsmGnnBwdLaunchPlan)]),
        "lsm_gnn_backward_last_error": (C.c_char_p, []),
        # include/lsm_gnn_backward_large.h
        "lsm_gnn_backward_large_workspace_bytes": (SZ, [LsmGnnConfig, I64, I32, I32]),
        "lsm_gnn_backward_large": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnBwdIo), I64, I32, I32, I32, P]),
        "lsm_host_gnn_backward_large": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnBwdIo), I64, I32, I32]),
        "lsm_gnn_backward_large_plan": (I32, [LsmGnnConfig, I64, I32, I32, I32, I32,
                                              C.POINTER(LsmGnnBwdLargeLaunchPlan)]),
        "lsm_gnn_backward_large_last_error": (C.c_char_p, []),
        # include/lsm_gnn_embed_backward.h (its slabs are LSM_GNN_BWD_SLAB graphs)
        "lsm_gnn_embed_floats": (SZ, [LsmGnnConfig]),
        "lsm_gnn_embed_backward_workspace_bytes": (SZ, [LsmGnnConfig, I64, I32]),
        "lsm_gnn_embed_backward": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnEmbedBwdIo), I64, I32, I32, P]),
        "lsm_host_gnn_embed_backward": (I32, [LsmGnnConfig, P, C.POINTER(LsmGnnEmbedBwdIo), I64, I32, I32]),
        "lsm_gnn_embed_backward_plan": (I32, [LsmGnnConfig, I64, I32, I32, I32, C.POINTER(LsmGnnEmbedBwdLaunchPlan)]),
        "lsm_gnn_embed_backward_last_error": (C.c_char_p, []),
        # include/lsm_optim.h
        "lsm_optim_workspace_bytes": (SZ, [C.POINTER(LsmOptimGroup), I32]),
        "lsm_optim_step": (I32, [C.POINTER(LsmOptimGroup), I32, P, P]),
        "lsm_host_optim_step": (I32, [C.POINTER(LsmOptimGroup), I32, P]),
        "lsm_optim_last_error": (C.c_char_p, []),
        # include/lsm_train_info.h
        "lsm_train_info_add": (I32, [P, LsmTrainInfoSrc, I32, P]),
        "lsm_train_info_mean": (I32, [P, I64, P, P]),
        "lsm_host_train_info_add": (I32, [P, LsmTrainInfoSrc, I32]),
        "lsm_host_train_info_mean": (I32, [P, I64, P]),
        "lsm_train_info_last_error": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name, None)
        if fn is None and os.environ.get("LSM_LIB_AB") == "1":
            continue   # tools/ab_bench.py --allow-old: an older library may lack a newer entry point
        if fn is None:
            raise AttributeError("%s: missing symbol %s" % (path, name))
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, handle=None):
    if rc != 0:
        lib = load_library()
        msg = lib.lsm_last_error(handle).decode() if handle else "lsm call failed"
        raise LsmError(msg)
