"""ctypes binding of librx.so (include/rx.h).

torch is imported first on purpose: torch ships its own libamdhip64.so.7 and
librx.so links against the same SONAME, so loading librx after torch makes
both share ONE HIP runtime (streams and device pointers are then
interchangeable).  There is no CPU fallback: if the library is missing or the
device is absent, calls fail loudly.
"""
import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede librx: shared HIP runtime, see above)

from . import _build

ABI_VERSION = 25
RX_EP_SHARDS = 64  # rx_io.ep_stats rows (include/rx.h)
RX_OK, RX_EINVAL, RX_EHIP, RX_ENOMEM, RX_ESTATE = 0, -1, -2, -3, -4
RX_F_CRASHED, RX_F_FINISHED, RX_F_CP25, RX_F_CP50, RX_F_CP75, RX_F_HAS_CRASHED = 1, 2, 4, 8, 16, 32
RX_EF_PENDING_RESET = 1
RX_AUTORESET_NEXT_STEP, RX_AUTORESET_SAME_STEP, RX_AUTORESET_DISABLED = 0, 1, 2
RX_INFO_W = 4
RX_INFO_SPEED, RX_INFO_PROGRESS, RX_INFO_PROGRESS_DELTA, RX_INFO_PLACEMENT = 0, 1, 2, 3

_P = ctypes.c_void_p

EXPORTS = ("rx_last_error", "rx_abi_version", "rx_create", "rx_destroy", "rx_sensor_angles", "rx_upload_tracks",
           "rx_assign", "rx_bind_state", "rx_set_speed_weight", "rx_reset", "rx_step", "rx_step_phases", "rx_gae",
           "rx_gae_scan", "rx_adam_workspace_floats", "rx_adam_clip_step", "rx_ppo_n_params", "rx_ppo_workspace_floats",
           "rx_ppo_workspace_doubles", "rx_ppo_adv_stats", "rx_ppo_minibatch_grad", "rx_policy_act",
           "rx_rollout_supported", "rx_rollout", "rx_ppo_adv_moments", "rx_ppo_adv_finalize", "rx_ppo_minibatch_grad_shard", "rx_ppo_kl_check", "rx_random_permutation",
           "rx_profile", "rx_profile_read", "rx_ppo_update_workspace_floats", "rx_ppo_minibatch_update", "rx_env_order",
           "rx_state_import", "rx_state_export", "rx_schedule",
           "rx_ppo_adv_workspace_doubles", "rx_ppo_adv_stats_ws", "rx_profile_waves", "rx_ray_waves", "rx_ray_tasks", "rx_set_start_draws",
           "rx_rollout_steps", "rx_selfplay_rollout_steps", "rx_steps", "rx_build_tracks", "rx_build_tracks_host",
           "rx_eval_steps", "rx_raster_static", "rx_raster_static_host", "rx_raster_trail", "rx_raster_trail_host",
           "rx_raster_frame", "rx_raster_frame_host", "rx_policy_act_bank", "rx_match_steps",
           "rx_league_weights", "rx_league_weights_host", "rx_league_draw", "rx_league_draw_host",
           "rx_league_rollout_steps", "rx_cull_table_sizes", "rx_build_cull_tables", "rx_build_cull_tables_host",
           "rx_upload_tracks_device", "rx_track_tally", "rx_track_tally_host", "rx_track_scores", "rx_track_scores_host",
           "rx_track_draw", "rx_track_draw_host", "rx_track_rollout_steps", "rx_track_learn_tally",
           "rx_track_learn_tally_host", "rx_track_learn_fold", "rx_track_learn_fold_host", "rx_track_learn_tables",
           "rx_track_learn_tables_host", "rx_track_learn_draw", "rx_track_learn_draw_host", "rx_track_evolve_plan",
           "rx_track_evolve_plan_host", "rx_track_evolve", "rx_track_evolve_host", "rx_track_evolve_classes",
           "rx_track_evolve_classes_host", "rx_track_evolve_inplace", "rx_track_evolve_inplace_host",
           "rx_track_evolve_commit", "rx_track_evolve_commit_host", "rx_track_episode",
           "rx_track_episode_host", "rx_track_episode_step", "rx_track_episodic_rollout_steps",
           "rx_track_learn_tally_slots", "rx_track_learn_tally_slots_host", "rx_track_learn_episode",
           "rx_track_learn_episode_host", "rx_track_learn_episode_step", "rx_track_learn_episodic_rollout_steps",
           "rx_track_tally2", "rx_track_tally2_host", "rx_track_duel_scores", "rx_track_duel_scores_host",
           "rx_track_duel_rollout_steps",
           "rx_steps_plan", "rx_patch_tracks", "rx_patch_tracks_host", "rx_replace_tracks_device", "rx_assign_plan",
           "rx_regroup_plan_host", "rx_regroup_scratch_bytes", "rx_regroup_plan", "rx_regroup_slots", "rx_lane_layout",
           "rx_set_lane_cars", "rx_assign_plan_cars")
RX_KERNEL_NAMES = ("k_dyn", "k_rays", "k_kin1", "k_step2", "k_step2_reward")
ADAM_MAX_TENSORS = 32
RX_PHASE_DYNAMICS, RX_PHASE_RAYS = 1, 2
RX_PREC_FP32, RX_PREC_BF16 = 0, 1
PRECISION = {"fp32": RX_PREC_FP32, "bf16": RX_PREC_BF16}


class RxConfig(ctypes.Structure):
    _fields_ = [("n_envs", ctypes.c_int32), ("n_agents", ctypes.c_int32), ("n_sensors", ctypes.c_int32),
                ("max_steps", ctypes.c_int32), ("autoreset", ctypes.c_int32), ("device", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("sensor_half_cone", ctypes.c_double), ("speed_weight", ctypes.c_double),
                ("cull_chunk", ctypes.c_int32), ("sort_interval", ctypes.c_int32),
                ("ray_order", ctypes.c_int32), ("cull_super", ctypes.c_int32)] + \
               [(k, ctypes.c_int32) for k in ("split", "wide_n", "dyn_lpe", "ray_lpr", "reward_lpe", "argmin_window",
                                               "seg_filter", "box_quadrants", "ray_dispatch", "ray_tail",
                                               "ray_tail_lpr", "task_sort", "lane_tracks", "reserved0")]


# rx_config launch-schedule fields (ABI v17, v19, v20, v23): 0 = auto, -1 = off / none (include/rx.h).
# Scheduling only: every value gives bit-identical results.
SCHEDULE_W = 18  # rx_schedule: resolved schedule (include/rx.h)
SCHEDULE_KEYS = ("split", "wide", "dyn_lpe", "ray_lpr", "reward_lpe", "argmin_window", "seg_filter", "box_quadrants",
                 "dyn_waves", "ray_waves", "ray_dispatch", "ray_tail", "ray_tail_lpr", "ray_tail_from", "task_sort",
                 "lane_tracks", "dyn_calls", "reserved")
SCHED_FIELDS = ("split", "wide_n", "dyn_lpe", "ray_lpr", "reward_lpe", "argmin_window", "seg_filter", "box_quadrants",
                "ray_dispatch", "ray_tail", "ray_tail_lpr", "task_sort", "lane_tracks")


STATE_FIELDS = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering", "finished_step", "flags",
                "steps", "track", "env_flags", "ep_return", "ep_length", "speed_weight")


class RxState(ctypes.Structure):
    _fields_ = [(k, _P) for k in STATE_FIELDS]


IO_FIELDS = ("actions", "obs", "reward", "reward64", "terminated", "truncated", "done_f32", "info", "ep_done",
             "ep_stats", "counters")


class RxIO(ctypes.Structure):
    _fields_ = [(k, _P) for k in IO_FIELDS]


# rx_steps (ABI v21): per-step element strides of the io rows
STRIDE_FIELDS = ("actions", "obs", "reward", "reward64", "terminated", "truncated", "done_f32", "info", "ep_done")


class RxIOStrides(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in STRIDE_FIELDS]


# rx_steps_plan (additive to ABI v25): the launch schedule of an rx_steps call, host only
RX_PLAN_MAX_DEPTH, RX_PLAN_CROSS_RING = 8, 3
PLAN_ARG_FIELDS = ("n_steps", "depth", "sort_interval", "dyn_calls", "task_sort", "task_calls", "tasks_stale", "cross",
                   "rank_in_kin", "ranked", "tasks_stale_out")
_PLAN_ROW = ctypes.c_int32 * RX_PLAN_MAX_DEPTH


class RxPlanArgs(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in PLAN_ARG_FIELDS]


class RxPlanLaunch(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("n_sub", "n_rank", "n_rays", "first_step")] + \
               [(k, _PLAN_ROW) for k in ("kin", "kin_pose", "kin_row")] + \
               [(k, ctypes.c_int32) for k in ("keys", "keys_snap")] + \
               [(k, _PLAN_ROW) for k in ("rank_step", "rank_pose", "rank_row", "ray_step", "ray_pose", "ray_row",
                                         "ray_snap", "ray_shadow")] + \
               [(k, ctypes.c_int32) for k in ("sort_after", "kin1_after", "kin1_pose", "kin1_row")]


def steps_plan(n_steps, depth, sort_interval=0, dyn_calls=0, task_sort=1, task_calls=0, tasks_stale=True, cross=True,
               rank_in_kin=False):
    """rx_steps_plan: (launch records as dicts of ints / lists, ranked steps, tasks_stale after the call)."""
    L = load()
    a = RxPlanArgs(n_steps, depth, sort_interval, dyn_calls, task_sort, task_calls, int(tasks_stale), int(cross),
                   int(rank_in_kin), 0, 0)
    n = L.rx_steps_plan(ctypes.byref(a), None, 0)
    if n < 0:
        raise RxError(f"rx_steps_plan: bad arguments ({n})")
    out = (RxPlanLaunch * n)()
    assert L.rx_steps_plan(ctypes.byref(a), out, n) == n
    recs = [{k: (list(v) if isinstance(v := getattr(r, k), _PLAN_ROW) else v) for k, _ in RxPlanLaunch._fields_}
            for r in out]
    return recs, a.ranked, bool(a.tasks_stale_out)


def steps_plan_default(n_steps):
    """(depth, rank_in_kin) that rx_steps takes for a call of n_steps steps."""
    a = RxPlanArgs(n_steps, 0, 0, 0, 0, 0, 1, 1, -1, 0, 0)
    if load().rx_steps_plan(ctypes.byref(a), None, 0) < 0:
        raise RxError("rx_steps_plan: bad arguments")
    return a.depth, bool(a.rank_in_kin)


# rx_assign_plan (additive to ABI v25): the assignment rx_assign would build, host only
ASSIGN_PLAN_PTRS = ("schedule", "perm", "dyn_waves", "ray_waves", "slot_n", "pos_slot", "env_pos", "sort_base")


class RxAssignPlanIO(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("dyn_cap", "ray_cap", "n_dyn_waves", "n_ray_waves", "sort_bins",
                                              "sort_shift")] + [(k, _P) for k in ASSIGN_PLAN_PTRS]


def assign_plan(cfg, wp_off, track_of_env, lane_cars=None):
    """rx_assign_plan for an RxConfig, wp_off int32 [n_tracks + 1] and track_of_env int32 [n_envs]: a dict of
    schedule (by SCHEDULE_KEYS), perm, sort_bins, sort_shift, dyn_waves / ray_waves int32 [n][4], slot_n, and
    pos_slot / env_pos (lane-varying schedules, else None) and sort_base (with sort_bins > 0, else None).
    lane_cars (-1, 0, 1): rx_assign_plan_cars, the plan of a two-car handle with that rx_set_lane_cars mode.
    A refusal raises RxError with the library's text."""
    L = load()
    wp_off = np.ascontiguousarray(wp_off, np.int32)
    toe = np.ascontiguousarray(track_of_env, np.int32)
    n_tracks, N = len(wp_off) - 1, cfg.n_envs
    io = RxAssignPlanIO()

    def plan():
        args = (n_tracks, ptr(wp_off), ptr(toe), ctypes.byref(io))
        if lane_cars is None:
            check(L.rx_assign_plan(ctypes.byref(cfg), *args), "rx_assign_plan")
        else:
            check(L.rx_assign_plan_cars(ctypes.byref(cfg), int(lane_cars), *args), "rx_assign_plan_cars")
    plan()
    out = dict(schedule=np.zeros(SCHEDULE_W, np.int32), perm=np.zeros(N, np.int32),
               dyn_waves=np.zeros((io.n_dyn_waves, 4), np.int32), ray_waves=np.zeros((io.n_ray_waves, 4), np.int32),
               slot_n=np.zeros(n_tracks, np.int32), pos_slot=np.zeros(N, np.int32), env_pos=np.zeros(N, np.int32),
               sort_base=np.zeros(n_tracks, np.int32))
    io.dyn_cap, io.ray_cap = io.n_dyn_waves, io.n_ray_waves
    for k in ASSIGN_PLAN_PTRS:
        setattr(io, k, out[k].ctypes.data)
    plan()
    out["schedule"] = {k: int(v) for k, v in zip(SCHEDULE_KEYS, out["schedule"])}
    out["sort_bins"], out["sort_shift"] = io.sort_bins, io.sort_shift
    if not out["schedule"]["lane_tracks"]:
        out["pos_slot"] = out["env_pos"] = None
    if io.sort_bins == 0:
        out["sort_base"] = None
    return out


class RxAdamConfig(ctypes.Structure):
    _fields_ = [("n_tensors", ctypes.c_int32), ("offsets", ctypes.c_int64 * 33), ("beta1", ctypes.c_double),
                ("beta2", ctypes.c_double), ("eps", ctypes.c_double), ("max_grad_norm", ctypes.c_double)]


class RxPPOBatch(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("mb", ctypes.c_int32), ("n_rows", ctypes.c_int64)] + \
               [(k, _P) for k in ("obs", "actions", "logprobs", "advantages", "returns", "values", "perm", "params",
                                  "log_std", "adv_stats")] + \
               [("clip_coef", ctypes.c_float), ("vf_coef", ctypes.c_float), ("kl_target", ctypes.c_float),
                ("precision", ctypes.c_int32)]


class RxRolloutIO(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("obs_dim", ctypes.c_int32)] + \
               [(k, _P) for k in ("params", "log_std", "eps", "obs", "actions", "logprobs", "values", "rewards",
                                  "dones", "next_obs", "next_done")]


class RxPolicyIO(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("n", ctypes.c_int64)] + \
               [(k, _P) for k in ("obs", "eps", "params", "log_std", "actions", "logprobs", "values")] + \
               [("obs_stride", ctypes.c_int64), ("act_stride", ctypes.c_int64), ("precision", ctypes.c_int32),
                ("actions2", _P), ("act2_stride", ctypes.c_int64)]


class RxSelfplayIO(ctypes.Structure):
    _fields_ = [(k, _P) for k in ("opp_params", "opp_log_std", "opp_eps", "env_actions", "env_obs", "env_reward",
                                  "sink")] + [("agent", ctypes.c_int32), ("opp_precision", ctypes.c_int32)]


RX_EVAL_W = 10  # doubles per (env, car) of rx_eval_io.acc (include/rx.h)


class RxEvalIO(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("precision", ctypes.c_int32)] + \
               [(k, _P) for k in ("params", "log_std", "eps", "actions", "logp_sink", "value_sink", "acc", "active",
                                  "n_active")]


# league play (ABI v25, additive): the policy-bank forward and the match loop (include/rx.h)
class RxPolicyBankIO(ctypes.Structure):
    _fields_ = [("io", RxPolicyIO), ("n_policies", ctypes.c_int32), ("tile_cars", ctypes.c_int32),
                ("params_stride", ctypes.c_int64), ("policy_of_row", _P)]


class RxMatchIO(ctypes.Structure):
    _fields_ = [("obs_dim", ctypes.c_int32), ("precision", ctypes.c_int32)] + \
               [(k, _P) for k in ("params", "log_std", "eps", "actions", "logp_sink", "value_sink", "acc", "active",
                                  "n_active")] + \
               [("n_policies", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("params_stride", ctypes.c_int64),
                ("seat", _P)]


# league training (ABI v25, additive): per-env opponents drawn and tallied on the device (include/rx.h)
RX_LEAGUE_MAX_SLOTS, RX_LEAGUE_MAX_POWER, RX_LEAGUE_TALLY_W = 64, 4, 3


class RxLeagueIO(ctypes.Structure):
    _fields_ = [("n_slots", ctypes.c_int32), ("agent", ctypes.c_int32), ("params", _P), ("log_std", _P),
                ("params_stride", ctypes.c_int64), ("opp_id", _P), ("draw_count", _P), ("tally", _P), ("cdf", _P),
                ("seed", ctypes.c_uint64), ("opp_precision", ctypes.c_int32)]


# track curriculum (ABI v25, additive): per-slot tallies and prioritised env -> slot draws (include/rx.h)
RX_TRACK_TALLY_W, RX_TRACK_MAX_POWER, RX_TRACK_SCORES_CHUNK = 4, 4, 1024
TRACK_SCORES = {"fail": 0, "potential": 1}


class RxTrackIO(ctypes.Structure):
    _fields_ = [("n_tracks", ctypes.c_int32), ("score", ctypes.c_int32), ("track", _P), ("tally", _P), ("cdf", _P),
                ("p", _P), ("track_of_env", _P), ("seed", ctypes.c_uint64)]


# the track curriculum for self-play (ABI v25, additive): two-car tallies and the win scores (include/rx.h)
RX_TRACK_DUEL_W = 4
TRACK_DUEL_SCORES = {"fail": 0, "potential": 1, "lose": 2, "contested": 3}


class RxTrackDuelIO(ctypes.Structure):
    _fields_ = [("agent", ctypes.c_int32), ("duel", _P)]


# episodic track draws (ABI v25, additive): an env takes a new slot when its episode ends (include/rx.h)
RX_TRACK_EPISODE_SALT = 0x9C3B5E2D7F1A8046  # csrc/rx_curriculum.h


class RxTrackEpisodeIO(ctypes.Structure):
    _fields_ = [("draws", _P), ("env_pos", _P), ("pos_slot", _P), ("slot_out", _P), ("mix", ctypes.c_double)]


# the curriculum's replay scores (ABI v25, additive): value-loss scores, rank and staleness draws (include/rx.h)
RX_TRACK_LEARN_W, RX_TRACK_LEARN_MAX_POWER, RX_TRACK_LEARN_CHUNK, RX_TRACK_RANK_TILE = 2, 10, 1024, 1024
TRACK_LEARN_KINDS = {"value_l1": 0, "value_pos": 1}
TRACK_LEARN_FIELDS = ("track", "learn", "score", "seen", "rank", "cdf_score", "cdf_stale", "track_of_env")


class RxTrackLearnIO(ctypes.Structure):
    _fields_ = [("n_tracks", ctypes.c_int32), ("kind", ctypes.c_int32)] + [(k, _P) for k in TRACK_LEARN_FIELDS] + \
               [("seed", ctypes.c_uint64)]


# track evolution (ABI v25, additive): fresh tracks and edited children written on the device (include/rx.h)
RX_TRACK_EVOLVE_W, RX_TRACK_EVOLVE_FRESH, RX_TRACK_EVOLVE_EDIT = 4, 0, 1
TRACK_EVOLVE_FIELDS = ("slots", "cp_off", "cp", "width", "cdf_score", "plan", "cp_off_new", "cp_new", "width_new")


class RxTrackEvolveIO(ctypes.Structure):
    _fields_ = [("n_tracks", ctypes.c_int32), ("n_spawn", ctypes.c_int32)] + [(k, _P) for k in TRACK_EVOLVE_FIELDS] + \
               [("seed", ctypes.c_uint64)]


# track evolution in place (ABI v25, additive): the rank table by point count, a staging buffer, a commit
RX_TRACK_MAX_P = 64
TRACK_EVOLVE_INPLACE_FIELDS = ("slots", "cp_off", "cp", "width", "cdf_score", "order", "cdf_class", "class_end", "plan",
                               "out_off", "cp_out", "width_out")


class RxTrackEvolveInplaceIO(ctypes.Structure):
    _fields_ = [("n_tracks", ctypes.c_int32), ("n_spawn", ctypes.c_int32)] + \
               [(k, _P) for k in TRACK_EVOLVE_INPLACE_FIELDS] + [("seed", ctypes.c_uint64)]


# rendering (ABI v25, additive): pixel classes / trail bits, size limits, edge record width (include/rx.h)
RX_PX_BACKGROUND, RX_PX_TRACK, RX_PX_BORDER, RX_PX_START, RX_PX_TRAIL0, RX_PX_TRAIL1 = 0, 1, 2, 3, 0x10, 0x20
RX_RASTER_SIZE_MIN, RX_RASTER_SIZE_MAX, RX_RASTER_EDGE_W = 16, 2048, 6
RASTER_PTR_FIELDS = ("env_ids", "x", "y", "angle", "view", "layer_of", "layer", "trail", "last", "out", "out_off")


class RxRasterIO(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("K", "A", "size", "n_envs", "n_layers", "reserved0")] + \
               [(k, _P) for k in RASTER_PTR_FIELDS] + [("out_pitch", ctypes.c_int64), ("out_size", ctypes.c_int64)]


# culling tables of a device-resident track table (ABI v25, additive; include/rx.h)
RX_WP_CHUNK, RX_WP_SUPER, RX_SLOT_HDR_BYTES = 8, 4, 128
CULL_FIELDS = ("chunk_off", "super_off", "wchunk_off", "wsuper_off", "chunk_box", "super_box", "wchunk_box",
               "wsuper_box", "slot_geo", "chunk_box_f", "super_box_f", "seg_f", "slot_hdr")


class RxCullTables(ctypes.Structure):
    _fields_ = [(k, _P) for k in CULL_FIELDS]


# slots replaced in place (ABI v25, additive; include/rx.h): the small source table and the slots it goes to
PATCH_FIELDS = ("slots", "src_off", "wp", "nrm", "seg", "meta")


class RxTrackPatch(ctypes.Structure):
    _fields_ = [("n_upd", ctypes.c_int32)] + [(k, _P) for k in PATCH_FIELDS]


class RxError(RuntimeError):
    pass


_lib = None


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load librx.so (building it with hipcc if it is missing and allowed)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RX_LIB_PATH") or _build.LIB  # override: profiling builds (tools/dyn_stamps.py)
    if not os.path.exists(path):
        if not build_if_missing:
            raise RxError(f"librx.so not built at {path} (run python -m rx._build)")
        _build.build()
    L = ctypes.CDLL(path)
    L.rx_last_error.restype = ctypes.c_char_p
    L.rx_abi_version.restype = ctypes.c_int
    L.rx_create.argtypes = [ctypes.POINTER(RxConfig), ctypes.POINTER(_P)]
    L.rx_destroy.argtypes = [_P]
    L.rx_sensor_angles.argtypes = [_P, _P]
    L.rx_upload_tracks.argtypes = [_P, ctypes.c_int32, _P, _P, _P, _P, _P]
    L.rx_assign.argtypes = [_P, _P]
    L.rx_bind_state.argtypes = [_P, ctypes.POINTER(RxState)]
    L.rx_set_speed_weight.argtypes = [_P, ctypes.c_double]
    L.rx_reset.argtypes = [_P, _P, ctypes.POINTER(RxIO), _P]
    L.rx_step.argtypes = [_P, ctypes.POINTER(RxIO), _P]
    L.rx_step_phases.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.c_int32, _P]
    L.rx_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.c_int32, ctypes.POINTER(RxIOStrides), _P]
    L.rx_steps_plan.argtypes = [ctypes.POINTER(RxPlanArgs), ctypes.POINTER(RxPlanLaunch), ctypes.c_int32]
    L.rx_steps_plan.restype = ctypes.c_int32
    L.rx_assign_plan.argtypes = [ctypes.POINTER(RxConfig), ctypes.c_int32, _P, _P, ctypes.POINTER(RxAssignPlanIO)]
    gae_args = [ctypes.c_int32, ctypes.c_int32, _P, _P, _P, _P, _P, ctypes.c_double, ctypes.c_double, _P, _P, _P]
    L.rx_gae.argtypes = gae_args
    L.rx_gae_scan.argtypes = gae_args
    L.rx_adam_workspace_floats.argtypes = [ctypes.POINTER(RxAdamConfig)]
    L.rx_adam_workspace_floats.restype = ctypes.c_size_t
    L.rx_adam_clip_step.argtypes = [ctypes.POINTER(RxAdamConfig), _P, _P, _P, _P, _P, _P, _P, _P, _P]
    L.rx_ppo_n_params.argtypes = [ctypes.c_int32]
    L.rx_ppo_workspace_floats.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.rx_ppo_workspace_floats.restype = ctypes.c_size_t
    L.rx_ppo_workspace_doubles.argtypes = [ctypes.c_int32]
    L.rx_ppo_workspace_doubles.restype = ctypes.c_size_t
    L.rx_ppo_adv_stats.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, _P, _P]
    L.rx_ppo_minibatch_grad.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, _P, _P, _P, _P, _P, _P]
    L.rx_policy_act.argtypes = [ctypes.POINTER(RxPolicyIO), _P]
    L.rx_rollout_supported.argtypes = [_P]
    L.rx_rollout.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO), _P]
    L.rx_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO), ctypes.c_int32, _P]
    L.rx_selfplay_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                            ctypes.POINTER(RxSelfplayIO), ctypes.c_int32, _P]
    L.rx_ppo_adv_moments.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, _P, _P]
    L.rx_ppo_adv_finalize.argtypes = [_P, ctypes.c_int32, ctypes.c_int64, _P, _P]
    L.rx_ppo_minibatch_grad_shard.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, ctypes.c_float, _P, _P, _P,
                                              _P, _P, _P]
    L.rx_ppo_kl_check.argtypes = [_P, ctypes.c_float, _P, _P, _P]
    L.rx_random_permutation.argtypes = [ctypes.c_int64, ctypes.c_uint64, _P, _P]
    L.rx_ppo_update_workspace_floats.argtypes = [ctypes.c_int32, ctypes.POINTER(RxAdamConfig)]
    L.rx_ppo_update_workspace_floats.restype = ctypes.c_size_t
    L.rx_ppo_minibatch_update.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, ctypes.POINTER(RxAdamConfig)] + \
        [_P] * 12
    L.rx_env_order.argtypes = [_P, _P, _P, _P]
    L.rx_state_import.argtypes = [_P, _P]
    L.rx_state_export.argtypes = [_P, _P]
    L.rx_schedule.argtypes = [_P, _P]
    L.rx_ppo_adv_workspace_doubles.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.rx_ppo_adv_workspace_doubles.restype = ctypes.c_size_t
    L.rx_ppo_adv_stats_ws.argtypes = [ctypes.POINTER(RxPPOBatch), ctypes.c_int32, _P, _P, _P, _P]
    L.rx_profile.argtypes = [_P, ctypes.c_int32]
    L.rx_profile_read.argtypes = [_P, _P, _P]
    L.rx_profile_waves.argtypes = [_P, ctypes.c_int32, _P, _P, ctypes.c_int32, _P, _P, _P]
    L.rx_ray_waves.argtypes = [_P, _P, ctypes.c_int32, _P]
    L.rx_ray_tasks.argtypes = [_P, _P, ctypes.c_int64, _P, _P]
    L.rx_set_start_draws.argtypes = [_P, _P, ctypes.c_int64, _P]
    L.rx_build_tracks.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_P] * 9
    L.rx_build_tracks_host.argtypes = L.rx_build_tracks.argtypes
    L.rx_cull_table_sizes.argtypes = [ctypes.c_int32, _P, ctypes.c_int32, ctypes.c_int32, _P]
    L.rx_build_cull_tables.argtypes = [ctypes.c_int32, _P, _P, _P, _P, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(RxCullTables), _P]
    L.rx_build_cull_tables_host.argtypes = L.rx_build_cull_tables.argtypes
    L.rx_upload_tracks_device.argtypes = [_P, ctypes.c_int32, _P, _P, _P, _P, _P, _P]
    L.rx_patch_tracks.argtypes = [ctypes.c_int32, _P, _P, _P, _P, _P, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.POINTER(RxCullTables), ctypes.POINTER(RxTrackPatch), _P]
    L.rx_patch_tracks_host.argtypes = L.rx_patch_tracks.argtypes
    L.rx_replace_tracks_device.argtypes = [_P, ctypes.POINTER(RxTrackPatch), _P]
    L.rx_regroup_plan_host.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_P] * 6
    L.rx_regroup_scratch_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32]
    L.rx_regroup_scratch_bytes.restype = ctypes.c_int64
    L.rx_regroup_plan.argtypes = [ctypes.c_int32, ctypes.c_int32] + [_P] * 7 + [ctypes.c_int64, _P]
    L.rx_regroup_slots.argtypes = [_P, _P]
    L.rx_lane_layout.argtypes = [_P, _P, _P, _P]
    L.rx_set_lane_cars.argtypes = [_P, ctypes.c_int32]
    L.rx_assign_plan_cars.argtypes = [ctypes.POINTER(RxConfig), ctypes.c_int32, ctypes.c_int32, _P, _P,
                                      ctypes.POINTER(RxAssignPlanIO)]
    L.rx_eval_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxEvalIO), ctypes.c_int32, _P]
    L.rx_policy_act_bank.argtypes = [ctypes.POINTER(RxPolicyBankIO), _P]
    L.rx_match_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxMatchIO), ctypes.c_int32, _P]
    L.rx_league_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                          ctypes.POINTER(RxSelfplayIO), ctypes.POINTER(RxLeagueIO), ctypes.c_int32, _P]
    L.rx_track_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                         ctypes.POINTER(RxTrackIO), ctypes.c_int32, _P]
    L.rx_track_episode_step.argtypes = [_P, ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackEpisodeIO),
                                        ctypes.POINTER(RxIO), _P, _P]
    L.rx_track_episodic_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                                  ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackEpisodeIO), _P,
                                                  ctypes.c_int32, _P]
    L.rx_track_learn_episode_step.argtypes = [_P, ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackLearnIO),
                                              ctypes.POINTER(RxTrackEpisodeIO), ctypes.c_double, ctypes.POINTER(RxIO),
                                              _P, _P]
    L.rx_track_learn_episodic_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                                        ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackLearnIO),
                                                        ctypes.POINTER(RxTrackEpisodeIO), ctypes.c_double, _P,
                                                        ctypes.c_int32, _P]
    L.rx_track_duel_rollout_steps.argtypes = [_P, ctypes.POINTER(RxIO), ctypes.POINTER(RxRolloutIO),
                                              ctypes.POINTER(RxSelfplayIO), ctypes.POINTER(RxLeagueIO),
                                              ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackDuelIO), ctypes.c_int32,
                                              _P]
    for sfx in ("", "_host"):
        td = ctypes.POINTER(RxTrackDuelIO)
        getattr(L, "rx_track_tally2" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), td, ctypes.c_int64, _P, _P, _P, _P]
        getattr(L, "rx_track_duel_scores" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), td, ctypes.c_int32,
                                                             ctypes.c_double, _P]
        getattr(L, "rx_track_episode" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), ctypes.POINTER(RxTrackEpisodeIO),
                                                         ctypes.c_int64, _P, _P, _P, _P]
        getattr(L, "rx_track_tally" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), ctypes.c_int64, _P, _P, _P, _P]
        getattr(L, "rx_track_scores" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), ctypes.c_int32, ctypes.c_double, _P]
        getattr(L, "rx_track_draw" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), ctypes.c_int64, ctypes.c_uint32,
                                                      ctypes.c_double, _P]
        lt = ctypes.POINTER(RxTrackLearnIO)
        getattr(L, "rx_track_learn_tally" + sfx).argtypes = [lt, ctypes.c_int32, ctypes.c_int64, _P, _P]
        getattr(L, "rx_track_learn_tally_slots" + sfx).argtypes = [lt, ctypes.c_int32, ctypes.c_int64, _P, _P, _P, _P]
        getattr(L, "rx_track_learn_episode" + sfx).argtypes = [ctypes.POINTER(RxTrackIO), lt,
                                                               ctypes.POINTER(RxTrackEpisodeIO), ctypes.c_double,
                                                               ctypes.c_int64, _P, _P, _P, _P]
        getattr(L, "rx_track_learn_fold" + sfx).argtypes = [lt, ctypes.c_int32, ctypes.c_double, _P]
        getattr(L, "rx_track_learn_tables" + sfx).argtypes = [lt, ctypes.c_int32, ctypes.c_int32, _P]
        getattr(L, "rx_track_learn_draw" + sfx).argtypes = [lt, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double,
                                                            ctypes.c_double, _P]
        ev = ctypes.POINTER(RxTrackEvolveIO)
        getattr(L, "rx_track_evolve_plan" + sfx).argtypes = [ev, ctypes.c_uint32, ctypes.c_double, _P]
        getattr(L, "rx_track_evolve" + sfx).argtypes = [ev, ctypes.c_uint32, _P]
        evi = ctypes.POINTER(RxTrackEvolveInplaceIO)
        getattr(L, "rx_track_evolve_classes" + sfx).argtypes = [evi, _P]
        getattr(L, "rx_track_evolve_inplace" + sfx).argtypes = [evi, ctypes.c_uint32, ctypes.c_double, _P]
        getattr(L, "rx_track_evolve_commit" + sfx).argtypes = [evi, _P]
        getattr(L, "rx_league_weights" + sfx).argtypes = [ctypes.POINTER(RxLeagueIO), ctypes.c_int32, ctypes.c_int32,
                                                         ctypes.c_double, ctypes.c_double, _P]
        getattr(L, "rx_league_draw" + sfx).argtypes = [ctypes.POINTER(RxLeagueIO), ctypes.c_int64, _P, _P, _P]
        getattr(L, "rx_raster_static" + sfx).argtypes = [ctypes.c_int32] * 3 + [_P] * 4
        getattr(L, "rx_raster_trail" + sfx).argtypes = [ctypes.POINTER(RxRasterIO), _P]
        getattr(L, "rx_raster_frame" + sfx).argtypes = [ctypes.POINTER(RxRasterIO), _P]
    for name in EXPORTS:
        if name not in ("rx_last_error", "rx_abi_version", "rx_ppo_workspace_floats", "rx_ppo_workspace_doubles",
                        "rx_ppo_update_workspace_floats", "rx_adam_workspace_floats",
                        "rx_ppo_adv_workspace_doubles", "rx_regroup_scratch_bytes"):
            getattr(L, name).restype = ctypes.c_int
    if L.rx_abi_version() != ABI_VERSION:
        raise RxError(f"librx ABI {L.rx_abi_version()} != {ABI_VERSION} (rebuild: python -m rx._build)")
    _lib = L
    return L


def check(rc, what=""):
    if rc != RX_OK:
        msg = _lib.rx_last_error().decode() if _lib is not None else "?"
        raise RxError(f"{what} failed (rc={rc}): {msg}")


def ptr(t):
    """Raw device (or host) pointer of a tensor / ndarray, None for None."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous(), "tensors handed to librx must be contiguous"
        return _P(t.data_ptr())
    return _P(t.ctypes.data)


def view_ptr(t):
    """Pointer of a strided view whose row stride the caller passes explicitly."""
    return _P(t.data_ptr())


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return _P(s.cuda_stream)
