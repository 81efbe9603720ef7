"""rx_assign_plan: the assignment rx_assign uploads -- the resolved launch schedule, the env
order and the dynamics- and ray-wave tables -- as a pure function (include/rx.h, DESIGN.md §3
"Plan, then upload"), checked by brute force without a GPU.

The grid: A in {1, 2}; R in {1, 3, 11, 16}, and 17 at ray_order 0 and 1; every ray_order; five
mixes of envs per slot drawn from 0, 1, 63, 64, 65 and 130 (a single slot, one env per slot,
ragged, empty slots in the middle), the envs interleaved so that grouping has work to do; and
per shape two blocks of forced schedules -- dyn_lpe 1/2/4/64 x ray_lpr 1/2/4 x lane_tracks
-1/0/1, and ray_dispatch -1/1/2/3 x ray_tail -1/1/3/16 x ray_tail_lpr 2/4 -- with reward_lpe
1/2/4, task_sort 0/1/3, sort_interval 0/8, split -1/1 and argmin_window 0/-1/32/4 cycled
through them: 8,260 plans.  Every ray-wave record is decoded as rays_wave (rx_kernels.hip)
decodes it and the plan is held to the rules the kernels rely on:

* perm is a permutation, grouped by slot, stable in env order;
* the dynamics waves partition the positions 0 .. N - 1 in order, at most 64 / dyn_lpe envs
  each, single-slot with that slot as track, or lane-varying with track -1;
* every (position, agent, ray) is cast by exactly one lane-owning task of exactly one ray wave;
  a wave that casts has its envs' slot as track (-1 lane-varying), a padding wave has count 0;
* where the table is placed (ray_order 1 and 2, lane-varying) its length is a multiple of 8 and
  the waves of the g-th 64-env group sit at indices congruent to g % 8; group-octet-major puts
  class j of group g at ((g / 8) maxw + j) 8 + g % 8; the class-major modes run the classes in
  the documented order (1 centre first, 2 ascending, 3 edge first), rank r from r * padded;
* with a tail, its classes are the last ray_tail ranks, from ray_tail_from to the end, each
  record split into ray_tail_lpr contiguous sub-records of at most 64 / ray_tail_lpr tasks
  that cover it exactly; ray_tail is 0 wherever the schedule has none (ray_order below 2,
  ray_lpr above 1, group-octet-major, wide, lane-varying);
* lane-varying schedules are single-agent at one lane per env, ray and REWARD env, dispatch 0,
  with pos_slot[p] = track_of_env[perm[p]], env_pos the inverse of perm, and no re-sort;
* the sort bins: sort_base is the running sum of (W_k >> shift) + 1, shift the smallest with
  at most 65,536 bins in all; off without sort_interval;
* argmin_window is at most the smallest W; forced schedule fields resolve to themselves.

Further tests: the automatic values just below and above each threshold of
csrc/rx_assign_plan.h, the sort bins' shift, every refusal (slot id, 17 sensors at ray_order 2,
each rx_config range of rx_create) with sentinel-filled outputs left untouched, and the
cap-and-count convention.
"""
import ctypes
import itertools

import numpy as np
import pytest

SORT_MAX_BINS = 65536

MIXES = {
    "single": [130],
    "full": [64],
    "one_each": [1] * 70,
    "ragged": [63, 1, 65, 130, 64],
    "holes": [65, 0, 0, 64, 0, 1, 130],
}


def _lib():
    from rx import _lib
    return _lib


def _config(N, A, R, ray_order, sort_interval=8, **sched):
    L = _lib()
    return L.RxConfig(N, A, R, 3000, 0, 0, 0, 1.0, 8.0, 8, sort_interval, ray_order, 8,
                      *[int(sched.get(k, 0)) for k in L.SCHED_FIELDS], 0)


def _tracks(counts, big=False):
    """(wp_off, track_of_env): slot k with 5 + 7 k waypoints (big: 2040 + k) and counts[k] envs,
    the envs of the slots interleaved by a fixed shuffle."""
    W = np.array([(2040 + k) if big else (5 + 7 * k) for k in range(len(counts))], np.int64)
    wp_off = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    toe = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    np.random.RandomState(len(toe) + len(counts)).shuffle(toe)
    return wp_off, toe


def _class_order(mode, maxw):
    off = [abs(2 * j - (maxw - 1)) for j in range(maxw)]
    if mode == 1:
        return sorted(range(maxw), key=lambda j: off[j])       # stable: centre first
    if mode == 3:
        return sorted(range(maxw), key=lambda j: -off[j])      # stable: edge first
    return list(range(maxw))


def _check(p, cfg, wp_off, toe):
    N, A, R, order = cfg.n_envs, cfg.n_agents, cfg.n_sensors, cfg.ray_order
    s = p["schedule"]
    n_tracks = len(wp_off) - 1
    perm, dyn, ray = p["perm"].astype(np.int64), p["dyn_waves"].astype(np.int64), p["ray_waves"].astype(np.int64)
    lv = bool(s["lane_tracks"])

    # ---- the schedule
    assert s["dyn_waves"] == len(dyn) and s["ray_waves"] == len(ray) and s["dyn_calls"] == 0 and s["reserved"] == 0
    assert s["wide"] == int(s["dyn_lpe"] == 64)
    assert s["split"] == int(cfg.split >= 0)
    if A == 1 and cfg.dyn_lpe:
        assert s["dyn_lpe"] == cfg.dyn_lpe
    if A == 2:
        assert s["dyn_lpe"] == 1
    if lv:
        assert A == 1 and s["dyn_lpe"] == 1 and cfg.lane_tracks >= 0
        assert s["ray_lpr"] == 1 and s["reward_lpe"] == 1 and s["ray_dispatch"] == 0 and s["ray_tail"] == 0
    else:
        assert cfg.lane_tracks != 1 or not (A == 1 and s["dyn_lpe"] == 1)
        if cfg.reward_lpe:
            assert s["reward_lpe"] == cfg.reward_lpe
        if order == 2 and s["dyn_lpe"] != 64:
            assert s["ray_lpr"] == (cfg.ray_lpr or 4)          # auto: 4 up to 8,192 (env, car) pairs
        else:
            assert s["ray_lpr"] == 1
        assert s["ray_dispatch"] == (3 if cfg.ray_dispatch == 0 else max(cfg.ray_dispatch, 0))
    assert s["ray_tail_lpr"] == (cfg.ray_tail_lpr or 2)
    assert s["task_sort"] == (cfg.task_sort or 2)               # auto: 2 up to 16,384 (env, car) pairs
    if order != 2 or s["ray_lpr"] != 1 or s["ray_dispatch"] == 0 or s["dyn_lpe"] == 64 or lv or cfg.ray_tail <= 0:
        assert s["ray_tail"] == 0 and s["ray_tail_from"] == -1
    W = np.diff(wp_off)
    want_window = 2 if cfg.argmin_window == 0 else max(cfg.argmin_window, 0)
    assert s["argmin_window"] == min(want_window, int(W.min()))

    # ---- the env order
    assert np.array_equal(np.sort(perm), np.arange(N))
    slot_at = toe[perm].astype(np.int64)
    assert np.all(np.diff(slot_at) >= 0), "grouped by slot"
    assert np.all((np.diff(slot_at) > 0) | (np.diff(perm) > 0)), "stable in env order"
    assert np.array_equal(p["slot_n"], np.bincount(toe, minlength=n_tracks))
    if lv:
        assert np.array_equal(p["pos_slot"], slot_at)
        assert np.array_equal(p["env_pos"][perm], np.arange(N))
    else:
        assert p["pos_slot"] is None and p["env_pos"] is None

    # ---- the dynamics waves
    epw = 64 if (A == 2 or lv) else 64 // s["dyn_lpe"]
    assert np.all(dyn[:, 3] >= 1) and np.all(dyn[:, 3] <= epw) and np.all(dyn[:, 2] == 0)
    assert dyn[0, 1] == 0 and np.array_equal(dyn[1:, 1], (dyn[:, 1] + dyn[:, 3])[:-1]) and dyn[-1, 1] + dyn[-1, 3] == N
    wave_of_pos = np.repeat(np.arange(len(dyn)), dyn[:, 3])
    if lv:
        assert np.all(dyn[:, 0] == -1)
        assert np.all(dyn[:-1, 3] == 64)
    else:
        assert np.array_equal(dyn[wave_of_pos, 0], slot_at), "single-slot waves with that slot as track"

    # ---- the ray waves, decoded as rays_wave does
    tail_from = s["ray_tail_from"]
    lpr = np.full(len(ray), s["ray_lpr"])
    if tail_from >= 0:
        lpr[tail_from:] = s["ray_tail_lpr"]
    cnt = ray[:, 3]
    assert np.all(cnt >= 0) and np.all(cnt * lpr <= 64), "a lane-owning task per count"
    w_id = np.repeat(np.arange(len(ray)), cnt)
    task = np.repeat(ray[:, 2], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    track, pstart = ray[w_id, 0], ray[w_id, 1]
    if lv or order == 0:
        env_local = task // (A * R)
        rem = task - env_local * (A * R)
        q, r = rem // R, rem % R
        pos = pstart + env_local
    elif order == 2:                 # through the initial task buffer: task id o at slot o
        assert task.min() >= 0 and task.max() < N * A * R
        iq, r = task // R, task % R
        pos, q = iq // A, iq % A
    else:                            # ray-major, through slot_n[track]
        ng = p["slot_n"].astype(np.int64)[track]
        qr, env_local = task // ng, task % ng
        q, r = qr // R, qr % R
        pos = pstart + env_local
    assert pos.min() >= 0 and pos.max() < N and q.min() >= 0 and q.max() < A and r.min() >= 0 and r.max() < R
    cast = np.zeros((N, A, R), np.int64)
    np.add.at(cast, (pos, q, r), 1)
    assert np.all(cast == 1), f"rays never cast: {np.argwhere(cast == 0)[:4]}, cast twice: {np.argwhere(cast > 1)[:4]}"
    assert np.array_equal(track, np.full_like(track, -1) if lv else slot_at[pos]), "a wave's track is its envs' slot"

    # ---- placement
    placed = order >= 1 or lv
    live = np.flatnonzero(cnt > 0)
    if not placed:
        assert len(live) == len(ray) and np.all(np.diff(ray[:, 1]) >= 0)
        return
    assert len(ray) % 8 == 0
    # the 64-env group of a wave, in the order the groups are made, and its class within the group
    if lv:
        group, per_group = ray[:, 1] // 64, 64 * A * R
        cls = ray[:, 2] // 64
        tpw = 64
    elif order == 2:
        group = wave_of_pos[np.minimum(ray[:, 1], N - 1)]
        tpw = 64 // s["ray_lpr"]
        cls = (ray[:, 2] - ray[:, 1] * A * R) // tpw
    else:
        ng = np.maximum(p["slot_n"].astype(np.int64)[ray[:, 0]], 1)
        blocks = (p["slot_n"].astype(np.int64) + 63) // 64
        first_group = np.cumsum(blocks) - blocks
        group = first_group[ray[:, 0]] + (ray[:, 2] % ng) // 64
        cls = ray[:, 2] // ng
        tpw = 64
    n_groups = int(group[live].max()) + 1
    padded = (n_groups + 7) // 8 * 8
    assert np.all(live % 8 == group[live] % 8), "a group's waves on one XCD"
    maxw = int(cls[live].max()) + 1
    mode, tail, m = s["ray_dispatch"], s["ray_tail"], s["ray_tail_lpr"]
    if mode == 0:
        assert len(ray) == padded * maxw
        assert np.array_equal(live, ((group[live] // 8) * maxw + cls[live]) * 8 + group[live] % 8)
        return
    can_tail = order == 2 and s["ray_lpr"] == 1 and s["dyn_lpe"] != 64
    assert tail == (min(max(cfg.ray_tail, 0), maxw) if can_tail else 0), "the last ray_tail ranks, at most all"
    assert len(ray) == padded * (maxw + tail * (m - 1))
    assert tail_from == ((maxw - tail) * padded if tail else -1)
    rank_of = np.empty(maxw, np.int64)
    rank_of[_class_order(mode, maxw)] = np.arange(maxw)
    rk = rank_of[cls[live]]
    in_tail = rk >= maxw - tail
    assert np.array_equal(in_tail, live >= tail_from) if tail else not in_tail.any()
    base = np.where(rk < maxw - tail, rk * padded, (maxw - tail) * padded + (rk - (maxw - tail)) * m * padded)
    rel = live - base
    sub = rel // padded
    assert np.all(rel >= 0) and np.all(sub < np.where(in_tail, m, 1)), "every rank in its own run of the table"
    assert np.array_equal(rel % padded, (group[live] // 8) * 8 + group[live] % 8)
    if order == 2:  # sub-record s of a tail record: its tasks from s * 64 / m on (the cover rule then makes the
        per = tpw // m  # pieces contiguous and exact); every other record starts at its class's first task
        t_rel = ray[live, 2] - ray[live, 1] * A * R - cls[live] * tpw
        assert np.array_equal(t_rel, np.where(in_tail, sub * per, 0))


def _grid():
    secondary = itertools.cycle(itertools.product((1, 2, 4), (0, 1, 3), (0, 8), (-1, 1), (0, -1, 32, 4)))
    for A, order in itertools.product((1, 2), (0, 1, 2)):
        for R in (1, 3, 11, 16) + ((17,) if order < 2 else ()):
            for mix in MIXES:
                blocks = [dict(dyn_lpe=d, ray_lpr=l, lane_tracks=t)
                          for d, l, t in itertools.product((1, 2, 4, 64) if A == 1 else (0, 1), (1, 2, 4), (-1, 0, 1))]
                blocks += [dict(dyn_lpe=1, ray_lpr=1, lane_tracks=-1, ray_dispatch=d, ray_tail=t, ray_tail_lpr=m)
                           for d, t, m in itertools.product((-1, 1, 2, 3), (-1, 1, 3, 16), (2, 4))]
                for sched in blocks:
                    rl, ts, si, sp, aw = next(secondary)
                    sched.update(reward_lpe=min(rl, 2) if A == 2 else rl, task_sort=ts, split=sp, argmin_window=aw)
                    yield A, R, order, mix, si, sched


N_PLANS = 8260


@pytest.fixture(scope="module")
def lib():
    L = _lib()
    L.load()
    return L


def test_every_plan_of_the_grid(lib):
    n = 0
    for A, R, order, mix, si, sched in _grid():
        counts = MIXES[mix]
        wp_off, toe = _tracks(counts, big=mix == "one_each")
        cfg = _config(len(toe), A, R, order, sort_interval=si, **sched)
        p = lib.assign_plan(cfg, wp_off, toe)
        try:
            _check(p, cfg, wp_off, toe)
            _check_sort(p, cfg, wp_off)
        except AssertionError as e:
            raise AssertionError(f"A={A} R={R} ray_order={order} mix={mix} sort_interval={si} {sched}: {e}") from e
        n += 1
    assert n == N_PLANS


def _check_sort(p, cfg, wp_off):
    W = np.diff(wp_off).astype(np.int64)
    if p["schedule"]["lane_tracks"] or cfg.sort_interval == 0:
        assert p["sort_bins"] == 0 and p["sort_base"] is None
        return
    totals = [int(((W >> sh) + 1).sum()) for sh in range(31)]
    shift = next((sh for sh in range(31) if totals[sh] <= SORT_MAX_BINS), None)
    if shift is None:
        assert p["sort_bins"] == 0 and p["sort_base"] is None
        return
    bins = (W >> shift) + 1
    assert p["sort_shift"] == shift and p["sort_bins"] == totals[shift]
    assert np.array_equal(p["sort_base"], np.cumsum(bins) - bins)


@pytest.mark.parametrize("n_tracks,w,shift", [(3, 2048, 0), (31, 2048, 0), (32, 2048, 1), (70, 2047, 2),
                                              (65536, 2, 2), (65537, 2, None)])
def test_sort_bins_shift(lib, n_tracks, w, shift):
    """The smallest shift with at most 65,536 bins (31 x 2,049 fit, 32 x 2,049 do not; 65,536 slots come
    down to a bin each at shift 2); more slots than bins: no re-sort."""
    wp_off = (np.arange(n_tracks + 1, dtype=np.int64) * w).astype(np.int32)
    toe = (np.arange(100) % min(n_tracks, 7)).astype(np.int32)
    cfg = _config(100, 1, 11, 2, sort_interval=8, lane_tracks=-1)
    p = lib.assign_plan(cfg, wp_off, toe)
    _check_sort(p, cfg, wp_off)
    assert (p["sort_shift"] if p["sort_bins"] else None) == shift


def _even(N, k):
    return [N // k + (i < N % k) for i in range(k)]


@pytest.mark.parametrize("A,N,sched,key,want", [
    (1, 2048, {}, "wide", 1), (1, 2049, {}, "wide", 0),                              # RX_WIDE_N
    (1, 2048, dict(wide_n=-1), "dyn_lpe", 4), (1, 2049, dict(wide_n=-1), "dyn_lpe", 1),  # RX_DYN1_SMALL_N
    (1, 8192, {}, "ray_lpr", 4), (1, 8193, {}, "ray_lpr", 2),                        # RX_RAY_LPR4_N
    (1, 16384, {}, "ray_lpr", 2), (1, 16385, {}, "ray_lpr", 1),                      # RX_RAY_LPR2_N
    (1, 4096, {}, "reward_lpe", 2), (1, 4097, {}, "reward_lpe", 1),                  # RX_REWARD_LPE2_N
    (1, 16384, {}, "task_sort", 2), (1, 16385, {}, "task_sort", 1),                  # RX_TASK_SORT2_PAIRS
    (2, 8192, {}, "task_sort", 2), (2, 8193, {}, "task_sort", 1),                    # ... in (env, car) pairs
])
def test_auto_thresholds(lib, A, N, sched, key, want):
    """Nothing forced (wide_n = -1 only where the wide kernels would hide the value): the automatic
    values of csrc/rx_assign_plan.h one env below and above each threshold."""
    wp_off, toe = _tracks(_even(N, 4))
    p = lib.assign_plan(_config(N, A, 11, 2, **sched), wp_off, toe)
    assert p["schedule"][key] == want


@pytest.mark.parametrize("k,want", [(66, 0), (67, 1)])
def test_auto_lane_tracks(lib, k, want):
    """2,049 envs fill 33 waves: slots that need 66 waves keep the grouping, 67 (more than twice) do not."""
    wp_off, toe = _tracks(_even(2049, k))
    p = lib.assign_plan(_config(2049, 1, 11, 2), wp_off, toe)
    assert p["schedule"]["lane_tracks"] == want and p["schedule"]["dyn_waves"] == (33 if want else k)


# ---- refusals --------------------------------------------------------------------------------
BAD_CONFIG = [("n_envs", 0), ("n_agents", 3), ("n_agents", 0), ("n_sensors", 0), ("n_sensors", 257), ("max_steps", 0),
              ("ray_order", 3), ("ray_order", -1), ("cull_super", 65), ("cull_super", -1), ("autoreset", 3),
              ("autoreset", -1), ("split", 2), ("seg_filter", -2), ("box_quadrants", 2), ("wide_n", -2),
              ("dyn_lpe", 3), ("dyn_lpe", 8), ("ray_lpr", 64), ("ray_lpr", 3), ("reward_lpe", 64), ("reward_lpe", -1),
              ("argmin_window", 33), ("argmin_window", -2), ("ray_dispatch", 4), ("ray_dispatch", -2),
              ("ray_tail", 17), ("ray_tail", -2), ("ray_tail_lpr", 1), ("ray_tail_lpr", 3), ("lane_tracks", 2),
              ("lane_tracks", -2), ("reserved0", 1), ("task_sort", 17), ("task_sort", -1)]


def _refused(lib, cfg, wp_off, toe, word):
    """The call is refused with RX_EINVAL and a text naming `word`, and writes nothing."""
    L = lib.load()
    N, n_tracks = max(cfg.n_envs, 1), len(wp_off) - 1
    bufs = {k: np.full(n, -7, np.int32) for k, n in (("schedule", lib.SCHEDULE_W), ("perm", N), ("dyn_waves", 4 * 4096),
                                                     ("ray_waves", 4 * 4096), ("slot_n", n_tracks), ("pos_slot", N),
                                                     ("env_pos", N), ("sort_base", n_tracks))}
    io = lib.RxAssignPlanIO(4096, 4096, -7, -7, -7, -7, *[bufs[k].ctypes.data for k in lib.ASSIGN_PLAN_PTRS])
    rc = L.rx_assign_plan(ctypes.byref(cfg), n_tracks, lib.ptr(wp_off), lib.ptr(toe), ctypes.byref(io))
    assert rc == lib.RX_EINVAL
    assert word in L.rx_last_error().decode()
    assert (io.dyn_cap, io.ray_cap, io.n_dyn_waves, io.n_ray_waves, io.sort_bins, io.sort_shift) == (4096, 4096) + (-7,) * 4
    for k, b in bufs.items():
        assert np.all(b == -7), k


@pytest.mark.parametrize("field,value", BAD_CONFIG)
def test_refuses_config_out_of_range(lib, field, value):
    wp_off, toe = _tracks([3, 4])
    cfg = _config(7, 1, 11, 2)
    setattr(cfg, field, value)
    _refused(lib, cfg, wp_off, toe, "autoreset" if field == "autoreset" else field)


def test_refuses_two_car_single_agent_schedules(lib):
    wp_off, toe = _tracks([3, 4])
    _refused(lib, _config(7, 2, 11, 2, dyn_lpe=2), wp_off, toe, "n_agents = 2")
    _refused(lib, _config(7, 2, 11, 2, reward_lpe=4), wp_off, toe, "n_agents = 2")


def test_refuses_int32_overflow(lib):
    wp_off, toe = _tracks([3, 4])                       # refused before track_of_env is read
    _refused(lib, _config(2 ** 23, 1, 256, 1), wp_off, toe, "overflows int32")
    _refused(lib, _config(2 ** 22 + 1, 2, 256, 1), wp_off, toe, "overflows int32")


@pytest.mark.parametrize("slot", [-1, 2, 2 ** 31 - 1])
def test_refuses_slot_out_of_range(lib, slot):
    wp_off, toe = _tracks([3, 4])
    toe[5] = slot
    _refused(lib, _config(7, 1, 11, 2), wp_off, toe, f"env 5 assigned to track {slot} (have 2)")


def test_refuses_17_sensors_at_ray_order_2(lib):
    wp_off, toe = _tracks([3, 4])
    _refused(lib, _config(7, 1, 17, 2), wp_off, toe, "ray_order 2 supports at most 16 sensors (got 17)")
    assert lib.assign_plan(_config(7, 1, 16, 2), wp_off, toe)["schedule"]["ray_waves"] > 0


def test_sizes_by_cap_and_count(lib):
    """A null buffer or a cap below the table's length: the two lengths and nothing else."""
    L = lib.load()
    wp_off, toe = _tracks([63, 1, 65])
    cfg = _config(129, 1, 11, 2, dyn_lpe=1)
    full = lib.assign_plan(cfg, wp_off, toe)
    nd, nr = len(full["dyn_waves"]), len(full["ray_waves"])
    for null, dyn_cap, ray_cap in ((None, nd, nr), ("perm", nd, nr), ("ray_waves", nd, nr), (0, nd - 1, nr),
                                   (0, nd, nr - 1)):
        bufs = {k: np.full(8192, -7, np.int32) for k in lib.ASSIGN_PLAN_PTRS}
        ptrs = [None if null in (None, k) else bufs[k].ctypes.data for k in lib.ASSIGN_PLAN_PTRS]
        io = lib.RxAssignPlanIO(dyn_cap, ray_cap, -7, -7, -7, -7, *ptrs)
        assert L.rx_assign_plan(ctypes.byref(cfg), 3, lib.ptr(wp_off), lib.ptr(toe), ctypes.byref(io)) == lib.RX_OK
        assert (io.n_dyn_waves, io.n_ray_waves, io.sort_bins, io.sort_shift) == (nd, nr, -7, -7)
        assert all(np.all(b == -7) for b in bufs.values())
