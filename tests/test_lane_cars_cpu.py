"""rx_assign_plan_cars / rx_set_lane_cars: the lane-varying schedule of two-car envs as the pure
planner resolves it (include/rx.h, DESIGN.md §3 "Lane-varying two-car envs"), by brute force
without a GPU.

The grid: N in {1, 63, 64, 65, 130, 4,097}; R in {1, 3, 11, 16}; every ray_order; four slot
mixes (one slot, 7 slots, one slot per env, every 4th env on a slot of its own): 288 shapes.
With the option on, every plan must be

* perm a permutation, pos_slot[p] = track_of_env[perm[p]], env_pos the inverse of perm;
* one dynamics wave per 64 positions, in order, with slot -1;
* per block, in block order, ceil(count * 2 * R / 64) ray waves with slot -1 that tile the
  block's tasks [0, count * 2 * R) in 64s (task_start relative to the block), no padding record;
* lane_tracks 1, one lane per env, ray and REWARD env, dispatch 0, no tail, no re-sort bins.

With the option off (-1) every output is rx_assign_plan's byte for byte, on sentinel-filled
buffers; with 0 the schedule is on exactly when grouping by slot needs more than
2 x ceil(N / 64) dynamics waves.  rx_config.lane_tracks never decides for two cars.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

NS = (1, 63, 64, 65, 130, 4097)
RS = (1, 3, 11, 16)
MIXES = ("one", "seven", "each", "fourth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 18  # wave records a raw call's buffers hold: above every table of the grid (ray-major, a slot per env)


@pytest.fixture(scope="module")
def lib():
    from rx import _lib
    _lib.load()
    return _lib


def _config(L, N, A, R, ray_order, sort_interval=8, **sched):
    return L.RxConfig(N, A, R, 3000, 0, 0, 0, 1.0, 8.0, 8, sort_interval, ray_order, 8,
                      *[int(sched.get(k, 0)) for k in L.SCHED_FIELDS], 0)


def _slots(N, mix):
    """(wp_off, track_of_env): slot k has 5 + (k % 50) waypoints."""
    i = np.arange(N)
    if mix == "one":
        toe = np.zeros(N, np.int64)
    elif mix == "seven":
        toe = (i * 5 + 3) % 7
    elif mix == "each":
        toe = np.random.RandomState(N).permutation(N)
    else:  # every 4th env on a slot of its own, the rest on 7 shared slots
        toe = np.where(i % 4 == 0, 7 + i // 4, i % 7)
    n_tracks = max(int(toe.max()) + 1, 7 if mix in ("seven", "fourth") else 1)
    W = 5 + np.arange(n_tracks) % 50
    return np.concatenate([[0], np.cumsum(W)]).astype(np.int32), toe.astype(np.int32)


def _grid():
    return itertools.product(NS, RS, (0, 1, 2), MIXES)


def _grouped_waves(toe):
    return int(((np.bincount(toe) + 63) // 64).sum())


def _check_on(p, N, R, wp_off, toe):
    s = p["schedule"]
    perm = p["perm"].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(N))
    assert np.array_equal(p["pos_slot"], toe[perm])
    assert np.array_equal(p["env_pos"][perm], np.arange(N))
    assert np.array_equal(p["slot_n"], np.bincount(toe, minlength=len(wp_off) - 1))
    nb = (N + 63) // 64
    cnt = np.minimum(64, N - 64 * np.arange(nb))
    dyn = p["dyn_waves"]
    assert np.array_equal(dyn, np.stack([np.full(nb, -1), 64 * np.arange(nb), np.zeros(nb, np.int64), cnt], 1))
    want = []
    for b in range(nb):
        nt = int(cnt[b]) * 2 * R
        want += [(-1, 64 * b, j, min(64, nt - j)) for j in range(0, nt, 64)]
    assert np.array_equal(p["ray_waves"], np.array(want, np.int32).reshape(-1, 4))
    assert (s["lane_tracks"], s["dyn_lpe"], s["ray_lpr"], s["reward_lpe"], s["ray_dispatch"], s["ray_tail"],
            s["ray_tail_from"], s["wide"], s["reserved"]) == (1, 1, 1, 1, 0, 0, -1, 0, 0)
    assert s["dyn_waves"] == nb and s["ray_waves"] == len(want)
    assert p["sort_bins"] == 0 and p["sort_base"] is None, "no spatial re-sort"


def test_plans_with_the_option_on(lib):
    n = 0
    for N, R, order, mix in _grid():
        wp_off, toe = _slots(N, mix)
        # rx_config.lane_tracks = -1 must not switch the option off, nor reward_lpe 2 / ray_lpr 4 survive it
        cfg = _config(lib, N, 2, R, order, lane_tracks=-1 if n % 2 else 0, reward_lpe=2 if n % 3 == 0 else 0,
                      ray_lpr=4 if n % 5 == 0 else 0, ray_tail=3 if n % 7 == 0 else 0)
        p = lib.assign_plan(cfg, wp_off, toe, lane_cars=1)
        try:
            _check_on(p, N, R, wp_off, toe)
        except AssertionError as e:
            raise AssertionError(f"N={N} R={R} ray_order={order} mix={mix}: {e}") from e
        n += 1
    assert n == 288


def _raw(lib, fn, cfg, wp_off, toe, *mode):
    """One call on sentinel-filled buffers: (rc, the io scalars, the eight buffers)."""
    L = lib.load()
    N, n_tracks = max(cfg.n_envs, 1), len(wp_off) - 1
    cap = CAP
    bufs = {k: np.full(n, -7, np.int32) for k, n in (("schedule", lib.SCHEDULE_W), ("perm", N), ("dyn_waves", 4 * cap),
                                                     ("ray_waves", 4 * cap), ("slot_n", n_tracks), ("pos_slot", N),
                                                     ("env_pos", N), ("sort_base", n_tracks))}
    io = lib.RxAssignPlanIO(cap, cap, -7, -7, -7, -7, *[bufs[k].ctypes.data for k in lib.ASSIGN_PLAN_PTRS])
    rc = getattr(L, fn)(ctypes.byref(cfg), *mode, n_tracks, lib.ptr(wp_off), lib.ptr(toe), ctypes.byref(io))
    return rc, (io.dyn_cap, io.ray_cap, io.n_dyn_waves, io.n_ray_waves, io.sort_bins, io.sort_shift), bufs


def test_option_off_is_rx_assign_plan_byte_for_byte(lib):
    for i, (N, R, order, mix) in enumerate(_grid()):
        wp_off, toe = _slots(N, mix)
        cfg = _config(lib, N, 2, R, order, lane_tracks=(0, 1, -1)[i % 3], sort_interval=(8, 0)[i % 2])
        a = _raw(lib, "rx_assign_plan", cfg, wp_off, toe)
        b = _raw(lib, "rx_assign_plan_cars", cfg, wp_off, toe, -1)
        assert a[0] == b[0] == lib.RX_OK and a[1] == b[1], (N, R, order, mix)
        for k in a[2]:
            assert a[2][k].tobytes() == b[2][k].tobytes(), (N, R, order, mix, k)
        assert a[2]["schedule"][lib.SCHEDULE_KEYS.index("lane_tracks")] == 0
        assert np.all(a[2]["pos_slot"] == -7) and np.all(a[2]["env_pos"] == -7)


def test_auto_rule_over_the_grid(lib):
    seen = set()
    for N, R, order, mix in _grid():
        wp_off, toe = _slots(N, mix)
        p = lib.assign_plan(_config(lib, N, 2, R, order), wp_off, toe, lane_cars=0)
        want = int(_grouped_waves(toe) > 2 * ((N + 63) // 64))
        assert p["schedule"]["lane_tracks"] == want, (N, R, order, mix)
        if want:
            _check_on(p, N, R, wp_off, toe)
        else:
            assert p["schedule"]["dyn_waves"] == _grouped_waves(toe) and p["pos_slot"] is None
        seen.add(want)
    assert seen == {0, 1}


@pytest.mark.parametrize("k,want", [(66, 0), (67, 1)])
def test_auto_rule_at_its_threshold(lib, k, want):
    """2,049 envs fill 33 waves: slots that need 66 waves keep the grouping, 67 (more than twice) do not."""
    N = 2049
    toe = np.repeat(np.arange(k), [N // k + (i < N % k) for i in range(k)]).astype(np.int32)
    wp_off = (np.arange(k + 1) * 9).astype(np.int32)
    p = lib.assign_plan(_config(lib, N, 2, 11, 2), wp_off, toe, lane_cars=0)
    assert p["schedule"]["lane_tracks"] == want and p["schedule"]["dyn_waves"] == (33 if want else k)


def _refused(lib, fn, cfg, wp_off, toe, mode, word):
    rc, scalars, bufs = _raw(lib, fn, cfg, wp_off, toe, *mode)
    assert rc == lib.RX_EINVAL
    assert word in lib.load().rx_last_error().decode()
    assert scalars == (CAP, CAP, -7, -7, -7, -7)
    for k, b in bufs.items():
        assert np.all(b == -7), k


def test_refusals(lib):
    wp_off, toe = _slots(7, "seven")
    _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 1, 11, 2), wp_off, toe, (1,), "n_agents = 1")
    _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 1, 11, 2), wp_off, toe, (-1,), "n_agents = 1")
    _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2), wp_off, toe, (2,), "lane_cars")
    _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2), wp_off, toe, (-2,), "lane_cars")
    # rx_config's own refusals stay, whatever the option
    for mode in (-1, 0, 1):
        _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2, reward_lpe=4), wp_off, toe, (mode,), "n_agents = 2")
        _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2, dyn_lpe=2), wp_off, toe, (mode,), "n_agents = 2")
        _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 17, 2), wp_off, toe, (mode,), "at most 16 sensors")
        _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2, lane_tracks=2), wp_off, toe, (mode,), "lane_tracks")
    bad = toe.copy()
    bad[5] = 9
    _refused(lib, "rx_assign_plan_cars", _config(lib, 7, 2, 11, 2), wp_off, bad, (1,), "env 5 assigned to track 9")
    L = lib.load()
    assert L.rx_set_lane_cars(None, 1) == lib.RX_EINVAL
    assert "rx_set_lane_cars" in L.rx_last_error().decode()


def test_abi_stays_v25_with_both_names_declared_and_exported(lib):
    L = lib.load()
    assert L.rx_abi_version() == 25
    header = open(os.path.join(ROOT, "include", "rx.h")).read()
    for name in ("rx_set_lane_cars", "rx_assign_plan_cars"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in lib.EXPORTS
    assert "#define RX_ABI_VERSION 25" in header and "#define RX_SCHEDULE_W 18" in header
