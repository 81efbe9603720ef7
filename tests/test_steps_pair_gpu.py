"""rx_steps' paired schedule (DESIGN.md §3 "The paired launch").

A paired launch's REWARD workgroups advance two steps (REWARD k, KIN k + 1, REWARD
k + 1, KIN k + 2) and its ray workgroups cast the rays of the two steps whose KIN
parts an earlier launch completed, from rings of four pose / task-row snapshots.
Only where and when the work runs changes, so ``steps_device(actions[K])`` must equal
K x ``step_device`` on a twin env BIT FOR BIT, exactly as tests/test_steps_carry_gpu.py
asks of the carried schedule (its helpers are used here): every step's obs / reward /
done rows, the info and mask rows, the episode statistics, ``schedule()`` and the whole
state -- for every K and re-sort interval that changes the shape of the launch program
(one or two sub-steps, one or two ray steps, the KIN-less last sub-step before a sort
or the end of the call), at stride 0 (the older ray step of a launch writes shadow
rows), across calls, under graph replay, and on the schedules that fall back.
"""
import random

import numpy as np
import pytest
import torch

from tests.test_steps_carry_gpu import (SPLIT, _actions, _bufs, _close, _one_call, _per_step, _same, _twins,
                                        _venv)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- per-step equivalence
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 7, 9, 40])
@pytest.mark.parametrize("sort_interval", [0, 1, 2, 3, 8])
def test_steps_equal_per_step(golden, sort_interval, K):
    """Three slots, 200 envs (67 / 67 / 66: a ragged last wave in every slot).
    sort_interval 0: pairs all the way, the call's last step plain or (K odd from 3)
    KIN-less beside two ray steps; 1: every step is a re-sort step; 2 and 3: single
    sub-steps and pairs between the sorts; 8: the window of the full-size run."""
    va, vb = _twins(golden, sort_interval=sort_interval)
    assert va.schedule()["split"] == 1 and va.schedule()["reward_lpe"] == 1 and va.schedule()["dyn_waves"] == 6
    acts = _actions(K, 200, seed=200 + K)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- stride-0 outputs
@pytest.mark.parametrize("K", [8, 9])
@pytest.mark.parametrize("sort_interval", [0, 3])
def test_stride0_rows_end_with_the_last_step(golden, sort_interval, K):
    """The env's own rows (stride 0, what bench.py runs): two ray steps of one launch
    would write the same obs rows, so the older one writes shadow rows; once the call's
    work has completed the caller's rows are the last step's."""
    va, vb = _twins(golden, sort_interval=sort_interval)
    acts = _actions(K, 200, seed=240 + K)
    oa = _per_step(va, acts)
    obs, rew, done = vb.steps_device(acts, full_info=True)
    assert obs is vb.buf["obs"]
    _same(va, vb, [o[-1] for o in oa], (obs, rew, done))
    _close(va, vb)


# ---------------------------------------------------------------- several calls, replay, reset
def test_calls_in_a_row(golden):
    """steps_device(3), (5), (8), then (5) again mid-window == 21 per-step calls: the
    snapshot rings and the queue of pending ray steps start clean with every call."""
    va, vb = _twins(golden, sort_interval=8)
    acts = _actions(21, 200, seed=31)
    oa = _per_step(va, acts)
    ob = _bufs(vb, 21)
    lo = 0
    for n in (3, 5, 8, 5):
        sl = slice(lo, lo + n)
        vb.steps_device(acts[sl], obs_out=ob[0][sl], reward_out=ob[1][sl], done_out=ob[2][sl], full_info=True)
        lo += n
    _same(va, vb, oa, ob)
    _close(va, vb)


def test_reset_between_calls(golden):
    va, vb = _twins(golden, sort_interval=3)
    acts = _actions(12, 200, seed=33)
    ob = _bufs(vb, 12)
    oa = _bufs(va, 12)
    for lo, hi in ((0, 7), (7, 12)):
        for k in range(lo, hi):
            va.step_device(acts[k], obs_out=oa[0][k], reward_out=oa[1][k], done_out=oa[2][k], full_info=True)
        vb.steps_device(acts[lo:hi], obs_out=ob[0][lo:hi], reward_out=ob[1][lo:hi], done_out=ob[2][lo:hi],
                        full_info=True)
        if hi == 7:
            assert torch.equal(va.reset_device(), vb.reset_device())
    _same(va, vb, oa, ob)
    _close(va, vb)


def test_captured_graph_replays(golden):
    """A graph captured over steps_device(9) and replayed three times == 27 per-step
    steps (on the same 9 actions): ring slots count from the start of the call, so every
    replay runs on the buffers it was captured with."""
    va, vb = _twins(golden, sort_interval=0)
    acts = _actions(9, 200, seed=32)
    for _ in range(3):
        oa = _per_step(va, acts)
    ob = _bufs(vb, 9)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap, capture_error_mode="thread_local"):
        vb.steps_device(acts, obs_out=ob[0], reward_out=ob[1], done_out=ob[2], full_info=True)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for name, x, y in zip(("obs", "reward", "done"), oa, ob):
        assert torch.equal(x, y), name
    for name in ("info", "reward64", "terminated", "truncated", "ep_done"):
        assert torch.equal(va.buf[name], vb.buf[name]), name
    assert va.episode_stats() == vb.episode_stats()
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    del graph
    _close(va, vb)


# ---------------------------------------------------------------- task sort, resets, lane-varying slots
@pytest.mark.parametrize("sort_interval", [0, 5])
def test_task_sort2(golden, sort_interval):
    """task_sort 2: one KIN part in two sorts, so the two ray steps of a launch read the
    same row or two rows of the ring, and a call beginning between two sorts reads the
    handle's buffer while its first sorts write the ring alone."""
    va, vb = _twins(golden, sched=dict(SPLIT, task_sort=2), sort_interval=sort_interval)
    assert va.schedule()["task_sort"] == 2
    acts = _actions(40, 200, seed=41)
    oa = _per_step(va, acts)
    ob = _bufs(vb, 40)
    lo = 0
    for n in (5, 4, 31):  # the second call begins between two sorts
        sl = slice(lo, lo + n)
        vb.steps_device(acts[sl], obs_out=ob[0][sl], reward_out=ob[1][sl], done_out=ob[2][sl], full_info=True)
        lo += n
    _same(va, vb, oa, ob)
    # a call that leaves the handle's task buffer behind: the next launches sort it
    vb.step_device(acts[0])
    vb.steps_device(acts[1:3])
    vb.step_device(acts[3])
    for k in range(4):
        va.step_device(acts[k])
    _same(va, vb)
    _close(va, vb)


def test_resets_inside_second_sub_steps(golden):
    """The carried file's seed-11 case: episodes end from step 35 on, so envs autoreset in
    KIN parts that follow a REWARD part of the SAME launch, and in its second sub-step."""
    K = 60
    va, vb = _twins(golden, sort_interval=0)
    acts = _actions(K, 200, seed=11)
    oa = _per_step(va, acts)
    ended = oa[2][:K - 1].bool().any(1)
    assert ended.any() and int(ended.nonzero()[0]) < K - 2, "no episode ends inside the window"
    assert bool(ended[0::2].any()) and bool(ended[1::2].any())  # endings in first and in second sub-steps
    st = _same(va, vb, oa, _one_call(vb, acts))
    assert st[2] > 0
    _close(va, vb)


def test_lane_tracks_distinct_pool():
    """lane_tracks on 130 distinct tracks (three blocks, the last one ragged)."""
    from rx.track import TrackSet, gen_tracks
    from rx.vector_env import RacingVectorEnv
    random.seed(1)
    np.random.seed(1)
    pool = gen_tracks(num_tracks=130, seed=None)
    widths = [np.random.randint(6, 10) for _ in range(130)]
    ts = TrackSet.build(pool, widths)
    mk = lambda: RacingVectorEnv(pool, widths, device="cuda", autoreset="next_step", track_set=ts,  # noqa: E731
                                 sched=dict(SPLIT, lane_tracks=1))
    va, vb = mk(), mk()
    assert va.schedule()["lane_tracks"] == 1 and va.schedule()["split"] == 1
    assert torch.equal(va.reset_device(), vb.reset_device())
    acts = _actions(21, 130, seed=42)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- fallbacks
def test_fallback_reward_lpe2(golden):
    va, vb = _twins(golden, sched=dict(SPLIT, reward_lpe=2), sort_interval=3)
    assert va.schedule()["reward_lpe"] == 2
    acts = _actions(12, 200, seed=51)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


def test_fallback_two_cars(golden):
    tracks = np.arange(200) % 3
    mk = lambda: _venv(golden, tracks, n_agents=2, sched=dict(wide_n=-1), sort_interval=3, seed=5)  # noqa: E731
    va, vb = mk(), mk()
    assert torch.equal(va.reset_device(), vb.reset_device())
    acts = _actions(12, 200, seed=52, n_agents=2)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- full blocks, a re-sort window
def test_full_blocks_and_a_resort_window(golden):
    """8,256 envs x 16 steps on all golden slots, the automatic schedule and bench.py's
    io (no info rows): more than 64 envs per slot, full blocks, and a whole re-sort
    window of paired launches (two of them: re-sorts at steps 0 and 8).  Several REWARD waves share an episode-statistics shard
    and their f64 atomics land in any order within a launch (in both envs), so the
    return SUM is compared to 1e-9 relative as tests/test_steps_carry_gpu.py does;
    everything else is exact."""
    N, K = 8256, 16
    tracks = np.arange(N) % golden.n_tracks
    va, vb = (_venv(golden, tracks, sched={}, sort_interval=8) for _ in range(2))  # the full-size run's window
    assert torch.equal(va.reset_device(), vb.reset_device())
    s = va.schedule()
    assert s["split"] == 1 and s["reward_lpe"] == 1 and s["wide"] == 0 and s["dyn_waves"] >= 129
    acts = _actions(K, N, seed=61)
    _same(va, vb, _per_step(va, acts, full=False), _one_call(vb, acts, full=False), ret_rel=1e-9)
    _close(va, vb)
