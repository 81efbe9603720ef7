"""rx_steps' crossing step (DESIGN.md §3 "The crossing step").

A step whose re-sort is due, and which a step follows in the call, gives up its own
launch: its REWARD part runs as the KIN-less second sub-step of the launch before it
(writing the sort keys, and snapshots of the row ids and of the visiting-order hint),
and its rays are cast AFTER the sort, in the next window's first paired launch, from
the pose / task-row rings and those snapshots.  Only where and when the work runs
changes, so ``steps_device(actions[K])`` must equal K x ``step_device`` on a twin env
BIT FOR BIT, exactly as tests/test_steps_carry_gpu.py asks (its helpers are used here):
every step's obs / reward / done rows, the info and mask rows, the episode statistics,
``schedule()`` and the whole state (the cases that warm up first: the SUM of the episode
returns to RET_REL, see there; every env's own return is part of the state and exact).
"""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests.test_steps_carry_gpu import (SPLIT, _actions, _bufs, _close, _one_call, _per_step, _same, _twins,
                                        _venv)

pytestmark = pytest.mark.gpu

WARM = 24  # at least this many untimed steps before the compared ones
# The return SUM of the episode statistics after a warm-up.  A re-sort ranks the envs of one
# sort bin by the arrival order of the REWARD waves' histogram atomics, so after the first
# re-sort that finds several cars in a bin the two twins hold the same envs in a different
# row order -- whatever schedule either of them runs -- and the per-wave partial sums of the
# returns are taken over different env sets.  The sum is then equal up to the reordering of
# an f64 sum, which is what tests/test_steps_carry_gpu.py allows where waves share a shard
# (1e-9 relative); counts, lengths, every env's own ep_return and everything else stay exact.
# (Seen with an exact comparison: -1351.5721750487198 against -1351.57217504872 over 27
# episodes, one ulp, in a case whose calls cross and in the twins' row orders of a call
# that does not cross at all.)
RET_REL = 1e-9


def _warm(va, vb, phase=0, seed=7):
    """The same per-step steps on both twins, so the cars have spread over the sort bins
    (after a reset every car of a slot stands in one bin and a re-sort moves nothing):
    WARM of them and as many more as leave the next step `phase` steps past a re-sort step
    (the reset launch counts in dyn_calls too)."""
    si, d0 = va.sort_interval, va.schedule()["dyn_calls"]
    n = WARM + (phase - d0 - WARM) % si
    acts = _actions(n, va.num_envs, seed=seed)
    for k in range(n):
        va.step_device(acts[k])
        vb.step_device(acts[k])


def _resort_steps(v, K):
    """The steps of a K-step call that begins now whose re-sort is due."""
    si, d0 = v.sort_interval, v.schedule()["dyn_calls"]
    return [k for k in range(K) if (d0 + k) % si == 0]


def _same_order(va, vb):
    """Both row permutations are permutations and put the same slot at every position (the
    re-sort keeps slot groups in place).  Within a sort bin the order is the arrival order
    of the REWARD waves' histogram atomics, in per-step launches too, so it is not compared."""
    pa, pb = va.env_order()[0], vb.env_order()[0]
    n = va.num_envs
    assert np.array_equal(np.sort(pa), np.arange(n)) and np.array_equal(np.sort(pb), np.arange(n))
    slot = va.get_state()["track"]
    assert np.array_equal(slot[pa], slot[pb])


def _per_step_orders(v, acts):
    """_per_step, and the row permutation before the call and after every step."""
    out = _bufs(v, acts.shape[0])
    perms = [v.env_order()[0].copy()]
    for k in range(acts.shape[0]):
        v.step_device(acts[k], obs_out=out[0][k], reward_out=out[1][k], done_out=out[2][k], full_info=True)
        perms.append(v.env_order()[0].copy())
    return out, perms


# ---------------------------------------------------------------- every phase of the window
@pytest.mark.parametrize("kk", ["si+1", "si+2", "2si+1", "3si+2"])
@pytest.mark.parametrize("sort_interval", [2, 3, 4, 8])
def test_crossings_at_every_phase(golden, sort_interval, kk):
    """Three slots, 200 envs (67 / 67 / 66: a ragged last wave in every slot).  The call
    begins on a re-sort step, so K = si + 1 ends on one (no crossing), si + 2 crosses once
    with one step behind it, 2 si + 1 crosses once and ends on a re-sort step, 3 si + 2
    crosses three times.  At 3 si + 2 a crossed sort must have moved rows: the snapshots
    are then what keeps the crossing step's obs rows right."""
    si = sort_interval
    K = {"si+1": si + 1, "si+2": si + 2, "2si+1": 2 * si + 1, "3si+2": 3 * si + 2}[kk]
    va, vb = _twins(golden, sort_interval=si)
    assert va.schedule()["split"] == 1 and va.schedule()["reward_lpe"] == 1 and va.schedule()["dyn_waves"] == 6
    _warm(va, vb)
    rs = _resort_steps(va, K)
    assert rs[0] == 0 and rs == _resort_steps(vb, K)
    crossed = [k for k in rs if k >= 1 and k + 1 < K]
    assert len(crossed) == {"si+1": 0, "si+2": 1, "2si+1": 1, "3si+2": 3}[kk]
    acts = _actions(K, 200, seed=300 + 10 * si + K)
    oa, perms = _per_step_orders(va, acts)
    moved = [k for k in crossed if not np.array_equal(perms[k], perms[k + 1])]
    print(f"sort_interval {si} K {K}: re-sorts at {rs}, crossed {crossed}, moved rows at {moved}")
    if kk == "3si+2":
        assert moved, "no crossed re-sort moved a row: the case is vacuous"
    _same(va, vb, oa, _one_call(vb, acts), ret_rel=RET_REL)
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- the call ends on the re-sort step
def test_last_step_is_the_resort_step(golden):
    """K = 9 from a re-sort step at sort_interval 8: step 8 is the call's last, so it
    keeps its own launch (REWARD and rays before the sort) and nothing is pending at
    return: a per-step step on both twins still agrees."""
    va, vb = _twins(golden, sort_interval=8)
    _warm(va, vb)
    assert _resort_steps(va, 9) == [0, 8]
    acts = _actions(10, 200, seed=71)
    oa = _per_step(va, acts[:9])
    _same(va, vb, oa, _one_call(vb, acts[:9]), ret_rel=RET_REL)
    _same_order(va, vb)
    o1, o2 = _per_step(va, acts[9:]), _per_step(vb, acts[9:])
    _same(va, vb, o1, o2, ret_rel=RET_REL)
    _close(va, vb)


# ---------------------------------------------------------------- stride-0 outputs
@pytest.mark.parametrize("K", [9, 17])
def test_stride0_rows_end_with_the_last_step(golden, K):
    """The env's own rows (stride 0, what bench.py runs) with the call beginning one step
    before a re-sort step, so steps 1 (and 9) cross with a step behind them at K = 9
    (17): the crossing step is the older ray step of its launch and writes the shadow
    rows; the caller's rows end with the last step's."""
    va, vb = _twins(golden, sort_interval=8)
    _warm(va, vb, phase=7)
    assert _resort_steps(va, K) == list(range(1, K, 8))
    acts = _actions(K, 200, seed=340 + K)
    oa = _per_step(va, acts)
    obs, rew, done = vb.steps_device(acts, full_info=True)
    assert obs is vb.buf["obs"]
    _same(va, vb, [o[-1] for o in oa], (obs, rew, done), ret_rel=RET_REL)
    _close(va, vb)


# ---------------------------------------------------------------- calls that begin mid-window
@pytest.mark.parametrize("task_sort", [1, 2, 4])
@pytest.mark.parametrize("calls", [(3, 5, 8, 5), (7, 2, 9)], ids=["3-5-8-5", "7-2-9"])
def test_calls_in_a_row_mid_window(golden, calls, task_sort):
    """Calls that begin between two re-sorts, the first one two steps past a re-sort step:
    (3, 5, 8, 5) crosses in its second and third call, (7, 2, 9) ends its first call on
    the re-sort step and crosses in its third.  task_sort > 1: a call that begins between
    two TASK sorts reads the handle's task buffer until its first sort; a step that would
    cross on that buffer (task_sort 4: no sort in the call yet) keeps its own launch
    instead, because the k_kin1 behind the re-sort rewrites the buffer."""
    sched = dict(SPLIT, task_sort=task_sort)  # (the automatic value is 2 at this size)
    va, vb = _twins(golden, sched=sched, sort_interval=8)
    assert va.schedule()["task_sort"] == task_sort
    _warm(va, vb, phase=2)
    n = sum(calls)
    acts = _actions(n, 200, seed=360 + n + task_sort)
    oa = _per_step(va, acts)
    ob = _bufs(vb, n)
    lo = 0
    for c in calls:
        sl = slice(lo, lo + c)
        vb.steps_device(acts[sl], obs_out=ob[0][sl], reward_out=ob[1][sl], done_out=ob[2][sl], full_info=True)
        lo += c
    _same(va, vb, oa, ob, ret_rel=RET_REL)
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- graph replay
def test_captured_graph_replays(golden):
    """A graph captured over steps_device(17) at sort_interval 8 (re-sorts at steps 0, 8
    and 16; 8 crosses, 16 is the call's last) and replayed three times == 51 per-step
    steps on the same 17 actions: the snapshot rings count from the start of the call,
    so every replay runs on the buffers it was captured with."""
    va, vb = _twins(golden, sort_interval=8)
    _warm(va, vb)
    acts = _actions(17, 200, seed=82)
    for _ in range(3):
        oa = _per_step(va, acts)
    ob = _bufs(vb, 17)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap, capture_error_mode="thread_local"):
        vb.steps_device(acts, obs_out=ob[0], reward_out=ob[1], done_out=ob[2], full_info=True)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    # (the capture advanced the host's launch counter by 17 steps, not 51: the state is what counts)
    for name, x, y in zip(("obs", "reward", "done"), oa, ob):
        assert torch.equal(x, y), name
    for name in ("info", "reward64", "terminated", "truncated", "ep_done"):
        assert torch.equal(va.buf[name], vb.buf[name]), name
    ea, eb = va.episode_stats(), vb.episode_stats()
    assert ea[1:] == eb[1:] and abs(ea[0] - eb[0]) <= RET_REL * max(1.0, abs(ea[0])), (ea, eb)
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    del graph
    _close(va, vb)


# ---------------------------------------------------------------- resets around the crossing
def test_resets_around_the_crossing(golden):
    """The carried file's seed-11 case from a reset (episodes end from step 35 on), K = 60,
    sort_interval 8: re-sorts at steps 7, 15, ..., 55 (the reset was launch 0), all crossed.  Episodes
    end in key-writing REWARD sub-steps (their envs autoreset in the k_kin1 behind the
    sort) and in the step after a sort (the first sub-step of the launch that casts the
    crossing step)."""
    K = 60
    va, vb = _twins(golden, sort_interval=8)
    rs = _resort_steps(va, K)
    assert rs == list(range(7, K, 8))
    acts = _actions(K, 200, seed=11)
    oa = _per_step(va, acts)
    ended = oa[2].bool().any(1).cpu().numpy()
    in_keys = [k for k in rs if ended[k]]
    after = [k + 1 for k in rs if ended[k + 1]]
    print(f"episodes end at steps {np.flatnonzero(ended).tolist()}; key-writing {in_keys}, after a sort {after}")
    assert in_keys, "no episode ends in a key-writing REWARD sub-step"
    assert after, "no episode ends in the step after a sort"
    st = _same(va, vb, oa, _one_call(vb, acts))
    assert st[2] > 0
    _close(va, vb)


# ---------------------------------------------------------------- fallbacks
def test_fallback_reward_lpe2(golden):
    va, vb = _twins(golden, sched=dict(SPLIT, reward_lpe=2), sort_interval=3)
    assert va.schedule()["reward_lpe"] == 2
    acts = _actions(11, 200, seed=91)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


def test_fallback_two_cars(golden):
    tracks = np.arange(200) % 3
    mk = lambda: _venv(golden, tracks, n_agents=2, sched=dict(wide_n=-1), sort_interval=3, seed=5)  # noqa: E731
    va, vb = mk(), mk()
    assert torch.equal(va.reset_device(), vb.reset_device())
    acts = _actions(11, 200, seed=92, n_agents=2)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- full blocks
def test_full_blocks_two_crossings(golden):
    """8,256 envs x 24 steps on all golden slots, the automatic schedule, sort_interval 8:
    re-sorts at steps 7, 15 and 23 (the reset was launch 0), the first two crossed.  Several REWARD waves share an
    episode-statistics shard and their f64 atomics land in any order within a launch (in
    both envs), so the return SUM is compared to 1e-9 relative as
    tests/test_steps_pair_gpu.py::test_full_blocks_and_a_resort_window does; everything
    else is exact."""
    N, K = 8256, 24
    tracks = np.arange(N) % golden.n_tracks
    va, vb = (_venv(golden, tracks, sched={}, sort_interval=8) for _ in range(2))
    assert torch.equal(va.reset_device(), vb.reset_device())
    s = va.schedule()
    assert s["split"] == 1 and s["reward_lpe"] == 1 and s["wide"] == 0 and s["dyn_waves"] >= 129
    assert _resort_steps(va, K) == [7, 15, 23]
    acts = _actions(K, N, seed=63)
    _same(va, vb, _per_step(va, acts, full=False), _one_call(vb, acts, full=False), ret_rel=1e-9)
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- host-side refusal
def test_launch_refuses_a_ray_step_on_the_snapshots_it_stores():
    """rx_launch_step2_pair checks its arguments on the host before it launches: a ray step
    that reads the row-id or the hint snapshot which the same launch's key-writing REWARD
    stores is refused (hipErrorInvalidValue = 1).  The structs are filled as bytes from
    rx_pair_layout's offsets; every other field is zero (no waves: nothing could run)."""
    from rx import _lib
    L = _lib.load()
    lay = L.rx_pair_layout
    lay.argtypes, lay.restype = [ctypes.c_int], ctypes.c_int64
    (n_ka, o_keys, o_rows, o_hint, n_p, o_nsub, o_nrays, o_obs, o_rrows, o_rhint) = (lay(i) for i in range(10))
    assert lay(10) == -1 and min(n_ka, o_keys, o_rows, o_hint, n_p, o_nrays, o_obs, o_rrows, o_rhint) > 0
    launch = L.rx_launch_step2_pair
    launch.argtypes, launch.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    KEYS, ROWS_A, HINT_A, ROWS_B, HINT_B, PERM, PROG, OBS = (0x1000 * (i + 1) for i in range(8))  # never dereferenced

    def rc(n_rays, rows, hints, keys=KEYS, rows_snap=ROWS_A, hint_snap=HINT_A):
        ka, p = bytearray(n_ka), bytearray(n_p)
        for off, v in ((o_keys, keys), (o_rows, rows_snap), (o_hint, hint_snap)):
            struct.pack_into("<Q", ka, off, v)
        struct.pack_into("<i", p, o_nsub, 1)
        struct.pack_into("<i", p, o_nrays, n_rays)
        for r in range(n_rays):
            struct.pack_into("<Q", p, o_obs + 8 * r, OBS + 64 * r)
            struct.pack_into("<Q", p, o_rrows + 8 * r, rows[r])
            struct.pack_into("<Q", p, o_rhint + 8 * r, hints[r])
        a = (ctypes.c_char * n_ka).from_buffer(ka)
        b = (ctypes.c_char * n_p).from_buffer(p)
        return launch(ctypes.addressof(a), ctypes.addressof(b), None)

    assert rc(1, [ROWS_A], [PROG]) == 1            # the row ids it stores
    assert rc(1, [PERM], [HINT_A]) == 1            # the hint it stores
    assert rc(2, [ROWS_B, ROWS_A], [HINT_B, PROG]) == 1   # the newer ray step
    assert rc(2, [ROWS_A, PERM], [HINT_A, PROG]) == 1     # the older one (the crossing step's place)
    assert rc(1, [0], [PROG]) == 1 and rc(1, [PERM], [0]) == 1   # a ray step without row ids / a hint
    assert rc(1, [PERM], [PROG], hint_snap=0) == 1                # row-id snapshot without the hint's
    torch.cuda.synchronize()
