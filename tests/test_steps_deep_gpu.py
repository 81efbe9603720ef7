"""rx_steps' deep launch (DESIGN.md §3 "The deep launch").

A k_step2_pair launch advances up to RX_STEPS_DEPTH steps, ranks the ray tasks of up to as
many earlier steps in RANK workgroups of its own and casts the rays of up to as many steps
ranked before; a step's KIN, ranking and rays are three launches in a row and steps stay
queued across re-sorts.  Only where and when the work runs changes, so
``steps_device(actions[K])`` must equal K x ``step_device`` on a twin env BIT FOR BIT, as
tests/test_steps_carry_gpu.py and tests/test_steps_cross_gpu.py ask (their helpers are used
here; the SUM of the episode returns to 1e-9 relative after a warm-up or where waves share
a statistics shard, see there).  rx_steps picks the schedule by the call's length
(rx._lib.steps_plan_default: the lag-1 schedule below 20 steps, the deep one at depth 4 up to
99 steps and at the build's depth from 100 on), so the K = 25 and 40 calls, the 60- and
24-step cases run the deep launch at depth 4, the 120-step calls at full depth, and the short
calls check that the lag-1 schedule still comes out of the same planner and kernel.
"""
import ctypes
import random
import struct

import numpy as np
import pytest
import torch

from tests.test_steps_carry_gpu import SPLIT, _actions, _bufs, _close, _one_call, _per_step, _same, _twins, _venv
from tests.test_steps_cross_gpu import RET_REL, _resort_steps, _same_order, _warm

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- small ragged pool
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 25, 40)


@pytest.mark.parametrize("rows", ["per_step", "stride0"])
@pytest.mark.parametrize("sort_interval", [0, 1, 3, 8])
@pytest.mark.parametrize("task_sort", [2, 1])
def test_small_ragged_pool(golden, task_sort, sort_interval, rows):
    """200 envs over 3 slots (67 / 67 / 66: a ragged last block in every slot), the automatic
    task_sort (2 at this size: every other step is ranked, the one between reads its row) and
    task_sort 1.  Calls of every K in a row on the same twins, each against K per-step steps:
    shorter than the depth, equal to it, one more, several windows; with rows of their own per
    step and with the env's rows (stride 0: all but the newest ray step of a launch write
    shadow rows, the caller's end with the last step's)."""
    sched = dict(SPLIT) if task_sort == 2 else dict(SPLIT, task_sort=1)
    va, vb = _twins(golden, sched=sched, sort_interval=sort_interval)
    s = va.schedule()
    assert s["task_sort"] == task_sort and s["split"] == 1 and s["reward_lpe"] == 1 and s["dyn_waves"] == 6
    for K in KS:
        acts = _actions(K, 200, seed=500 + 10 * sort_interval + K)
        oa = _per_step(va, acts)
        if rows == "per_step":
            _same(va, vb, oa, _one_call(vb, acts), ret_rel=RET_REL)
        else:
            obs, rew, done = vb.steps_device(acts, full_info=True)
            assert obs is vb.buf["obs"]
            _same(va, vb, [o[-1] for o in oa], (obs, rew, done), ret_rel=RET_REL)
    if sort_interval:
        _same_order(va, vb)
    _close(va, vb)


@pytest.mark.parametrize("rows", ["per_step", "stride0"])
@pytest.mark.parametrize("sort_interval", [3, 8])
def test_long_call_at_full_depth(golden, sort_interval, rows):
    """120 steps in one call: the deep schedule at the build's full depth (8: whole windows of
    sort_interval 8 per launch, steps queued across two re-sorts; nearly three windows of
    sort_interval 3 per launch would be, but every launch ends at its re-sort step)."""
    from rx import _lib
    K = 120
    depth, lag1 = _lib.steps_plan_default(K)
    assert not lag1 and depth >= 4
    va, vb = _twins(golden, sort_interval=sort_interval)
    _warm(va, vb, phase=5)
    acts = _actions(K, 200, seed=900 + sort_interval)
    oa = _per_step(va, acts)
    if rows == "per_step":
        _same(va, vb, oa, _one_call(vb, acts), ret_rel=RET_REL)
    else:
        obs, rew, done = vb.steps_device(acts, full_info=True)
        _same(va, vb, [o[-1] for o in oa], (obs, rew, done), ret_rel=RET_REL)
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- calls in a row
def test_calls_in_a_row_with_a_reset(golden):
    """Calls of 3, 5, 8, 5 and 19 steps from two steps past a re-sort step at sort_interval 8,
    with a reset between the third and the fourth: calls that begin mid-window, steps that
    cross one re-sort and (the 19-step call at depth 8) two, and a queue that must be empty at
    the end of every call for the reset and the next call to find the state current."""
    va, vb = _twins(golden, sort_interval=8)
    _warm(va, vb, phase=2)
    lo = 0
    for i, c in enumerate((3, 5, 8, 5, 19)):
        if i == 3:
            assert torch.equal(va.reset_device(), vb.reset_device())
        acts = _actions(c, 200, seed=700 + i)
        rs = _resort_steps(va, c)
        print(f"call {i}: {c} steps, re-sort steps {rs}")
        _same(va, vb, _per_step(va, acts), _one_call(vb, acts), ret_rel=RET_REL)
        lo += c
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- episode ends
@pytest.mark.parametrize("sort_interval", [0, 8])
def test_episodes_end_in_every_sub_step(golden, sort_interval):
    """The carried file's seed-11 actions from a reset, 60 steps: episodes end from step 35
    on, so REWARD parts at every position of the sub-step loop store the flags their own
    lane's KIN part -- the next sub-step, or the k_kin1 behind a re-sort -- resets from."""
    from rx import _lib
    K = 60
    va, vb = _twins(golden, sort_interval=sort_interval)
    depth, lag1 = _lib.steps_plan_default(K)
    assert not lag1
    plan, _, _ = _lib.steps_plan(K, depth, sort_interval, va.schedule()["dyn_calls"], 1, 0, True, True, False)
    pos = {L["first_step"] + j: j for L in plan for j in range(L["n_sub"])}
    acts = _actions(K, 200, seed=11)
    oa = _per_step(va, acts)
    ended = np.flatnonzero(oa[2].bool().any(1).cpu().numpy())
    hit = sorted({pos[int(k)] for k in ended})
    print(f"episodes end at steps {ended.tolist()}: sub-step positions {hit} of {sorted(set(pos.values()))}")
    assert hit == sorted(set(pos.values())), "an episode must end at every sub-step position"
    st = _same(va, vb, oa, _one_call(vb, acts))
    assert st[2] > 0
    _close(va, vb)


# ---------------------------------------------------------------- graph replay
def test_captured_graph_replays(golden):
    """A graph captured over steps_device(19) at sort_interval 8 and replayed three times ==
    57 per-step steps on the same 19 actions: every ring counts from the start of the call, so
    a replay runs on the buffers it was captured with."""
    va, vb = _twins(golden, sort_interval=8)
    _warm(va, vb)
    acts = _actions(19, 200, seed=83)
    for _ in range(3):
        oa = _per_step(va, acts)
    ob = _bufs(vb, 19)
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
    ea, eb = va.episode_stats(), vb.episode_stats()
    assert ea[1:] == eb[1:] and abs(ea[0] - eb[0]) <= RET_REL * max(1.0, abs(ea[0])), (ea, eb)
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    del graph
    _close(va, vb)


# ---------------------------------------------------------------- distinct tracks
def test_lane_tracks_distinct_pool():
    """lane_tracks on 130 distinct tracks (three blocks, the last one ragged): the handle ranks
    nothing, so the deep launch has no RANK class and rays follow their KIN by one launch."""
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
    acts = _actions(40, 130, seed=42)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- full blocks
def test_full_blocks(golden):
    """8,256 envs x 24 steps on all golden slots, the automatic schedule, sort_interval 8: more
    than 128 dynamics waves (RANK workgroups on every XCD several times over), full blocks of
    64, re-sorts at steps 7, 15 and 23.  Several REWARD waves share an episode-statistics
    shard, so the return SUM is compared to 1e-9 relative as the existing files do; everything
    else is exact."""
    N, K = 8256, 24
    tracks = np.arange(N) % golden.n_tracks
    va, vb = (_venv(golden, tracks, sched={}, sort_interval=8) for _ in range(2))
    assert torch.equal(va.reset_device(), vb.reset_device())
    s = va.schedule()
    assert s["split"] == 1 and s["reward_lpe"] == 1 and s["wide"] == 0 and s["dyn_waves"] >= 129
    assert _resort_steps(va, K) == [7, 15, 23]
    acts = _actions(K, N, seed=64)
    _same(va, vb, _per_step(va, acts, full=False), _one_call(vb, acts, full=False), ret_rel=1e-9)
    _same_order(va, vb)
    _close(va, vb)


# ---------------------------------------------------------------- host-side refusals
def test_launch_refusals():
    """rx_launch_step2_pair checks its arguments on the host before it launches
    (hipErrorInvalidValue = 1).  The structs are filled as bytes from rx_pair_layout's offsets
    (0 to 9 as before, -1 at 10, the deep launch's from 11 on); every other field is zero (no
    waves: nothing could run).  The same fill without the offending pointer is accepted, so
    each refusal is the one named."""
    from rx import _lib
    L = _lib.load()
    lay = L.rx_pair_layout
    lay.argtypes, lay.restype = [ctypes.c_int], ctypes.c_int64
    (n_ka, o_keys, o_rows, o_hint, n_p, o_nsub, o_nrays, o_obs, o_rrows, o_rhint) = (lay(i) for i in range(10))
    assert lay(10) == -1 and lay(21) == -1
    depth, o_kin, o_snap, o_tout, o_tsnap, o_rpose, o_rtasks, o_nrank, o_kpose, o_krow = (lay(i) for i in range(11, 21))
    assert 2 <= depth <= 8 and min(o_kin, o_snap, o_tout, o_tsnap, o_rpose, o_rtasks, o_nrank, o_kpose, o_krow) > 0
    launch = L.rx_launch_step2_pair
    launch.argtypes, launch.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    A = lambda i: 0x1000 * (i + 1)  # noqa: E731 -- distinct addresses, never dereferenced
    PERM, PROG, KEYS, RSNAP, HSNAP = A(0), A(1), A(2), A(3), A(4)

    def rc(n_sub=0, n_rays=0, n_rank=0, kin=(), snap=(), tout=(), rays=(), ranks=(), keys=0, snaps=(0, 0)):
        """rays: (pose, tasks, obs, rows, hint) per ray step; ranks: (pose, row) per rank step."""
        ka, p = bytearray(n_ka), bytearray(n_p)
        for off, v in ((o_keys, keys), (o_rows, snaps[0]), (o_hint, snaps[1])):
            struct.pack_into("<Q", ka, off, v)
        for off, v in ((o_nsub, n_sub), (o_nrays, n_rays), (o_nrank, n_rank)):
            struct.pack_into("<i", p, off, v)
        for j, v in enumerate(kin):
            struct.pack_into("<i", p, o_kin + 4 * j, v)
        for base, vals in ((o_snap, snap), (o_tout, tout)):
            for j, v in enumerate(vals):
                struct.pack_into("<Q", p, base + 8 * j, v)
        for r, vals in enumerate(rays):
            for base, v in zip((o_rpose, o_rtasks, o_obs, o_rrows, o_rhint), vals):
                struct.pack_into("<Q", p, base + 8 * r, v)
        for t, vals in enumerate(ranks):
            for base, v in zip((o_kpose, o_krow), vals):
                struct.pack_into("<Q", p, base + 8 * t, v)
        a = (ctypes.c_char * n_ka).from_buffer(ka)
        b = (ctypes.c_char * n_p).from_buffer(p)
        return launch(ctypes.addressof(a), ctypes.addressof(b), None)

    ray = lambda i, **kw: tuple(kw.get(k, d) for k, d in (("pose", A(10 + i)), ("tasks", A(20 + i)),  # noqa: E731
                                                          ("obs", A(30 + i)), ("rows", PERM), ("hint", PROG)))
    # (an accepted fill has an empty grid: the launch does nothing and returns anything but the refusal code)
    # counts outside [0, depth], and all three zero
    assert rc() == 1
    for kw in (dict(n_sub=depth + 1), dict(n_sub=-1), dict(n_rays=depth + 1), dict(n_rays=-1),
               dict(n_rank=depth + 1), dict(n_rank=-1)):
        assert rc(**kw) == 1, kw
    assert rc(n_rays=1, rays=[ray(0)]) != 1
    # a KIN snapshot target equal to a ray step's or a RANK class's pose source
    assert rc(n_sub=1, kin=[1], snap=[A(10)], n_rays=1, rays=[ray(0)]) == 1
    assert rc(n_sub=2, kin=[1, 1], snap=[A(50), A(11)], n_rays=2, rays=[ray(0), ray(1)]) == 1
    assert rc(n_sub=1, kin=[1], snap=[A(40)], n_rank=1, ranks=[(A(40), A(41))]) == 1
    assert rc(n_sub=1, kin=[1], snap=[A(50)], n_rays=1, rays=[ray(0)], n_rank=1, ranks=[(A(40), A(41))]) != 1
    # a RANK output row equal to a ray step's task row, or to another RANK class's
    assert rc(n_rays=2, rays=[ray(0), ray(1)], n_rank=1, ranks=[(A(40), A(21))]) == 1
    assert rc(n_rank=2, ranks=[(A(40), A(41)), (A(42), A(41))]) == 1
    assert rc(n_rank=1, ranks=[(0, A(41))]) == 1 and rc(n_rank=1, ranks=[(A(40), 0)]) == 1
    assert rc(n_rank=2, ranks=[(A(40), A(41)), (A(42), A(43))]) != 1
    # a KIN part's own ranking into a row a ray step reads (the lag-1 schedule's rule)
    assert rc(n_sub=1, kin=[1], snap=[A(50)], tout=[A(20)], n_rays=1, rays=[ray(0)]) == 1
    # two ray steps on the same obs rows, any two of them
    if depth >= 3:
        assert rc(n_rays=3, rays=[ray(0), ray(1), ray(2, obs=A(30))]) == 1
    assert rc(n_rays=2, rays=[ray(0), ray(1, obs=A(30))]) == 1
    # a ray step on the snapshots that the launch's key-writing REWARD stores
    assert rc(n_sub=1, keys=KEYS, snaps=(RSNAP, HSNAP), n_rays=1, rays=[ray(0, rows=RSNAP)]) == 1
    assert rc(n_sub=1, keys=KEYS, snaps=(RSNAP, HSNAP), n_rays=2, rays=[ray(0), ray(1, hint=HSNAP)]) == 1
    assert rc(n_sub=1, keys=KEYS, snaps=(RSNAP, HSNAP), n_rays=1, rays=[ray(0, rows=A(5), hint=A(6))]) != 1
    # ... which a launch without sub-steps does not store: a drain launch may read them
    assert rc(n_sub=0, keys=KEYS, snaps=(RSNAP, HSNAP), n_rays=1, rays=[ray(0, rows=RSNAP, hint=HSNAP)]) != 1
    # a sub-step behind a KIN-less one, and a KIN behind the key-writing REWARD
    assert rc(n_sub=2, kin=[0, 0]) == 1
    assert rc(n_sub=1, kin=[1], snap=[A(50)], keys=KEYS) == 1
    torch.cuda.synchronize()
