"""rx_steps' carried schedule (DESIGN.md §3 "The carried step").

With the actions of all K steps on the device, rx_steps runs the KIN part of step
k + 1 (autoreset, kinematics, non-ray obs columns, the block's ray-task sort) in the
REWARD waves of step k's launch (k_step2_pair) and the ray waves read a ring of
snapshots of the stepped pose and the task rows.  Only the place the work runs
changes, so ``steps_device(actions[K])`` must equal K x ``step_device`` on a twin env
BIT FOR BIT: every step's obs / reward / done rows, the info and mask rows, the
episode statistics and the whole state -- on carried steps, on re-sort steps (which
stay plain), across calls, under graph replay, beside every ray schedule, and on the
schedules that keep the per-step launches.

The split step is forced at small N as tests/test_env_gpu.py does.  Actions come
from a CPU generator, so the episode endings the reset case relies on are the same
on every machine (checked against the oracle on the CPU when the case was chosen:
200 envs on slots 0-2, seed 11, K = 60 -- the first episode ends at step 35, and 76
episodes end before the last step).
"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPLIT = dict(wide_n=-1, dyn_lpe=1, reward_lpe=1, ray_lpr=1)
ROWS = ("info", "reward64", "terminated", "truncated", "ep_done")  # written at stride 0: the last step's


def _venv(golden, tracks, n_agents=1, sched=SPLIT, **kw):
    from rx.track import DEFAULT_CONTROL_POINTS
    from rx.vector_env import RacingVectorEnv
    cps = [golden.tracks[k]["cp"] if golden.tracks[k]["label"] != "default" else DEFAULT_CONTROL_POINTS
           for k in tracks]
    ws = [golden.tracks[k]["width"] for k in tracks]
    kw.setdefault("autoreset", "next_step")
    return RacingVectorEnv(cps, ws, n_agents=n_agents, device="cuda", sched=dict(sched), **kw)


def _actions(K, N, seed, n_agents=1):
    """Uniform random play (steer ~ U(-1, 1), throttle ~ U(0, 1)), [K, N, (A,) 2]."""
    shape = (K, N, 2) if n_agents == 1 else (K, N, n_agents, 2)
    u = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    u[..., 0] = u[..., 0] * 2 - 1
    return u.cuda().contiguous()


def _bufs(v, K):
    z = lambda name: torch.zeros((K,) + tuple(v.buf[name].shape), dtype=v.buf[name].dtype, device="cuda")  # noqa: E731
    return z("obs"), z("reward"), z("done_f32")


def _per_step(v, acts, full=True):
    """K x step_device, step k's outputs in row k."""
    out = _bufs(v, acts.shape[0])
    for k in range(acts.shape[0]):
        v.step_device(acts[k], obs_out=out[0][k], reward_out=out[1][k], done_out=out[2][k], full_info=full)
    return out


def _one_call(v, acts, full=True):
    out = _bufs(v, acts.shape[0])
    v.steps_device(acts, obs_out=out[0], reward_out=out[1], done_out=out[2], full_info=full)
    return out


def _same(va, vb, oa=None, ob=None, ret_rel=0.0):
    """Outputs, info / mask rows, episode statistics, bookkeeping and the whole state."""
    torch.cuda.synchronize()
    if oa is not None:
        for name, x, y in zip(("obs", "reward", "done"), oa, ob):
            assert torch.equal(x, y), (name, (x != y).flatten().nonzero()[:4].tolist())
    for name in ROWS:
        assert torch.equal(va.buf[name], vb.buf[name]), name
    ea, eb = va.episode_stats(reset=False), vb.episode_stats(reset=False)
    assert ea[1:] == eb[1:] and abs(ea[0] - eb[0]) <= ret_rel * max(1.0, abs(ea[0])), (ea, eb)
    assert va.schedule() == vb.schedule()  # dyn_calls: as if every step had its own dynamics launch
    sa, sb = va.get_state(), vb.get_state()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    return ea


def _twins(golden, N=200, slots=3, sched=SPLIT, **kw):
    tracks = np.arange(N) % slots
    va, vb = _venv(golden, tracks, sched=sched, **kw), _venv(golden, tracks, sched=sched, **kw)
    assert torch.equal(va.reset_device(), vb.reset_device())
    return va, vb


def _close(*vs):
    for v in vs:
        v.close()


# ---------------------------------------------------------------- case 1
@pytest.mark.parametrize("K", [1, 2, 3, 7, 40])
@pytest.mark.parametrize("sort_interval", [0, 1, 3])
def test_steps_equal_per_step(golden, sort_interval, K):
    """Three slots, 200 envs (67 / 67 / 66: a ragged last wave in every slot).
    sort_interval 0: every step but the last is carried; 1: every step is a re-sort
    step and none is; 3: carried and plain steps alternate."""
    va, vb = _twins(golden, sort_interval=sort_interval)
    assert va.schedule()["split"] == 1 and va.schedule()["reward_lpe"] == 1 and va.schedule()["dyn_waves"] == 6
    acts = _actions(K, 200, seed=100 + K)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


@pytest.mark.parametrize("sort_interval", [0, 3])
def test_steps_stride0_rows_end_with_the_last_step(golden, sort_interval):
    """K = 40 with the env's own rows (stride 0, what bench.py runs): KIN of step k + 1
    writes its non-ray columns beside step k's ray columns of the same row; once the
    call's work has completed the rows are the last step's."""
    va, vb = _twins(golden, sort_interval=sort_interval)
    acts = _actions(40, 200, seed=140)
    oa = _per_step(va, acts)
    obs, rew, done = vb.steps_device(acts, full_info=True)
    assert obs is vb.buf["obs"]
    _same(va, vb, [o[-1] for o in oa], (obs, rew, done))
    _close(va, vb)


# ---------------------------------------------------------------- case 2
def test_resets_inside_the_window(golden):
    """Episodes end -- and their envs autoreset in the carried KIN part of the next
    step -- well before the call's last step: the flags, progress and episode counters
    REWARD has just stored are what KIN reads in the same lane."""
    K = 60
    va, vb = _twins(golden, sort_interval=0)
    acts = _actions(K, 200, seed=11)
    oa = _per_step(va, acts)
    ended = oa[2][:K - 1].bool().any(1)  # steps before the last one that ended an episode
    assert ended.any() and int(ended.nonzero()[0]) < K - 2, "no episode ends inside the window"
    # the step after an ending is a reset step: reward 0, not done, for that env
    k0 = int(ended.nonzero()[0])
    e0 = oa[2][k0].bool()
    assert (oa[1][k0 + 1][e0] == 0).all() and (oa[2][k0 + 1][e0] == 0).all()
    st = _same(va, vb, oa, _one_call(vb, acts))
    assert st[2] > 0
    _close(va, vb)


# ---------------------------------------------------------------- case 3
def test_mixing_steps_and_step_calls(golden):
    """steps_device(5), step_device, steps_device(4) == 10 per-step calls."""
    va, vb = _twins(golden, sort_interval=3)
    acts = _actions(10, 200, seed=31)
    oa = _per_step(va, acts)
    ob = _bufs(vb, 10)
    vb.steps_device(acts[:5], obs_out=ob[0][:5], reward_out=ob[1][:5], done_out=ob[2][:5], full_info=True)
    vb.step_device(acts[5], obs_out=ob[0][5], reward_out=ob[1][5], done_out=ob[2][5], full_info=True)
    vb.steps_device(acts[6:], obs_out=ob[0][6:], reward_out=ob[1][6:], done_out=ob[2][6:], full_info=True)
    _same(va, vb, oa, ob)
    _close(va, vb)


def test_captured_graph_replays(golden):
    """A graph captured over steps_device(9) and replayed three times == 27 per-step
    steps (on the same 9 actions): the snapshot parity counts from the start of the
    call, so every replay runs on the buffers it was captured with."""
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
    # (the capture advanced the host's launch counter by 9 steps, not 27: the state is what counts)
    for name, x, y in zip(("obs", "reward", "done"), oa, ob):
        assert torch.equal(x, y), name
    for name in ROWS:
        assert torch.equal(va.buf[name], vb.buf[name]), name
    assert va.episode_stats() == vb.episode_stats()
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    del graph
    _close(va, vb)


# ---------------------------------------------------------------- case 4
@pytest.mark.parametrize("extra", [dict(ray_lpr=2), dict(ray_lpr=4), dict(ray_tail=2), dict(task_sort=2)],
                         ids=["ray_lpr2", "ray_lpr4", "ray_tail2", "task_sort2"])
def test_ray_schedules_beside_the_carried_waves(golden, extra):
    """The ray waves of every schedule read the snapshot; task_sort 2: the rows of the
    last sort, which the next one must not overwrite under them."""
    sched = dict(SPLIT, **extra)
    va, vb = _twins(golden, sched=sched, sort_interval=5)
    for key, val in extra.items():
        assert va.schedule()[key] == val
    acts = _actions(40, 200, seed=41)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


def test_task_sort2_first_sort_of_a_call_is_carried(golden):
    """task_sort 2 at 65,536 envs: 11,264 ray waves for 8,192 wave slots, so ray waves
    still start after the REWARD+KIN waves have sorted.  After a reset the first call
    begins between two sorts: its ray waves read the handle's task buffer and the
    call's first sort runs carried -- it must not land on the rows those waves read
    (it writes the snapshot alone; rx_launch_step2_pair refuses a launch that reads
    the buffer it sorts into, as tests/test_steps_cross_gpu.py checks of its other
    refusals, so a regression fails here whatever the timing).  The
    second call begins on a sort.  steps_device(5), steps_device(4) == 9 per-step
    calls; the return sum to 1e-9 as in test_many_blocks_per_xcd (16 waves a shard)."""
    N = 65536
    tracks = np.arange(N) % golden.n_tracks
    va, vb = _venv(golden, tracks, sched=dict(task_sort=2)), _venv(golden, tracks, sched=dict(task_sort=2))
    assert torch.equal(va.reset_device(), vb.reset_device())
    s = va.schedule()
    assert s["task_sort"] == 2 and s["split"] == 1 and s["reward_lpe"] == 1 and s["ray_waves"] > 8192
    acts = _actions(9, N, seed=43)
    oa = _per_step(va, acts, full=False)
    ob = _bufs(vb, 9)
    vb.steps_device(acts[:5], obs_out=ob[0][:5], reward_out=ob[1][:5], done_out=ob[2][:5])
    vb.steps_device(acts[5:], obs_out=ob[0][5:], reward_out=ob[1][5:], done_out=ob[2][5:])
    _same(va, vb, oa, ob, ret_rel=1e-9)
    # a call that ends right after such a sort leaves the handle's buffer to the next launch's sort
    # (ten dynamics launches so far: one step, then a 2-step call beginning between two sorts)
    vb.step_device(acts[0])
    vb.steps_device(acts[1:3])
    vb.step_device(acts[3])
    for k in range(4):
        va.step_device(acts[k])
    _same(va, vb, ret_rel=1e-9)
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
    acts = _actions(40, 130, seed=42)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


# ---------------------------------------------------------------- case 5
def test_fallback_reward_lpe2(golden):
    va, vb = _twins(golden, sched=dict(SPLIT, reward_lpe=2), sort_interval=3)
    assert va.schedule()["reward_lpe"] == 2
    acts = _actions(40, 200, seed=51)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


def test_fallback_two_cars(golden):
    tracks = np.arange(200) % 3
    mk = lambda: _venv(golden, tracks, n_agents=2, sched=dict(wide_n=-1), sort_interval=3, seed=5)  # noqa: E731
    va, vb = mk(), mk()
    assert torch.equal(va.reset_device(), vb.reset_device())
    acts = _actions(40, 200, seed=52, n_agents=2)
    _same(va, vb, _per_step(va, acts), _one_call(vb, acts))
    _close(va, vb)


def test_fallback_profile_lists_both_kernels(golden):
    va, vb = _twins(golden, sort_interval=3)
    acts = _actions(12, 200, seed=53)
    oa = _per_step(va, acts)
    vb.profile(1)
    ob = _one_call(vb, acts)
    vb.profile(0)
    prof = vb.profile_read()
    assert prof["k_kin1"][1] == 12 and prof["k_step2"][1] == 12, prof
    _same(va, vb, oa, ob)
    _close(va, vb)


def test_fallback_counters(golden):
    va, vb = _twins(golden, sort_interval=3)
    acts = _actions(12, 200, seed=54)
    oa = _per_step(va, acts)
    vb.enable_counters(True)
    ob = _one_call(vb, acts)
    cnt = vb.read_counters()
    assert cnt["ray_chunk_tests"] > 0 and cnt["wp_chunk_tests"] > 0  # both halves counted their box tests
    vb.enable_counters(False)
    _same(va, vb, oa, ob)
    _close(va, vb)


# ---------------------------------------------------------------- case 6
def test_many_blocks_per_xcd(golden):
    """8,256 envs x 24 steps on all golden slots, the automatic schedule (2 lanes per ray,
    task sort every other launch), without the info rows -- bench.py's io.  Several
    REWARD waves share an episode-statistics shard here and their f64 atomics land in
    any order within a launch (in both envs), so the return SUM is compared to 1e-9
    relative as tests/test_env_gpu.py does for that reason; counts, lengths and every
    env's own ep_return (the state) are exact."""
    N, K = 8256, 24
    tracks = np.arange(N) % golden.n_tracks
    va, vb = _venv(golden, tracks, sched={}), _venv(golden, tracks, sched={})
    assert torch.equal(va.reset_device(), vb.reset_device())
    s = va.schedule()
    assert s["split"] == 1 and s["reward_lpe"] == 1 and s["wide"] == 0 and s["dyn_waves"] >= 129
    acts = _actions(K, N, seed=61)
    _same(va, vb, _per_step(va, acts, full=False), _one_call(vb, acts, full=False), ret_rel=1e-9)
    _close(va, vb)
