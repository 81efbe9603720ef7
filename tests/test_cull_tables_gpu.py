"""Resident track tables on the GPU: the culling-table kernel (rx_build_cull_tables,
csrc/rx_cull.hip) against its host twin, the device door into an env
(rx_upload_tracks_device, RacingVectorEnv.set_tracks) against the host door
(rx_upload_tracks) step for step, a swapped env against a fresh one, a refused
swap, DeviceTrackTable and PPO's track resampling.

Every C-level output buffer carries a guard element past its end.  The tables are
equal by value (tests/test_cull_tables_cpu.py explains the zeros) except the
circle radius, which goes through the platform's hypot: an upper bound of the
largest np.hypot distance, within 1e-13 relative of max_hypot * (1 + 1e-12) + 1e-9
and of the host twin's value.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.test_cull_tables_cpu import (DTYPES, GUARD, PARAMS, TABLES, buffer_sizes, check_against, decode,
                                        host_build, make_table, np_tables, tables_struct)

pytestmark = pytest.mark.gpu

TABLES = dict(TABLES)
# 130 slots: crosses the 64 and 128 slot boundaries of any lane-per-slot mapping and leaves the
# last workgroup of 4 wavefronts half empty; then the smallest and the largest slot alone
TABLES["slots130"] = lambda: make_table([(3, 4, 6, 10)[k % 4] for k in range(130)], 3)
TABLES["one_w3"] = lambda: make_table((3,), 4)
TABLES["one_w2048"] = lambda: make_table((2048,), 5)
_TORCH = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
_cache = {}


def _table(name):
    """The table, the host twin's output per (G, SG) and the restatement's max_hypot, computed once."""
    if name not in _cache:
        t = TABLES[name]()
        _cache[name] = (t, {}, np_tables(t, 8, 0)[1])
    return _cache[name]


def _device_build(t, G, SG):
    """rx_build_cull_tables into guarded device buffers on torch's current stream; the first wait is the download."""
    from rx import _lib
    L = _lib.load()
    up = {k: torch.from_numpy(t[k]).cuda() for k in ("wp", "seg", "meta")}
    bufs = {k: torch.full((m + 1,), GUARD, dtype=_TORCH[DTYPES[k]], device="cuda")
            for k, m in buffer_sizes(t, G, SG).items()}
    st = tables_struct(bufs)
    _lib.check(L.rx_build_cull_tables(len(t["wp_off"]) - 1, _lib.ptr(t["wp_off"]), _lib.ptr(up["wp"]),
                                      _lib.ptr(up["seg"]), _lib.ptr(up["meta"]), G, SG, ctypes.byref(st),
                                      _lib.stream_ptr()), "rx_build_cull_tables")
    return {k: v.cpu().numpy() for k, v in bufs.items()}


@pytest.mark.parametrize("G,SG", PARAMS)
@pytest.mark.parametrize("name", list(TABLES))
def test_kernel_equals_host_twin(name, G, SG):
    t, host, reach = _table(name)
    if (G, SG) not in host:
        host[(G, SG)] = decode(host_build(t, G, SG))
    want = host[(G, SG)]
    got = decode(_device_build(t, G, SG))
    check_against(got, want, reach if G > 0 else None, f"{name} G={G} SG={SG}")
    if G > 0:  # and against the host's own radius
        for k in ("slot_geo", "hdr_f"):
            a, b = got[k].reshape(len(reach), -1)[:, 2], want[k].reshape(len(reach), -1)[:, 2]
            assert np.all(np.abs(a - b) <= 1e-13 * b), (name, k)


# ---------------------------------------------------------------- the two doors into an env
def _tracks(n, seed):
    from rx.track import gen_tracks
    random.seed(seed)
    np.random.seed(seed)
    return gen_tracks(num_tracks=n, seed=None)


def _actions(g, N, A):
    a = torch.rand((N, 2) if A == 1 else (N, A, 2), device="cuda", generator=g) * 2 - 1
    a[..., 1].abs_()
    return a


def _same_step(va, vb, a, t):
    oa, ra, da = va.step_device(a)
    ob, rb, db = vb.step_device(a)
    assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
    for k in ("terminated", "truncated"):
        assert torch.equal(va.buf[k], vb.buf[k]), (t, k)


def _same_stats(ea, eb):
    """Episode tallies: counts and lengths equal; the returns are summed by atomics (any order)."""
    assert ea[2] == eb[2] and ea[1] == eb[1] and abs(ea[0] - eb[0]) <= 1e-9 * max(1.0, abs(ea[0])), (ea, eb)


SPLIT = dict(wide_n=-1, dyn_lpe=1)  # the split step forced at a size that would run the wide kernels
DOORS = {
    "single_default": dict(N=130, slots=5, A=1, sched={}),
    "single_split": dict(N=130, slots=5, A=1, sched=SPLIT),
    "single_lane_tracks": dict(N=130, slots=130, A=1, sched=dict(SPLIT, lane_tracks=1)),
    "two_car": dict(N=64, slots=4, A=2, sched={}),
}


def _pool(N, slots, seed):
    base = _tracks(slots, seed)
    return [base[i % slots] for i in range(N)], [float(6 + (i % slots) % 4) for i in range(N)]


@pytest.mark.parametrize("case", list(DOORS))
def test_same_table_through_both_doors(case):
    """Env B is constructed on a native TrackSet (rx_upload_tracks: the host loop);
    env A on another pool, then swapped onto the same arrays (set_tracks:
    rx_upload_tracks_device, the kernel).  Every consumer of the tables then agrees
    bit for bit for 200 steps."""
    from rx.track import TrackSet
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    c = DOORS[case]
    N, A = c["N"], c["A"]
    pool, widths = _pool(N, c["slots"], 21)
    ts = TrackSet.build(pool, widths, backend="native")
    assert len(ts) == c["slots"]
    kw = dict(n_agents=A, device="cuda", autoreset="next_step", seed=5, sched=c["sched"])
    vb = RacingVectorEnv(pool, widths, track_set=ts, **kw)
    other, other_w = _pool(N, 3, 22)
    va = RacingVectorEnv(other, other_w, **kw)
    va.reset_device()
    obs_a = va.set_tracks(DeviceTrackTable.from_arrays(ts.arrays(), "cuda"), vb.track_of_env)
    assert torch.equal(obs_a, vb.reset_device())
    sa, sb = va.schedule(), vb.schedule()
    assert {k: v for k, v in sa.items() if k != "dyn_calls"} == {k: v for k, v in sb.items() if k != "dyn_calls"}
    assert np.array_equal(va.track_of_env, vb.track_of_env)
    assert sb["lane_tracks"] == (1 if "lane_tracks" in c["sched"] else 0)
    if c["sched"]:
        assert sb["split"] == 1 and sb["wide"] == 0
    assert torch.equal(va.state["track"], vb.state["track"])
    g = torch.Generator(device="cuda").manual_seed(1000 + N)
    for t in range(200):
        _same_step(va, vb, _actions(g, N, A), t)
    ea, eb = va.episode_stats(), vb.episode_stats()
    assert eb[2] > 0, "no episode ended: the run proves little"
    _same_stats(ea, eb)
    va.close()
    vb.close()


@pytest.mark.parametrize("A", [1, 2])
def test_swapped_env_equals_a_fresh_one(A):
    from rx.track import TrackSet
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    N = 96
    p0, w0 = _pool(N, 3, 31)
    p1, w1 = _pool(N, 7, 32)
    ts1 = TrackSet.build(p1, w1, backend="native")
    kw = dict(n_agents=A, device="cuda", autoreset="next_step", seed=9)
    vx = RacingVectorEnv(p0, w0, **kw)
    vx.reset_device()
    g = torch.Generator(device="cuda").manual_seed(77)
    for _ in range(50):
        vx.step_device(_actions(g, N, A))
    in_flight = int((vx.get_state()["ep_length"] > 0).sum())
    assert in_flight > 0
    vx.episode_stats(reset=True)
    vy = RacingVectorEnv(p1, w1, track_set=ts1, **kw)
    obs = vx.set_tracks(DeviceTrackTable.from_arrays(ts1.arrays(), "cuda"), vy.track_of_env)
    assert vx.track_generation == 1 and vy.track_generation == 0
    assert vx.episode_stats(reset=False) == (0.0, 0.0, 0), "a dropped episode was tallied"
    assert torch.equal(obs, vy.reset_device())
    assert len(vx.tracks.geoms) == len(ts1.geoms) == 7
    for a, b in zip(vx.tracks.geoms, ts1.geoms):
        assert np.array_equal(a.waypoints, b.waypoints) and np.array_equal(a.left_boundary, b.left_boundary)
        assert a.track_width == b.track_width and a.max_track_distance == b.max_track_distance
    g = torch.Generator(device="cuda").manual_seed(78)
    for t in range(100):
        _same_step(vx, vy, _actions(g, N, A), t)
    sx, sy = vx.get_state(), vy.get_state()
    for k in sx:
        assert np.array_equal(sx[k], sy[k]), k
    _same_stats(vx.episode_stats(), vy.episode_stats())
    vx.close()
    vy.close()


def test_a_refused_swap_leaves_the_env_on_its_old_tracks():
    from rx import _lib
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    N = 64
    p0, w0 = _pool(N, 4, 41)
    kw = dict(device="cuda", autoreset="next_step", seed=3)
    va, vb = RacingVectorEnv(p0, w0, **kw), RacingVectorEnv(p0, w0, **kw)
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(10):
        _same_step(va, vb, _actions(g, N, 1), t)
    bad = [np.array(c, dtype=np.float64) for c in _tracks(4, 42)]
    bad[2][5] = bad[2][4]  # two coincident consecutive control points: only device memory shows it
    table = DeviceTrackTable.build(bad, [6.0, 7.0, 8.0, 9.0], device="cuda")
    with pytest.raises(_lib.RxError, match=r"track 2\b"):
        va.set_tracks(table)
    assert va.track_generation == 0 and np.array_equal(va.track_of_env, vb.track_of_env)
    for t in range(30):
        _same_step(va, vb, _actions(g, N, 1), t)
    va.close()
    vb.close()


def test_device_table_download_is_build_tables_bytes():
    from rx.track import DEFAULT_CONTROL_POINTS, DEFAULT_WIDTH, build_table
    from rx.track_device import DeviceTrackTable
    pool = _tracks(37, 51) + [None]
    widths = [float(4 + k % 6) for k in range(37)] + [None]
    table = DeviceTrackTable.build(pool, widths, device="cuda")
    got = table.download()
    want = build_table(pool[:-1] + [DEFAULT_CONTROL_POINTS], widths[:-1] + [DEFAULT_WIDTH], 30, "device")
    assert len(table) == 38
    for k in ("wp_off", "wp", "nrm", "seg", "meta"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
    ts = table.track_set()
    assert ts is table.track_set() and ts.backend == "device" and len(ts) == 38
    assert np.array_equal(ts.geoms[3].waypoints, want["wp"][want["wp_off"][3]:want["wp_off"][4]])


# ---------------------------------------------------------------- PPO
def _train(updates=3, **over):
    """train.py:65-115 with rx imports -> (trainer, np.random state after training, the obs buffer of every
    rollout, np.random's state before and after every ppo_update)."""
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.ppo import PPO
    from rx.track import gen_tracks
    config = base_config(num_envs=64, num_steps=16, **over)
    config["total_timesteps"] = updates * config["batch_size"]
    random.seed(config["seed"])
    np.random.seed(config["seed"])
    torch.manual_seed(config["seed"])
    pool = gen_tracks(num_tracks=64, seed=config["seed"])
    widths = [np.random.randint(6, 10) for _ in range(64)]
    t = PPO(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i, track_width=widths[i]), config,
            device="cuda")
    rollouts, marks, collect, update = [], [], t.collect_rollout, t.ppo_update

    def recording(*a):
        out = collect(*a)
        rollouts.append(out[0].clone())
        return out

    def marking(*a):
        marks.append(np.random.get_state())
        update(*a)
        marks.append(np.random.get_state())

    t.collect_rollout, t.ppo_update = recording, marking
    done = [u for u, _, _, _ in t.train_iter()]
    assert done == list(range(updates)) and len(marks) == 2 * updates
    return t, np.random.get_state(), rollouts, marks


@pytest.fixture(scope="module")
def resampled():
    return _train(track_resample_every=1)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_ppo_resamples_tracks_without_moving_np_random(resampled):
    """base_config(num_envs=64, num_steps=16, track_resample_every=1), 3 updates: it
    runs, two swaps happen, everything stays finite, and the swaps do not move
    np.random, which shuffles the minibatches.

    The final np.random state of this run cannot simply be compared with the
    key-0 run's: the KL early stop (agent/ppo.py:178-182) ends an update after a
    data-dependent number of epochs, each epoch is one np.random.shuffle, and after
    the first swap the two runs see different tracks.  Measured on an MI355X: the
    updates stop in epochs 1, 2, 2 with the key 1 and in epochs 1, 2, 3 with the key
    0, so the final states differ (positions 149 against 337 of different key
    blocks) although no swap drew anything.  What holds, and is asserted:
    * in both runs np.random moves inside ppo_update only: its state after update
      u is its state before update u + 1, with the swap and the rollout in between;
    * up to the first swap the runs are one: equal states before and after update 0;
    * with the early stop out of the way (kl_target = 1e9: every update shuffles
      update_epochs times) the final states of the two runs ARE equal."""
    t, state, rollouts, marks = resampled
    assert t.envs.track_generation == 2 and len(t.envs.tracks) == 64
    assert len(rollouts) == 3 and all(torch.isfinite(r).all() for r in rollouts)
    assert not torch.equal(rollouts[0][0], rollouts[1][0]), "the second rollout started on the old tracks"
    for p in t.agent.parameters():  # finite parameters after three updates: every loss and gradient was finite
        assert torch.isfinite(p).all()
    t0, state0, _, marks0 = _train(track_resample_every=0)
    assert t0.envs.track_generation == 0
    for m, end in ((marks, state), (marks0, state0)):
        assert _same_state(m[1], m[2]) and _same_state(m[3], m[4]) and _same_state(m[5], end), \
            "np.random moved between two updates"
    assert _same_state(marks[0], marks0[0]) and _same_state(marks[1], marks0[1])
    assert not _same_state(marks[0], marks[1]), "the update did not shuffle with np.random"
    full = [_train(track_resample_every=k, kl_target=1e9) for k in (1, 0)]
    assert full[0][0].envs.track_generation == 2 and full[1][0].envs.track_generation == 0
    assert _same_state(full[0][1], full[1][1]), "a track swap moved the global numpy stream"


def test_ppo_resampling_graph_rollout_equals_eager(resampled):
    """The swap drops the captured rollout graph (it holds the old table's pointers
    and wave counts): the third update's rollout, two swaps in, equals the eager one."""
    _, _, eager, _ = resampled
    tg, _, graph, _ = _train(track_resample_every=1, graph_rollout=True)
    assert tg.envs.track_generation == 2
    assert torch.equal(graph[2], eager[2])


def test_selfplay_refuses_track_resampling():
    from rx.configs import self_play_config
    from rx.selfplay import SelfPlayPPO
    with pytest.raises(ValueError, match="track_resample_every"):
        SelfPlayPPO(lambda i: None, self_play_config(num_envs=64, num_steps=16, track_resample_every=2), device="cuda")
