"""Slots replaced in place on the GPU: k_patch_slots (rx_patch_tracks, csrc/rx_cull.hip)
against a device full rebuild bit for bit and against its host twin; a live env
whose slots are replaced (RacingVectorEnv.replace_tracks: rx_replace_tracks_device
plus a masked reset) against an untouched twin and against a fresh env on the
updated pool, step for step; a refused replace; and the partial resample of the two
episodic trainers.  Everything compared is a bit pattern, except the circle radius
against the HOST twin (the platform's hypot: tests/test_cull_tables_cpu.py).
"""
import random

import numpy as np
import pytest
import torch

from tests.test_cull_tables_cpu import DTYPES, PARAMS, check_against, decode, np_tables
from tests.test_cull_tables_gpu import DOORS, TABLES, _actions, _tracks
from tests.test_track_replace_cpu import (KEYS, call_patch, cull_build, guarded, patch_struct, table_with_nrm,
                                          updated)

pytestmark = pytest.mark.gpu

_TORCH = {np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
# slots130: the first slot, the last (it owns the offset arrays' final entries), five spread so that the
# second workgroup of 4 wavefronts is mostly empty, and all 130 (the last workgroup half empty)
LISTS = {"slots130": ([0], [129], [3, 40, 64, 77, 128], list(range(130))), "one_w3": ([0],), "one_w2048": ([0],)}
_cache = {}


def _cuda_full(n, value, dtype):
    return torch.full((n,), value, dtype=_TORCH[dtype], device="cuda")


def _table(name):
    if name not in _cache:
        t = TABLES[name]()
        t["nrm"] = np.random.RandomState(7).uniform(-1.0, 1.0, t["wp"].shape)
        _cache[name] = t
    return _cache[name]


def _up(arrays):
    return {k: torch.from_numpy(v).cuda() for k, v in arrays.items()}


@pytest.mark.parametrize("G,SG", PARAMS)
@pytest.mark.parametrize("name", list(LISTS))
def test_kernel_patch_equals_rebuild_and_host_twin(name, G, SG):
    from rx import _lib
    t = _table(name)
    ws = np.diff(t["wp_off"])
    for slots in LISTS[name]:
        what = f"{name} G={G} SG={SG} slots={slots[:5]}"
        src = table_with_nrm([int(ws[k]) for k in slots], 60 + len(slots))
        u = updated(t, slots, src)
        dst = _up(guarded(t))
        bufs = cull_build("rx_build_cull_tables", t, G, SG, arrays=_up({k: t[k] for k in KEYS}),
                          stream=_lib.stream_ptr(), full=_cuda_full)
        src_d = dict(_up({k: src[k] for k in KEYS}), wp_off=src["wp_off"])
        p, keep = patch_struct(slots, src_d)
        rc, msg = call_patch("rx_patch_tracks", t, dst, G, SG, bufs, p, stream=_lib.stream_ptr())
        assert rc == _lib.RX_OK, msg
        want_dst = _up(guarded(u))
        for k in KEYS:
            assert torch.equal(dst[k], want_dst[k]), (what, k)
        want = cull_build("rx_build_cull_tables", u, G, SG, arrays=_up({k: u[k] for k in KEYS}),
                          stream=_lib.stream_ptr(), full=_cuda_full)
        assert set(bufs) == set(want)
        for k in want:  # the device's own full rebuild: bytes, guards included
            assert torch.equal(bufs[k].view(torch.int32 if DTYPES[k] != np.float64 else torch.int64),
                               want[k].view(torch.int32 if DTYPES[k] != np.float64 else torch.int64)), (what, k)
        host = cull_build("rx_build_cull_tables_host", u, G, SG)
        reach = np_tables(u, 8, 0)[1] if G > 0 else None
        got, ref = decode({k: v.cpu().numpy() for k, v in bufs.items()}), decode(host)
        check_against(got, ref, reach, what)
        if G > 0:  # and against the host's own radius
            for k in ("slot_geo", "hdr_f"):
                a, b = got[k].reshape(len(reach), -1)[:, 2], ref[k].reshape(len(reach), -1)[:, 2]
                assert np.all(np.abs(a - b) <= 1e-13 * b), (what, k)


def test_kernel_patch_without_tables_touches_the_four_arrays_only():
    from rx import _lib
    t = _table("slots130")
    ws = np.diff(t["wp_off"])
    slots = [3, 40, 64, 77, 128]
    src = table_with_nrm([int(ws[k]) for k in slots], 71)
    dst = _up(guarded(t))
    src_d = dict(_up({k: src[k] for k in KEYS}), wp_off=src["wp_off"])
    p, keep = patch_struct(slots, src_d)
    rc, msg = call_patch("rx_patch_tracks", t, dst, 0, 0, None, p, stream=_lib.stream_ptr())
    assert rc == _lib.RX_OK, msg
    want = _up(guarded(updated(t, slots, src)))
    for k in KEYS:
        assert torch.equal(dst[k], want[k]), k


# ---------------------------------------------------------------- a live env
def _pool(N, slots, seed):
    base = _tracks(slots, seed)
    return base, [base[i % slots] for i in range(N)], [float(6 + (i % slots) % 4) for i in range(N)]


def _step(v, a):
    o, r, d = v.step_device(a)
    return [o.clone(), r.clone(), d.clone(), v.buf["terminated"].clone(), v.buf["truncated"].clone()]


def _rows_equal(xa, xb, rows, what):
    for i, (a, b) in enumerate(zip(xa, xb)):
        assert torch.equal(a[rows], b[rows]), (what, ("obs", "reward", "done", "terminated", "truncated")[i])


def _replacement(base, S, seed):
    from rx.track_episodic import spawn_same_points
    return spawn_same_points(seed, 1, [len(base[k]) for k in S])


@pytest.mark.parametrize("case", ["single_default", "single_split", "single_lane_tracks"])
def test_replaced_slots_restart_and_the_rest_goes_on(case):
    """A and B: equal envs, 50 equal steps.  A has two occupied slots replaced; C is a
    fresh env put on A's updated table with A's assignment and reset at that moment.
    For 200 more steps the envs off the replaced slots are A == B and the envs on them
    A == C, bit for bit."""
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    c = DOORS[case]
    N, n = c["N"], c["slots"]
    S = [1, 3] if n == 5 else [7, 100]
    base, pool, widths = _pool(N, n, 21)
    kw = dict(device="cuda", autoreset="next_step", seed=5, sched=c["sched"])
    va, vb, vc = (RacingVectorEnv(pool, widths, **kw) for _ in range(3))
    assert len(va.tracks) == n and np.array_equal(va.track_of_env, np.arange(N) % n)
    assert va.schedule()["lane_tracks"] == (1 if "lane_tracks" in c["sched"] else 0)
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device="cuda").manual_seed(1000 + N)
    for t in range(50):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), t)
    on = np.isin(va.track_of_env, S)
    hit = torch.from_numpy(on).cuda()
    before = va.get_state()
    in_flight = int((before["ep_length"][on] > 0).sum())
    assert in_flight > 0, "no env on the replaced slots was in flight: the run proves little"
    stats0, sched0 = va.episode_stats(reset=False), va.schedule()
    cps, ws = _replacement(base, S, 77)
    obs, mask = va.replace_tracks(S, cps, ws)
    assert torch.equal(mask.bool(), hit) and mask.dtype == torch.uint8
    after = va.get_state()
    assert np.all(after["ep_length"][on] == 0) and np.all(after["steps"][on] == 0)
    for k in before:  # nobody else was touched
        assert np.array_equal(before[k][~on], after[k][~on]), k
    assert va.episode_stats(reset=False) == stats0, "a dropped episode was tallied"
    assert va.track_generation == 1 and np.array_equal(va.track_of_env, np.arange(N) % n)
    assert {k: v for k, v in va.schedule().items() if k != "dyn_calls"} == \
        {k: v for k, v in sched0.items() if k != "dyn_calls"}
    table = va._table
    want = DeviceTrackTable.build(cps, ws, device="cuda")
    for j, k in enumerate(S):  # the resident table holds the new tracks' rows
        s0, s1 = int(table.wp_off[k]), int(table.wp_off[k + 1])
        q0, q1 = int(want.wp_off[j]), int(want.wp_off[j + 1])
        assert torch.equal(table.wp[s0:s1], want.wp[q0:q1]) and torch.equal(table.seg[2 * s0:2 * s1],
                                                                             want.seg[2 * q0:2 * q1])
        assert torch.equal(table.meta[k], want.meta[j])
    obs_c = vc.set_tracks(DeviceTrackTable.from_arrays(table.download(), "cuda"), va.track_of_env)
    assert torch.equal(obs[hit], obs_c[hit])
    for t in range(200):
        a = _actions(g, N, 1)
        xa, xb, xc = _step(va, a), _step(vb, a), _step(vc, a)
        _rows_equal(xa, xb, ~hit, (case, "untouched", t))
        _rows_equal(xa, xc, hit, (case, "replaced", t))
    assert va.episode_stats()[2] > 0 and vb.episode_stats()[2] > 0, "no episode ended: the run proves little"
    sa, sc = va.get_state(), vc.get_state()
    for k in sa:
        assert np.array_equal(sa[k][on], sc[k][on]), k
    for v in (va, vb, vc):
        v.close()


def test_two_car_envs_off_the_replaced_slots_go_on():
    from rx.vector_env import RacingVectorEnv
    N, n, S = 64, 4, [1, 2]
    base, pool, widths = _pool(N, n, 23)
    kw = dict(n_agents=2, device="cuda", autoreset="next_step", seed=5)
    va, vb = RacingVectorEnv(pool, widths, **kw), RacingVectorEnv(pool, widths, **kw)
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device="cuda").manual_seed(31)
    for t in range(50):
        a = _actions(g, N, 2)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), t)
    on = np.isin(va.track_of_env, S)
    hit = torch.from_numpy(on).cuda()
    assert int((va.get_state()["ep_length"][on] > 0).sum()) > 0
    cps, ws = _replacement(base, S, 78)
    _, mask = va.replace_tracks(S, cps, ws)
    assert torch.equal(mask.bool(), hit)
    st = va.get_state()
    assert np.all(st["ep_length"][on] == 0) and np.all(st["steps"][on] == 0) and va.track_generation == 1
    for t in range(100):
        a = _actions(g, N, 2)
        _rows_equal(_step(va, a), _step(vb, a), ~hit, ("two_car", t))
    for v in (va, vb):
        v.close()


def test_a_refused_replace_leaves_the_env_as_it_was():
    from rx import _lib
    from rx.vector_env import RacingVectorEnv
    N, n = 64, 4
    base, pool, widths = _pool(N, n, 41)
    kw = dict(device="cuda", autoreset="next_step", seed=3)
    va, vb = RacingVectorEnv(pool, widths, **kw), RacingVectorEnv(pool, widths, **kw)
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(10):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), t)
    cps, ws = _replacement(base, [0, 2], 79)
    with pytest.raises(ValueError, match=r"slot 2\b"):
        va.replace_tracks([0, 2], [cps[0], np.vstack([cps[1], [[1.0, 2.0]]])], ws)
    bad = np.array(cps[1], dtype=np.float64)
    bad[5] = bad[4]  # two coincident consecutive control points: only device memory shows it
    with pytest.raises(_lib.RxError, match=r"slot 2\b"):
        va.replace_tracks([0, 2], [cps[0], bad], ws)
    assert va.track_generation == 0 and va._table is None
    for t in range(20):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), ("after the refusals", t))
    for v in (va, vb):
        v.close()


# ---------------------------------------------------------------- trainers
class _SetTracksCalled(Exception):
    pass


def _trainer(monkeypatch, cls_path, rollout_steps, **over):
    """4,160 envs x 16 steps on a 64-slot pool that holds point counts 10..14, max_steps = 12, every slot
    with an episode counts as mastered: each resample retires floor(0.25 * 64) = 16 slots."""
    import importlib
    from rx import track_episodic
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.track import gen_tracks
    build = track_episodic.build_vector_env
    monkeypatch.setattr(track_episodic, "build_vector_env", lambda *a, **kw: build(*a, **dict(kw, max_steps=12)))
    config = base_config(**dict(dict(num_envs=4160, num_steps=16, kl_target=1e9, update_epochs=1,
                                     track_resample_every=1, curriculum_refresh=0.25, curriculum_mastery=0.0,
                                     curriculum_min_episodes=1, rollout_steps=rollout_steps, track_backend="device"),
                                **over))
    config["total_timesteps"] = 2 * config["batch_size"]
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    rng = np.random.RandomState(21)
    pool = gen_tracks(64, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(64)]
    assert {len(c) for c in pool} == {10, 11, 12, 13, 14}
    mod, name = cls_path.rsplit(".", 1)
    cls = getattr(importlib.import_module(mod), name)
    t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 64, track_width=widths[i % 64]), config,
            device="cuda")
    return t, pool


@pytest.mark.parametrize("rollout_steps", ["auto", "off"])
@pytest.mark.parametrize("cls_path", ["rx.track_episodic.EpisodicCurriculumPPO",
                                      "rx.track_replay_episodic.EpisodicReplayCurriculumPPO"])
def test_partial_resample_replaces_slots_without_a_global_reset(monkeypatch, cls_path, rollout_steps):
    from rx.track_device import DeviceTrackTable
    t, pool = _trainer(monkeypatch, cls_path, rollout_steps, episodic_partial=True)
    monkeypatch.setattr(t.envs, "reassign_tracks", lambda *a: pytest.fail("reassign_tracks was called"))
    monkeypatch.setattr(t.envs, "set_tracks", lambda *a: pytest.fail("set_tracks was called"))
    monkeypatch.setattr(t, "_draw_tracks", lambda *a: pytest.fail("_draw_tracks was called"))
    counts0 = sorted(len(c) for c in t._cps)
    flags, seen_after, collect, resample = [], [], t.collect_rollout, t.resample_tracks

    def recording(*a):
        out = collect(*a)
        flags.append(int((out[3][1:] != 0).sum().item() + (out[7] != 0).sum().item()))
        return out

    def resampling(*a):
        stepping0 = t.envs.get_state()["ep_length"].copy()
        out = resample(*a)
        retired = np.asarray(t.retired[-1], dtype=np.int64)
        on = np.isin(t.envs._st["track"].cpu().numpy(), retired)
        st = t.envs.get_state()
        assert np.all(st["ep_length"][on] == 0) and np.array_equal(st["ep_length"][~on], stepping0[~on])
        assert on.any() and not on.all() and (stepping0[~on] > 0).any(), "no episode went on across the resample"
        assert torch.all(out[1][torch.from_numpy(on).cuda()] == 0)
        assert torch.equal(out[0][torch.from_numpy(on).cuda()], t.envs.buf["obs"][torch.from_numpy(on).cuda()])
        if hasattr(t, "replay"):
            tab = t.track_table()
            seen_after.append((tab["seen"][retired].copy(), tab["score"][retired].copy(),
                               tab["episodes"][retired].copy()))
        return out

    t.collect_rollout, t.resample_tracks = recording, resampling
    graphs_kept = []
    keep = t.resample_tracks
    t.resample_tracks = lambda *a: (graphs_kept.append(dict(getattr(t, "_graphs", {}))), keep(*a),
                                    graphs_kept.append(dict(getattr(t, "_graphs", {}))))[1]
    assert [u for u, _, _, _ in t.train_iter()] == [0, 1]
    assert len(t.retired) == 1 and len(t.retired[0]) == 16 and len(set(t.retired[0])) == 16
    assert graphs_kept[0] == graphs_kept[1], "the captured rollout graphs were dropped"
    assert int(t.curriculum.draws.sum().item()) == sum(flags) and sum(flags) >= 2 * 4160
    assert t.envs.track_generation == 1
    assert sorted(len(c) for c in t._cps) == counts0, "the pool's point-count histogram moved"
    assert sum(not np.array_equal(a, b) for a, b in zip(t._cps, pool)) == 16
    table, want = t.envs._table, DeviceTrackTable.build(t._cps, t._widths, device="cuda")
    assert np.array_equal(table.wp_off, want.wp_off)
    for k in ("wp", "nrm", "seg"):
        assert torch.equal(getattr(table, k), getattr(want, k)), k
    # meta: the replaced rows are the kernel's; the others came through TrackSet, which rewrites the start angle
    # and max_track_distance (columns 2 and 4) by numpy's expressions: the last bit at most (include/rx.h)
    got_m, want_m = table.meta.cpu().numpy(), want.meta.cpu().numpy()
    assert np.array_equal(got_m[t.retired[0]], want_m[t.retired[0]])
    assert np.array_equal(np.delete(got_m, (2, 4), axis=1), np.delete(want_m, (2, 4), axis=1))
    assert np.all(np.abs(got_m[:, (2, 4)] - want_m[:, (2, 4)]) <= np.spacing(np.abs(want_m[:, (2, 4)])))
    if hasattr(t, "replay"):
        (seen, score, episodes), = seen_after
        assert np.all(seen == -1) and np.all(score == 0.0) and np.all(episodes == 0)
    for p in t.agent.parameters():
        assert torch.isfinite(p).all()
    t.envs.close()


def test_partial_resample_keeps_the_captured_rollout_graph(monkeypatch):
    """No address moves, so the graph captured for the first rollout is kept and replayed after
    the slots were replaced.  The first rollout equals the eager run's; the second one, past the
    resample, equals it for its first 10 steps, in which the 1,040 envs on the replaced slots run
    their new tracks from the reset and everyone else goes on.  With max_steps = 12 the envs that
    were not reset end their episode at step 9 of that rollout and restart at step 10 on the slot
    they drew; from there a REPLAYED rollout graph and the eager call draw different slots.  That
    is so without this feature too: measured with ``curriculum_refresh=0`` (nothing retired, the
    parent's path), 4,104 of 4,160 envs differ from step 10 on, and 3,088 with the partial
    resample (the same envs less the 1,040 reset ones, which restart later); a graph captured
    afresh after the resample equals the eager run throughout.  So the comparison stops where the
    first episodic draw after the resample takes effect."""
    runs = {}
    for graph in (False, True):
        t, _ = _trainer(monkeypatch, "rx.track_episodic.EpisodicCurriculumPPO", "auto", episodic_partial=True,
                        graph_rollout=graph)
        rollouts, collect, resample, kept = [], t.collect_rollout, t.resample_tracks, []

        def recording(*a, collect=collect, rollouts=rollouts):
            out = collect(*a)
            rollouts.append([out[i].clone() for i in (0, 1, 3, 4)])
            return out

        def resampling(*a, t=t, resample=resample, kept=kept):
            before = dict(getattr(t, "_graphs", {}))
            out = resample(*a)
            kept.append(bool(before) and before == dict(getattr(t, "_graphs", {})))
            return out

        t.collect_rollout, t.resample_tracks = recording, resampling
        assert [u for u, _, _, _ in t.train_iter()] == [0, 1]
        assert len(t.retired) == 1 and len(t.retired[0]) == 16 and t.envs.track_generation == 1
        runs[graph] = (rollouts, kept)
        t.envs.close()
    assert runs[True][1] == [True], "no captured graph survived the resample"
    for u, steps in ((0, 16), (1, 10)):
        for a, b, name in zip(runs[True][0][u], runs[False][0][u], ("obs", "actions", "dones", "rewards")):
            assert torch.equal(a[:steps], b[:steps]), (u, name)


def test_without_the_key_a_retiring_resample_is_still_the_global_one(monkeypatch):
    t, _ = _trainer(monkeypatch, "rx.track_episodic.EpisodicCurriculumPPO", "auto")
    assert t.partial is False

    def called(*a):
        raise _SetTracksCalled()

    monkeypatch.setattr(t.envs, "set_tracks", called)
    monkeypatch.setattr(t.envs, "replace_tracks", lambda *a: pytest.fail("replace_tracks was called"))
    with pytest.raises(_SetTracksCalled):
        for _ in t.train_iter():
            pass
    t.envs.close()
