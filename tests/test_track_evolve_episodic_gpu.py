"""Track evolution in place on the GPU: the three kernels (csrc/rx_track_evolve.hip) against
their host twins byte for byte; a live env that takes a device spawn
(RacingVectorEnv.replace_tracks_device) against a twin that takes the downloaded children
through replace_tracks; a refused source; and EpisodicEvolvingCurriculumPPO against the host
twins' in-place evolution of its own pool, against EpisodicReplayCurriculumPPO before the first
retiring resample, and against itself.

Every device output buffer carries a guard element past its end.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_track_evolve_cpu import GUARD, SEED, hand_made_pool, pool_case, rank_cdf, spawn_sets
from tests.test_track_evolve_episodic_cpu import (MAX_P, class_cases, host_classes, host_commit, host_inplace,
                                                  inplace_io, one_class_zero, same, staging_offsets)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def dev_classes(L, cp_off, cdf):
    from rx import _lib
    n = len(cp_off) - 1
    order = torch.full((n + 1,), -9, dtype=torch.int32, device="cuda")
    cdf_class = torch.full((n + 1,), -9, dtype=torch.int64, device="cuda")
    class_end = torch.full((MAX_P + 2,), -9, dtype=torch.int32, device="cuda")
    off_d, cdf_d = _dev(cp_off, np.int32), _dev(cdf, np.int64)
    ev = inplace_io(_lib, n, 0, cp_off=off_d, cdf_score=cdf_d, order=order, cdf_class=cdf_class, class_end=class_end)
    _lib.check(L.rx_track_evolve_classes(ctypes.byref(ev), _lib.stream_ptr()), "rx_track_evolve_classes")
    o, c, e = order.cpu().numpy(), cdf_class.cpu().numpy(), class_end.cpu().numpy()
    assert o[n] == -9 and c[n] == -9 and e[MAX_P + 1] == -9
    return o[:n], c[:n], e[:MAX_P + 1]


def dev_inplace_commit(L, slots, cp_off, cp, width, classes, seed, g, edit_frac, out_off=None):
    """The inplace and the commit kernel -> ((plan, out_off, cp_out, width_out), (cp, width) after the commit)."""
    from rx import _lib
    n, ns = len(cp_off) - 1, len(slots)
    out_off = np.ascontiguousarray(staging_offsets(slots, cp_off) if out_off is None else out_off, dtype=np.int32)
    d = dict(slots=_dev(slots, np.int32), cp_off=_dev(cp_off, np.int32),
             cp=_dev(np.concatenate([cp, [[GUARD, GUARD]]]), np.float64), width=_dev(np.concatenate([width, [GUARD]])),
             order=_dev(classes[0]), cdf_class=_dev(classes[1]), class_end=_dev(classes[2]), out_off=_dev(out_off),
             plan=torch.full((ns + 1, 4), -9, dtype=torch.int32, device="cuda"),
             cp_out=torch.full((int(out_off[-1]) + 1, 2), GUARD, dtype=torch.float64, device="cuda"),
             width_out=torch.full((ns + 1,), GUARD, dtype=torch.float64, device="cuda"))
    ev = inplace_io(_lib, n, ns, seed, **d)
    _lib.check(L.rx_track_evolve_inplace(ctypes.byref(ev), g, edit_frac, _lib.stream_ptr()), "rx_track_evolve_inplace")
    plan, cp_out, width_out = d["plan"].cpu().numpy(), d["cp_out"].cpu().numpy(), d["width_out"].cpu().numpy()
    assert (plan[ns] == -9).all() and (cp_out[-1] == GUARD).all() and width_out[ns] == GUARD
    assert d["cp"].cpu().numpy()[:-1].tobytes() == np.ascontiguousarray(cp).tobytes(), "inplace wrote the pool"
    _lib.check(L.rx_track_evolve_commit(ctypes.byref(ev), _lib.stream_ptr()), "rx_track_evolve_commit")
    cp1, w1 = d["cp"].cpu().numpy(), d["width"].cpu().numpy()
    assert (cp1[-1] == GUARD).all() and w1[n] == GUARD
    return (plan[:ns], out_off, cp_out[:-1], width_out[:ns]), (cp1[:-1], w1[:n])


# ---------------------------------------------------------------- 1. the kernels
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2500]  # a lane, the wave's and the 1,024-lane pass's edges, three passes


@pytest.mark.parametrize("n", SIZES)
def test_class_kernel_equals_host_twin(L, n):
    cases = class_cases(L, n)
    if n >= 64:  # point counts of no class among the others, on both sides of a pass's edge
        P = 3 + np.arange(n) % 62
        P[[0, n // 2, n - 1]] = (0, 65, 200)
        off = np.concatenate([[0], np.cumsum(P)]).astype(np.int32)
        cases.append(("no class", off, rank_cdf(L, n)))
    for name, off, cdf in cases:
        want, got = host_classes(L, off, cdf), dev_classes(L, off, cdf)
        for a, b in zip(want, got):
            assert same(a, b), name


def test_class_kernel_on_the_hand_made_pool(L):
    off, _, _, cdf = hand_made_pool()
    for a, b in zip(host_classes(L, off, cdf), dev_classes(L, off, cdf)):
        assert same(a, b)


@pytest.mark.parametrize("n", SIZES)
def test_inplace_and_commit_kernels_equal_host_twins(L, n):
    off, cp, width = pool_case(n, 40 + n)
    cdf = rank_cdf(L, n)
    p0 = int(np.diff(off)[n // 2])
    for name, table in (("ranked", cdf), ("zero", np.zeros(n, dtype=np.int64)),
                        ("one class zero", one_class_zero(off, cdf, p0))):
        classes = host_classes(L, off, table)
        for slots in spawn_sets(n):
            for edit_frac in (0.0, 0.5, 1.0):
                want = host_inplace(L, slots, off, cp, width, classes, SEED, 3, edit_frac)
                got, pool = dev_inplace_commit(L, slots, off, cp, width, classes, SEED, 3, edit_frac)
                for a, b in zip(want, got):
                    assert same(a, b), (name, len(slots), edit_frac)
                for a, b in zip(host_commit(L, slots, off, cp, width, *want[1:]), pool):
                    assert same(a, b), (name, len(slots), edit_frac, "commit")


def test_kernels_mark_a_span_or_a_point_count_that_does_not_fit(L):
    n = 5
    off, cp, width = pool_case(n, 2)
    classes = host_classes(L, off, rank_cdf(L, n))
    slots = np.array([1, 3, 4], dtype=np.int32)
    bad = staging_offsets(slots, off)
    bad[2:] += 1
    want = host_inplace(L, slots, off, cp, width, classes, SEED, 1, 0.5, out_off=bad)
    got, pool = dev_inplace_commit(L, slots, off, cp, width, classes, SEED, 1, 0.5, out_off=bad)
    for a, b in zip(want, got):
        assert same(a, b)
    assert np.isnan(got[3][1]) and (got[2][bad[1]:bad[2]] == GUARD).all()
    for a, b in zip(host_commit(L, slots, off, cp, width, *want[1:]), pool):
        assert same(a, b)
    # P = 0 and P = 65 in the pool
    real = pool_case(3, 5)
    tracks = [real[1][real[0][0]:real[0][1]], np.zeros((0, 2)), 50.0 * np.random.RandomState(3).rand(65, 2),
              real[1][real[0][1]:real[0][2]], np.zeros((0, 2)), real[1][real[0][2]:real[0][3]]]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    cp, width = np.ascontiguousarray(np.concatenate(tracks)), np.array([6.0, 7.0, 8.0, 9.0, 6.0, 7.0])
    cdf = np.cumsum(np.full(6, 1 << 30, dtype=np.int64))
    classes = host_classes(L, off, cdf)
    for a, b in zip(classes, dev_classes(L, off, cdf)):
        assert same(a, b)
    slots = np.arange(6, dtype=np.int32)
    want = host_inplace(L, slots, off, cp, width, classes, SEED, 1, 1.0)
    got, pool = dev_inplace_commit(L, slots, off, cp, width, classes, SEED, 1, 1.0)
    for a, b in zip(want, got):
        assert same(a, b)
    for a, b in zip(host_commit(L, slots, off, cp, width, *want[1:]), pool):
        assert same(a, b)


# ---------------------------------------------------------------- 2. a live env
def _twins():
    from rx.vector_env import RacingVectorEnv
    from tests.test_cull_tables_gpu import DOORS, _actions
    from tests.test_track_replace_gpu import _pool, _rows_equal, _step
    c = DOORS["single_lane_tracks"]
    N, n = c["N"], c["slots"]
    base, pool, widths = _pool(N, n, 21)
    kw = dict(device="cuda", autoreset="next_step", seed=5, sched=c["sched"])
    va, vb = RacingVectorEnv(pool, widths, **kw), RacingVectorEnv(pool, widths, **kw)
    assert len(va.tracks) == n and va.schedule()["lane_tracks"] == 1
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device="cuda").manual_seed(1000 + N)
    for t in range(50):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), t)
    return va, vb, g, N, n


def _spawn(L, va, S, edit_frac=0.5):
    from rx.track_evolve import TrackEvolver
    ev = TrackEvolver(va, SEED, edit_frac)
    ev.classes(_dev(rank_cdf(L, ev.n_tracks), np.int64))
    return ev, ev.spawn_in_place(S, 1)


def test_device_replacement_equals_the_host_path():
    """A takes the spawn from device memory, B the same children downloaded, through replace_tracks."""
    from rx import _lib
    from tests.test_cull_tables_gpu import _actions
    from tests.test_track_replace_gpu import _rows_equal, _step
    va, vb, g, N, n = _twins()
    S = [7, 30, 31, 64, 100, 129]
    ev, p = _spawn(_lib.load(), va, S)
    assert p.slots.tolist() == S and np.array_equal(np.diff(p.out_off), np.diff(ev.cp_off_host)[S])
    pool0 = ev.control_points()
    on = np.isin(va.track_of_env, S)
    hit = torch.from_numpy(on).cuda()
    before = va.get_state()
    assert int((before["ep_length"][on] > 0).sum()) > 0
    obs_a, mask_a = va.replace_tracks_device(p.slots, p.out_off, p.cp_out, p.width_out)
    assert va._table.control_points is None, "the source's control points were not downloaded for the bookkeeping"
    ev.commit(p)
    va._table.point_at(ev.cp_off_host, ev.cp, ev.width)
    plan = p.plan.cpu().numpy()
    assert set(plan[:, 0].tolist()) == {0, 1}, "pick another seed: the spawn holds one kind only"
    cp_out, w_out = p.cp_out.cpu().numpy(), p.width_out.cpu().numpy()
    cps = [cp_out[p.out_off[j]:p.out_off[j + 1]] for j in range(len(S))]
    obs_b, mask_b = vb.replace_tracks(S, cps, list(w_out))
    assert torch.equal(obs_a, obs_b) and torch.equal(mask_a, mask_b) and torch.equal(mask_a.bool(), hit)
    assert va.track_generation == vb.track_generation == 1
    assert np.array_equal(va._table.wp_off, vb._table.wp_off)
    for k in ("wp", "nrm", "seg", "meta"):
        assert torch.equal(getattr(va._table, k), getattr(vb._table, k)), k
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
        assert np.array_equal(before[k][~on], sa[k][~on]), (k, "an env off the slots was touched")
    assert np.all(sa["ep_length"][on] == 0)
    # the pool: the children in their slots, every other slot as it was; the table reads it when asked
    pool1 = ev.control_points()
    for k in range(n):
        want = cps[S.index(k)] if k in S else pool0[0][k]
        assert pool1[0][k].tobytes() == want.tobytes(), k
        assert pool1[1][k] == (w_out[S.index(k)] if k in S else pool0[1][k])
        assert va._table.control_points[k].tobytes() == pool1[0][k].tobytes()
    for t in range(30):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), ("after", t))
    for v in (va, vb):
        v.close()


def test_a_refused_source_leaves_env_table_and_pool_as_they_were():
    from rx import _lib
    from tests.test_cull_tables_gpu import _actions
    from tests.test_track_replace_gpu import _rows_equal, _step
    va, vb, g, N, n = _twins()
    S = [7, 100]
    ev, p = _spawn(_lib.load(), va, S)
    cp0, w0 = ev.cp.clone(), ev.width.clone()
    with pytest.raises(ValueError, match=r"slot 100\b"):
        va.replace_tracks_device(p.slots, p.out_off + np.array([0, 0, 1], dtype=np.int32), p.cp_out, p.width_out)
    p.width_out[1] = float("nan")  # what rx_track_evolve_inplace leaves for a slot it could not write
    with pytest.raises(_lib.RxError, match=r"slot 100\b"):
        va.replace_tracks_device(p.slots, p.out_off, p.cp_out, p.width_out)
    assert va.track_generation == 0 and va._table is None
    assert torch.equal(ev.cp, cp0) and torch.equal(ev.width, w0)
    for t in range(20):
        a = _actions(g, N, 1)
        _rows_equal(_step(va, a), _step(vb, a), slice(None), ("after the refusals", t))
    for v in (va, vb):
        v.close()


# ---------------------------------------------------------------- 3. the trainer
CLS = "rx.track_evolve_episodic.EpisodicEvolvingCurriculumPPO"


def _evolving(monkeypatch, rollout_steps, updates=3, cls_path=CLS, **over):
    from rx import track_episodic
    from tests.test_track_replace_gpu import _trainer
    t, pool = _trainer(monkeypatch, cls_path, rollout_steps, **over)
    t.config["total_timesteps"] = updates * t.config["batch_size"]
    monkeypatch.setattr(t.envs, "reassign_tracks", lambda *a: pytest.fail("reassign_tracks was called"))
    monkeypatch.setattr(t.envs, "set_tracks", lambda *a: pytest.fail("set_tracks was called"))
    monkeypatch.setattr(t, "_draw_tracks", lambda *a: pytest.fail("_draw_tracks was called"))
    if cls_path == CLS:
        monkeypatch.setattr(track_episodic, "spawn_same_points", lambda *a: pytest.fail("spawn_same_points was called"))
        monkeypatch.setattr(t.envs, "replace_tracks",
                            lambda *a: pytest.fail("replace_tracks (the host path) was called"))
    return t, pool


def _params(t):
    return [p.detach().clone() for p in t.agent.parameters()]


@pytest.mark.parametrize("rollout_steps", ["auto", "off"])
def test_trainer_evolves_retired_slots_in_place(L, monkeypatch, rollout_steps):
    from rx.track_device import DeviceTrackTable
    graph = rollout_steps == "auto"  # the one-call rollout captured as a graph: it must survive the resamples
    t, pool = _evolving(monkeypatch, rollout_steps, evolve_edit=0.5, graph_rollout=graph)
    ev = t.evolver
    off = ev.cp_off_host.copy()
    assert t.partial is True and t._cps is None and sorted(np.diff(off)) == sorted(len(c) for c in pool)
    cp_addr = (ev.cp.data_ptr(), ev.width.data_ptr())
    seen, checks, spawn, resample = [], [], ev.spawn_in_place, t.resample_tracks

    def spawning(slots, generation, stream=None):  # what the spawn reads, as it stands at that moment
        seen.append(dict(cdf=t.replay.cdf_score.cpu().numpy(), classes=[c.cpu().numpy() for c in ev._classes],
                         cp=ev.cp.cpu().numpy(), width=ev.width.cpu().numpy(), slots=np.asarray(slots), g=generation))
        return spawn(slots, generation, stream)

    def resampling(*a):
        graphs = dict(getattr(t, "_graphs", {}))
        stepping0 = t.envs.get_state()["ep_length"].copy()
        out = resample(*a)
        assert graphs == dict(getattr(t, "_graphs", {})), "the captured rollout graphs were dropped"
        checks.append(bool(graphs))
        retired = np.asarray(t.retired[-1], dtype=np.int64)
        on = np.isin(t.envs._st["track"].cpu().numpy(), retired)
        st = t.envs.get_state()
        assert np.all(st["ep_length"][on] == 0) and np.array_equal(st["ep_length"][~on], stepping0[~on])
        assert on.any() and not on.all() and (stepping0[~on] > 0).any(), "no episode went on across the resample"
        tab = t.track_table()
        assert np.all(tab["seen"][retired] == -1) and np.all(tab["score"][retired] == 0.0)
        assert np.all(tab["episodes"][retired] == 0)
        # the pool against the host twins' in-place evolution of the pool before
        s = seen[-1]
        g, plan = t.plans[-1][0], t.plans[-1][2]
        assert np.array_equal(s["slots"], retired) and s["g"] == g == t.envs.track_generation
        assert np.array_equal(t.plans[-1][1], retired)
        classes = host_classes(L, off, s["cdf"])
        for a, b in zip(classes, s["classes"]):
            assert same(a, b), "the class table"
        want = host_inplace(L, retired, off, s["cp"], s["width"], classes, ev.seed, g, 0.5)
        assert same(want[0], plan)
        cp1, w1 = host_commit(L, retired, off, s["cp"], s["width"], *want[1:])
        assert ev.cp.cpu().numpy().tobytes() == cp1.tobytes() and ev.width.cpu().numpy().tobytes() == w1.tobytes()
        assert (ev.cp.data_ptr(), ev.width.data_ptr()) == cp_addr and np.array_equal(ev.cp_off_host, off)
        # the env's table against a build of the downloaded pool
        cps, ws = t.control_points()
        table, ref = t.envs._table, DeviceTrackTable.build(cps, list(ws), device="cuda")
        assert np.array_equal(table.wp_off, ref.wp_off)
        for k in ("wp", "nrm", "seg"):
            assert torch.equal(getattr(table, k), getattr(ref, k)), k
        assert torch.equal(table.meta[torch.from_numpy(retired).cuda()], ref.meta[torch.from_numpy(retired).cuda()])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(table.control_points, cps))
        # the lineage follows the plans
        lin = {k: np.full(64, -1 if k in ("parent", "kind") else 0, dtype=np.int32) for k in t.lineage}
        for gg, slots, pl in t.plans:
            lin["kind"][slots], lin["parent"][slots], lin["edits"][slots], lin["born"][slots] = \
                pl[:, 0], pl[:, 1], pl[:, 3], gg
        for k in lin:
            assert np.array_equal(tab[k], lin[k]), k
        assert np.array_equal(np.diff(off)[plan[plan[:, 0] == 1, 1]], plan[plan[:, 0] == 1, 2])
        return out

    ev.spawn_in_place, t.resample_tracks = spawning, resampling
    assert [u for u, _, _, _ in t.train_iter()] == [0, 1, 2]
    assert len(t.retired) == 2 and len(t.retired[0]) == 16 and len(t.retired[1]) >= 1 and len(seen) == 2
    assert t.envs.track_generation == 2 and len(t.plans) == 2
    kinds = np.concatenate([pl[:, 0] for _, _, pl in t.plans])
    assert (kinds == 1).any() and (kinds == 0).any(), "pick another seed: the plans hold one kind only"
    assert checks == [graph, graph], "no captured graph was there to be kept"
    for p in t.agent.parameters():
        assert torch.isfinite(p).all()
    t.envs.close()


@pytest.mark.parametrize("rollout_steps", ["auto", "off"])
def test_trainer_equals_the_replay_trainer_before_the_first_resample_and_itself(monkeypatch, rollout_steps):
    runs = []
    for _ in range(2):
        t, _ = _evolving(monkeypatch, rollout_steps, updates=2, evolve_edit=0.5)
        after = []
        for u, _, _, _ in t.train_iter():
            after.append(_params(t))
        cps, ws = t.control_points()
        runs.append((after, cps, ws, [pl for _, _, pl in t.plans], t.retired))
        t.envs.close()
    (a, cps_a, ws_a, plans_a, ret_a), (b, cps_b, ws_b, plans_b, ret_b) = runs
    assert len(a) == 2 and ret_a == ret_b and len(ret_a[0]) == 16
    for u in range(2):
        assert all(torch.equal(x, y) for x, y in zip(a[u], b[u])), u
    assert all(x.tobytes() == y.tobytes() for x, y in zip(cps_a, cps_b)) and ws_a.tobytes() == ws_b.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(plans_a, plans_b))
    r, _ = _evolving(monkeypatch, rollout_steps, updates=1,
                     cls_path="rx.track_replay_episodic.EpisodicReplayCurriculumPPO", episodic_partial=True)
    assert [u for u, _, _, _ in r.train_iter()] == [0]
    assert all(torch.equal(x, y) for x, y in zip(a[0], _params(r))), "before the first retiring resample"
    r.envs.close()
