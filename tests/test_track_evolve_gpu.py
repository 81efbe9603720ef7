"""Track evolution on the GPU: the two kernels (csrc/rx_track_evolve.hip) against
their host twins byte for byte, DeviceTrackTable.build_from_device against build, and
EvolvingCurriculumPPO against the host twins' evolution of its own pool, against
ReplayCurriculumPPO before the first resample, and against itself.

Every device output buffer carries a guard element past its end.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.test_track_evolve_cpu import (GUARD, SEED, build_host, evolve_io, hand_made_pool, host_evolve, pool_case,
                                         rank_cdf, spawn_sets)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_evolve(L, slots, cp_off, cp, width, cdf, seed, g, edit_frac):
    """host_evolve with the two kernels -> (plan after the plan kernel, plan, cp_off_new, cp_new, width_new)."""
    from rx import _lib
    n, ns = len(width), len(slots)
    d = {k: _dev(v) for k, v in dict(slots=np.asarray(slots, dtype=np.int32), cp_off=np.asarray(cp_off, dtype=np.int32),
                                     cp=cp, width=width, cdf_score=np.asarray(cdf, dtype=np.int64)).items()}
    plan = torch.full((ns + 1, 4), -9, dtype=torch.int32, device="cuda")
    ev = evolve_io(_lib, n, ns, seed, slots=d["slots"], cp_off=d["cp_off"], cdf_score=d["cdf_score"], plan=plan)
    _lib.check(L.rx_track_evolve_plan(ctypes.byref(ev), g, edit_frac, _lib.stream_ptr()), "rx_track_evolve_plan")
    plan0 = plan.cpu().numpy()
    assert (plan0[ns] == -9).all()
    points = np.diff(np.asarray(cp_off, dtype=np.int32))
    points[slots] = plan0[:ns, 2]
    off_new = np.concatenate([[0], np.cumsum(points)]).astype(np.int32)
    cp_new = torch.full((int(off_new[-1]) + 1, 2), GUARD, dtype=torch.float64, device="cuda")
    width_new = torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda")
    ev = evolve_io(_lib, n, ns, seed, slots=d["slots"], cp_off=d["cp_off"], cp=d["cp"], width=d["width"], plan=plan,
                   cp_off_new=_dev(off_new), cp_new=cp_new, width_new=width_new)
    _lib.check(L.rx_track_evolve(ctypes.byref(ev), g, _lib.stream_ptr()), "rx_track_evolve")
    plan1, cp1, w1 = plan.cpu().numpy(), cp_new.cpu().numpy(), width_new.cpu().numpy()
    assert (plan1[ns] == -9).all() and (cp1[-1] == GUARD).all() and w1[n] == GUARD
    return plan0[:ns], plan1[:ns], off_new, cp1[:-1], w1[:n]


# ---------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_kernels_equal_host_twins(L, n):
    """One lane, a partial wave, an exact wave, a wave plus a lane, sixteen waves less 24 lanes; nothing,
    one slot, a scattered quarter and every slot spawned; all fresh, mixed and all edits; a zero rank table."""
    off, cp, width = pool_case(n, 40 + n)
    for cdf in (rank_cdf(L, n), np.zeros(n, dtype=np.int64)):
        for slots in spawn_sets(n):
            for edit_frac in (0.0, 0.5, 1.0):
                want = host_evolve(L, slots, off, cp, width, cdf, SEED, 3, edit_frac)
                plan0, *got = dev_evolve(L, slots, off, cp, width, cdf, SEED, 3, edit_frac)
                assert np.array_equal(plan0[:, :3], want[0][:, :3]) and not plan0[:, 3].any(), "the plan kernel"
                for a, b in zip(want, got):
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (len(slots),
                                                                                                      edit_frac)


def test_kernels_equal_host_twins_on_hand_made_parents_and_chained(L):
    off, cp, width, cdf = hand_made_pool()
    slots = np.arange(5, dtype=np.int32)
    host = dev = (off, cp, width)
    for g in (1, 2, 3):
        want = host_evolve(L, slots, *host, cdf, SEED, g, 1.0)
        _, *got = dev_evolve(L, slots, *dev, cdf, SEED, g, 1.0)
        for a, b in zip(want, got):
            assert a.tobytes() == b.tobytes(), g
        assert set(got[0][:, 2].tolist()) <= {3, 64}
        host, dev = want[1:], tuple(got[1:])


# ---------------------------------------------------------------- 2. build_from_device
@pytest.mark.parametrize("n", [1, 65])
def test_build_from_device_equals_build(L, n):
    from rx.track_device import KEYS, DeviceTrackTable
    off, cp, width = pool_case(n, 3)
    _, plan, off1, cp1, w1 = dev_evolve(L, spawn_sets(n)[-1], off, cp, width, rank_cdf(L, n), SEED, 1, 0.5)
    cp_d, w_d = _dev(cp1), _dev(w1)
    table = DeviceTrackTable.build_from_device(off1, cp_d, w_d)
    assert table._control_points is None and table._cp_dev is not None, "nothing comes down until someone asks"
    cps = [cp1[off1[k]:off1[k + 1]] for k in range(n)]
    ref = DeviceTrackTable.build(cps, list(w1), device="cuda")
    a, b = table.download(), ref.download()
    assert np.array_equal(a["wp_off"], b["wp_off"]) and len(table) == n
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    host = build_host(L, off1, cp1, w1)
    assert np.array_equal(a["wp_off"], host[0]) and np.isfinite(a["meta"]).all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(table.control_points, cps))
    assert table.widths == [float(w) for w in w1] and table._cp_dev is None
    assert len(table.track_set().geoms) == n
    with pytest.raises(ValueError, match="build_from_device"):
        DeviceTrackTable.build_from_device(off1, cp_d.float(), w_d)


# ---------------------------------------------------------------- 3. EvolvingCurriculumPPO
def _pool(n_tracks, seed):
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    return gen_tracks(n_tracks, seed=None, rng=rng), [int(rng.randint(6, 10)) for _ in range(n_tracks)]


def _train(evolve, updates=6):
    """256 envs x 32 steps on a pool of 16 tracks, max_steps = 12, a resample every 2 updates that retires
    floor(0.25 * 16) = 4 slots -> (trainer, the parameters after every update, what every spawn saw and
    left, what every resample left)."""
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.ppo import build_vector_env
    from rx.track_evolve import EvolvingCurriculumPPO
    from rx.track_replay import ReplayCurriculumPPO

    class ShortEpisodes(EvolvingCurriculumPPO if evolve else ReplayCurriculumPPO):
        def _make_envs(self, env_fn):
            c = self.config
            return build_vector_env(env_fn, c["num_envs"], c["seed"], self.device, max_steps=12)

    config = base_config(num_envs=256, num_steps=32, kl_target=1e9, track_resample_every=2, curriculum_mastery=0.0,
                         curriculum_min_episodes=0)
    config["total_timesteps"] = updates * config["batch_size"]
    random.seed(config["seed"])
    np.random.seed(config["seed"])
    torch.manual_seed(config["seed"])
    pool, widths = _pool(16, 21)
    t = ShortEpisodes(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 16,
                                          track_width=widths[i % 16]), config, device="cuda")
    spawns, swaps, params = [], [], []
    resample = t.resample_tracks
    if evolve:
        ev, spawn = t.evolver, t.evolver.spawn

        def spawning(slots, generation, cdf_score, stream=None):
            before = (ev.cp_off_host.copy(), ev.cp.cpu().numpy(), ev.width.cpu().numpy(), ev.table().download())
            table, plan = spawn(slots, generation, cdf_score, stream)
            spawns.append(dict(slots=np.asarray(slots).copy(), generation=generation, cdf=cdf_score.cpu().numpy(),
                               before=before, plan=plan.copy(), table=table.download(),
                               after=(ev.cp_off_host.copy(), ev.cp.cpu().numpy(), ev.width.cpu().numpy())))
            return table, plan
        ev.spawn = spawning

    def swapping(*a):
        out = resample(*a)
        swaps.append(dict(generation=t.envs.track_generation, retired=list(t.retired[-1]),
                          rank=t.replay.rank.cpu().numpy(), seen=t.replay.seen.cpu().numpy(),
                          bound=t.envs._st["track"].cpu().numpy(), table=t.track_table() if evolve else None))
        return out

    t.resample_tracks = swapping
    for u, _, _, _ in t.train_iter():
        params.append([p.detach().clone() for p in t.agent.parameters()])
    assert len(params) == updates
    return t, params, spawns, swaps


@pytest.fixture(scope="module")
def trained():
    return _train(True)


def test_trainer_pool_is_the_host_twins_evolution_of_the_pool_before(L, trained):
    t, _, spawns, swaps = trained
    assert len(spawns) == len(swaps) == 2 and t.envs.track_generation == 2
    for sp, sw in zip(spawns, swaps):
        slots, g = sp["slots"], sp["generation"]
        assert len(slots) == 4 and sorted(sw["retired"]) == slots.tolist() and g == sw["generation"]
        off0, cp0, w0, table0 = sp["before"]
        want = host_evolve(L, slots, off0, cp0, w0, sp["cdf"], t.config["seed"], g, 0.5)
        assert want[0].tobytes() == sp["plan"].tobytes(), "the downloaded plan"
        for a, b in zip(want[1:], sp["after"]):
            assert a.tobytes() == np.ascontiguousarray(b).tobytes()
        assert sp["cdf"][-1] > 0, "the rank table the parents were drawn from"
        # the table rows of the kept slots are the ones they had
        a, b = table0, sp["table"]
        for k in np.setdiff1d(np.arange(16), slots):
            for key, per in (("wp", 1), ("nrm", 1), ("seg", 2)):
                ra = a[key][per * a["wp_off"][k]:per * a["wp_off"][k + 1]]
                rb = b[key][per * b["wp_off"][k]:per * b["wp_off"][k + 1]]
                assert ra.tobytes() == rb.tobytes(), (k, key)
            assert a["meta"][k].tobytes() == b["meta"][k].tobytes(), k
        assert np.isfinite(b["meta"]).all()
    cps, widths = t.control_points()
    off, cp, w = spawns[-1]["after"]
    assert all(c.tobytes() == cp[off[k]:off[k + 1]].tobytes() for k, c in enumerate(cps)) and np.array_equal(widths, w)
    assert all(c.tobytes() == d.tobytes() for c, d in zip(t.envs._table.control_points, cps))


def test_trainer_track_table_carries_the_lineage(trained):
    t, _, spawns, swaps = trained
    kind, parent = np.full(16, -1), np.full(16, -1)
    edits, born = np.zeros(16, dtype=int), np.zeros(16, dtype=int)
    for sp, sw in zip(spawns, swaps):
        s, plan = sp["slots"], sp["plan"]
        kind[s], parent[s], edits[s], born[s] = plan[:, 0], plan[:, 1], plan[:, 3], sp["generation"]
        tab = sw["table"]
        for key, want in (("kind", kind), ("parent", parent), ("edits", edits), ("born", born)):
            assert np.array_equal(tab[key], want), key
        assert "score" in tab and "episodes" in tab and "rank" in tab
    assert (kind >= 0).sum() >= 4 and set(kind.tolist()) <= {-1, 0, 1}


def test_every_retired_slot_ranks_first_in_the_following_draw(trained):
    _, _, _, swaps = trained
    for sw in swaps:
        assert sorted(sw["rank"][sw["retired"]].tolist()) == [1, 2, 3, 4]
        assert (sw["seen"][sw["retired"]] == -1).all()
        assert sw["bound"].min() >= 0 and sw["bound"].max() < 16


def test_trainer_equals_replay_curriculum_ppo_until_the_first_resample(trained):
    t, params, _, _ = trained
    tr, params_r, _, swaps_r = _train(False)  # the same number of updates: the learning rate anneals over them
    assert tr.envs.track_generation == 2
    for u in (0, 1):
        for a, b in zip(params[u], params_r[u]):
            assert torch.equal(a, b), u
    assert t.retired[0] == tr.retired[0], "retirement still comes from the finish tallies"


def test_trainer_is_deterministic(trained):
    t, params, spawns, swaps = trained
    t2, params2, spawns2, swaps2 = _train(True)
    for a, b in zip(params[-1], params2[-1]):
        assert torch.equal(a, b)
    for a, b in zip(spawns, spawns2):
        assert a["plan"].tobytes() == b["plan"].tobytes() and a["after"][1].tobytes() == b["after"][1].tobytes()
    for a, b in zip(swaps, swaps2):
        assert np.array_equal(a["bound"], b["bound"])
    assert torch.equal(t.evolver.cp, t2.evolver.cp) and torch.equal(t.replay.score, t2.replay.score)
