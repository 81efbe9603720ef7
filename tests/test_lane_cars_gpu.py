"""Lane-varying track slots for two-car envs (rx_set_lane_cars, additive to ABI v25; DESIGN.md
§3 "Lane-varying two-car envs").

On a pool of many distinct tracks the slot-grouped schedule leaves k_kin2 / k_step2<2> one or
two live lanes per dynamics wave; with the option on, the two-car kernels take 64 consecutive
positions of any slots and every lane reads its own slot's tables.  The culling is exact either
way, so the lane-varying kernels (k_dyn2<KIN, true>, k_step2<2, 1, 1, true>, k_dyn2<FULL, true>,
k_rays<2, true>) must give the grouped kernels' outputs BIT FOR BIT -- observations, f32 and f64
rewards, masks, info rows with the placement, the f64 state, flags, finished_step and the
episode counters -- and the oracle's, and the CPU lap-event trace's; every step loop, pool change
and a training run must come out the same on either schedule.  Sizes are the smallest at which
the schedule can go wrong: 130 envs = 3 blocks, the last of 2 envs, the REWARD workgroups padded
to 8; 1,100 envs = 18 blocks (more than XCDs), the last ragged.  No tolerance anywhere but the
sum of the episode returns (1e-9 relative, tests/test_lane_tracks_gpu.py's bound: the shards add
other env sets).
"""
import random

import numpy as np
import pytest
import torch

from oracle.orc import TrackTable, multi_state, sensor_angles
from tests import lap_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL2 = sensor_angles(11, np.pi / 2)
STATE = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering", "steps", "flags", "env_flags",
         "finished_step", "ep_return", "ep_length")
OUT = ("terminated", "truncated", "info", "reward64")


def _pool(n, kind, seed=1):
    from rx.track import gen_tracks
    random.seed(seed)
    np.random.seed(seed)
    if kind == "seed1":  # train.py:67-80: 7 slots
        pool = gen_tracks(num_tracks=n, seed=1)
    elif kind == "distinct":
        pool = gen_tracks(num_tracks=n, seed=None)
    else:  # mixed: every 4th env its own track, the rest on the seed-1 pool's slots
        a = gen_tracks(num_tracks=n, seed=1)
        b = gen_tracks(num_tracks=n // 4 + 1, seed=None)
        pool = [b[i // 4] if i % 4 == 0 else a[i] for i in range(n)]
    widths = [np.random.randint(6, 10) for _ in range(n)]
    return pool, widths


def _pair(n, kind, modes=(-1, 1), **kw):
    """Two-car envs on one TrackSet with one seed (the same device start-side draws), one per lane_cars mode."""
    from rx.track import TrackSet
    from rx.vector_env import RacingVectorEnv
    pool, widths = _pool(n, kind)
    ts = TrackSet.build(pool, widths)
    kw = dict(dict(n_agents=2, device=DEV, autoreset="next_step", seed=9), **kw)
    return [RacingVectorEnv(pool, widths, track_set=ts, lane_cars=m, **kw) for m in modes]


def _actions(g, n):
    return torch.rand((n, 2, 2), device=DEV, generator=g) * 2 - 1  # U(-1, 1)^2 per car


def _same_state(va, vb, at):
    sa, sb = va.get_state(), vb.get_state()
    for k in STATE:
        assert np.array_equal(sa[k], sb[k]), (at, k)


def _same_steps(va, vb, steps, g, state_every=50):
    """Obs, f32 reward, done and the full_info rows every step, the state every state_every steps; the dones."""
    n, ended = va.num_envs, 0
    for t in range(steps):
        a = _actions(g, n)
        oa, ra, da = va.step_device(a, full_info=True)
        ob, rb, db = vb.step_device(a, full_info=True)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        for k in OUT:
            assert torch.equal(va.buf[k], vb.buf[k]), (t, k)
        ended += int((da != 0).sum())
        if (t + 1) % state_every == 0:
            _same_state(va, vb, t)
    return ended


def _run(va, vb, steps, seed):
    n = va.num_envs
    assert va.schedule()["lane_tracks"] == 0 and vb.schedule()["lane_tracks"] == 1
    assert torch.equal(va.reset_device(), vb.reset_device())
    ended = _same_steps(va, vb, steps, torch.Generator(device=DEV).manual_seed(seed))
    ea, eb = va.episode_stats(), vb.episode_stats()
    assert ea[2] == eb[2] == ended and ea[1] == eb[1] and abs(ea[0] - eb[0]) <= 1e-9 * max(1.0, abs(ea[0])), (ea, eb)
    # the raycast on its own (k_rays<2, true>, rx_step_phases) and an explicit reset of some envs
    z = torch.zeros((n, 2, 2), device=DEV)
    assert torch.equal(va.step_device(z, phases=2)[0], vb.step_device(z, phases=2)[0])
    m = (torch.arange(n, device=DEV) % 3 == 0)
    assert torch.equal(va.reset_device(mask=m), vb.reset_device(mask=m))
    _same_state(va, vb, "reset")
    return ended


# ---- 1. the split step against the grouped schedule -------------------------------------------------
@pytest.mark.parametrize("N,kind", [(130, "distinct"), (130, "seed1"), (1100, "mixed")])
def test_equals_the_grouped_schedule_split_step(N, kind):
    """k_dyn2<KIN, true> + k_step2<2, 1, 1, true> against k_kin2 + k_step2<2> over 200 steps.  The CPU
    oracle with these action ranges ends 183 (distinct), 188 (seed-1) and 188 (mixed) episodes in
    200 steps at N = 130; the device's start-side draws differ, hence at least 90."""
    va, vb = _pair(N, kind)
    sa, sb = va.schedule(), vb.schedule()
    assert sa["split"] == sb["split"] == 1 and sb["dyn_waves"] == (N + 63) // 64
    ended = _run(va, vb, 200, seed=N)
    print(f"\nN={N} {kind}: {ended} episodes ended; grouped dyn waves {sa['dyn_waves']}, lane-varying {sb['dyn_waves']}")
    assert ended >= (90 if N == 130 else 1)
    va.close()
    vb.close()


# ---- 2. the one-kernel paths ------------------------------------------------------------------------
def test_equals_the_grouped_schedule_same_step_autoreset():
    """k_dyn2<FULL, true> + k_rays<2, true>: same-step autoreset needs done before the observation."""
    va, vb = _pair(130, "distinct", autoreset="same_step")
    assert _run(va, vb, 150, seed=7) > 0
    va.close()
    vb.close()


def test_equals_the_grouped_schedule_without_the_split():
    va, vb = _pair(130, "distinct", sched=dict(split=-1))
    assert va.schedule()["split"] == vb.schedule()["split"] == 0
    assert _run(va, vb, 150, seed=8) > 0
    va.close()
    vb.close()


# ---- 3. against the oracle --------------------------------------------------------------------------
def _oracle_table(v):
    t = TrackTable.__new__(TrackTable)
    a = v.tracks.arrays()
    t.wp_off, t.wp, t.nrm, t.seg, t.meta = a["wp_off"], a["wp"], a["nrm"], a["seg"], a["meta"]
    t.n = len(a["meta"])
    return t


def test_bit_exact_vs_oracle(oracle_dev):
    """tests/test_fullsize_gpu.py::test_two_car_subset_bit_exact_vs_oracle's loop over every env of 130
    on the distinct pool: the oracle is reset with whichever of the two start orders the device chose."""
    N = 130
    v, = _pair(N, "distinct", modes=(1,))
    assert v.schedule()["lane_tracks"] == 1
    tab = _oracle_table(v)
    idx = np.arange(N)
    st = multi_state(N)
    st["track"][:] = v.track_of_env[idx]

    def oracle_reset(mask):
        dx = v.get_state()["x"].reshape(N, 2)[idx]
        keep = {k: val.copy() for k, val in st.items()}
        outs = []
        for first in (0, 1):
            for k in st:
                st[k][...] = keep[k]
            o = oracle_dev.multi_reset(tab, st, first, REL2, mask=mask)
            outs.append((o, {k: val.copy() for k, val in st.items()}))
        pick = np.where(np.all(outs[0][1]["x"] == dx, axis=1), 0, 1)
        ok = np.all(outs[1][1]["x"] == dx, axis=1) | (pick == 0)
        assert ok[mask].all(), "device start slots are neither oracle order"
        obs = np.where(pick[:, None, None] == 0, outs[0][0], outs[1][0])
        for k in st:
            val0, val1 = outs[0][1][k], outs[1][1][k]
            sel = pick.reshape((-1,) + (1,) * (val0.ndim - 1)) == 0
            st[k][...] = np.where(sel, val0, val1)
        return obs

    obs = v.reset_device().cpu().numpy()
    assert np.array_equal(obs[idx], oracle_reset(np.ones(N, bool)))
    rng = np.random.default_rng(13)
    pending = np.zeros(N, bool)
    ended = 0
    for t in range(200):
        a = rng.uniform(-1, 1, (N, 2, 2)).astype(np.float32)
        obs, rew, done = v.step_device(torch.from_numpy(a).cuda())
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        o_obs, o_rew, _, o_done_all, _, _, _ = oracle_dev.multi_step(tab, st, a[idx], REL2)
        if pending.any():
            r_obs = oracle_reset(pending)
            o_obs[pending] = r_obs[pending]
            o_rew[pending] = 0.0
            o_done_all[pending] = False
        assert np.array_equal(obs[idx], o_obs), t
        assert np.array_equal(rew[idx], o_rew.astype(np.float32)), t
        assert np.array_equal(done[idx], o_done_all), t
        pending = o_done_all.copy()
        ended += int(pending.sum())
        if (t + 1) % 25 == 0:
            g = v.get_state()
            for k in ("x", "y", "angle", "vx", "vy", "progress", "flags", "finished_step"):
                assert np.array_equal(g[k].reshape(N, 2)[idx], st[k]), (t, k)
    assert ended >= 90
    v.close()


# ---- 4. lap events ----------------------------------------------------------------------------------
def test_lap_events_trace(golden, oracle_dev):
    """tests/test_lap_events_gpu.py's two-car form (130 envs, 4 slots: finishes, placements, contacts,
    timeouts, numpy start draws) on an env built with lane_cars=1: rows, end state and event census
    equal the CPU trace."""
    from tests.test_lap_events_gpu import _step_form
    _step_form(golden, lc.get("multi", golden, oracle_dev), {}, "two cars lane_cars 1",
               dict(lane_tracks=1, split=1, reward_lpe=1, ray_lpr=1), lane_cars=1)


# ---- 5. the step loops ------------------------------------------------------------------------------
T, N5, SLOTS5 = 16, 192, 48
NAMES = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")


def _venv5(mode):
    from rx.vector_env import RacingVectorEnv
    pool, _ = _pool(SLOTS5, "distinct", seed=51)
    widths = [float(6 + k % 4) for k in range(SLOTS5)]
    v = RacingVectorEnv([pool[i % SLOTS5] for i in range(N5)], [widths[i % SLOTS5] for i in range(N5)], n_agents=2,
                        device=DEV, seed=9, max_steps=12, lane_cars=mode)
    assert v.schedule()["lane_tracks"] == int(mode == 1) and len(np.unique(v.track_of_env)) == SLOTS5
    return v


def _agents(seeds, D=19):
    from rx.agent import Agent
    from rx.spaces import Box
    out = []
    for k, seed in enumerate(seeds):
        torch.manual_seed(seed)
        a = Agent(Box(-1.0, 1.0, shape=(D,), dtype=np.float32), Box(-1.0, 1.0, shape=(2,), dtype=np.float32)).to(DEV)
        with torch.no_grad():
            a.actor_mu[4].weight.mul_(40.0)  # the mean actions depend on the observation
            a.log_std.copy_(torch.tensor([-0.3 - 0.2 * k, -0.5 + 0.15 * k]))
        out.append(a)
    return out


def _bufs():
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    return [z(T, N5, 19), z(T, N5, 2), z(T, N5), z(T, N5), z(T, N5), z(T, N5)]


def _noise(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((T, N5, 2), device=DEV, generator=g), torch.randn((T, N5, 2), device=DEV, generator=g)


def _start(env, bufs):
    bufs[0][0].copy_(env.reset_device())
    bufs[3][0].zero_()
    return torch.full((N5, 19), float("nan"), device=DEV), torch.full((N5,), float("nan"), device=DEV)


def _same(a, b, names):
    for name, x, y in zip(names, a, b):
        assert not (x.is_floating_point() and torch.isnan(x).any()), name
        assert torch.equal(x, y), name


def _both(run):
    """run(mode) -> (tensors, env to close) on the grouped and on the lane-varying handle."""
    res = []
    for mode in (-1, 1):
        out, env = run(mode)
        torch.cuda.synchronize()
        res.append([x.clone() for x in out])
        env.close()
    return res


@pytest.mark.parametrize("duel", [False, True])
def test_selfplay_rollout_steps(duel):
    """rx_selfplay_rollout_steps, and rx_track_duel_rollout_steps with its per-track tallies."""
    from rx import _lib
    from rx.optim import FlatParams
    from rx.ppo_fused import SelfPlayStepRollout
    from rx.selfplay import SelfPlayVectorEnv
    from rx.track_selfplay import DuelSelfPlayStepRollout, DuelTrackCurriculum
    P = _lib.RX_PREC_FP32
    learner, opp = _agents((29, 21))
    flat, oflat = FlatParams(learner), FlatParams(opp)
    eps, oeps = _noise(8)

    def run(mode):
        sp = SelfPlayVectorEnv(_venv5(mode), 0)
        sp.set_opponent(opp, oflat, P)
        bufs = _bufs()
        nobs, nd = _start(sp, bufs)
        extra = []
        if duel:
            cur = DuelTrackCurriculum(sp.venv, 0, seed=5)
            DuelSelfPlayStepRollout(learner, flat, sp, T, cur, P)(*bufs, nobs, nd, eps=eps, opp_eps=oeps)
            extra = [cur.tally, cur.duel]
        else:
            SelfPlayStepRollout(learner, flat, sp, T, P)(*bufs, nobs, nd, eps=eps, opp_eps=oeps)
        return bufs + [nobs, nd, sp.venv.buf["obs"]] + extra, sp
    a, b = _both(run)
    _same(a, b, NAMES + ("env_obs", "tally", "duel"))
    assert int((a[3][1:] != 0).sum()) >= N5  # max_steps = 12: every env ended within the 16 steps
    if duel:
        assert int(a[-2][:, 0].sum()) >= N5 and (a[-2][:, 0] > 0).all()


def test_league_rollout_steps():
    from rx import _lib
    from rx.league_train import LeagueStepRollout, LeagueVectorEnv
    from rx.optim import FlatParams
    P = _lib.RX_PREC_FP32
    bank = _agents((31, 32))
    learner = _agents((39,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(18)

    def run(mode):
        lenv = LeagueVectorEnv(_venv5(mode), 0, seed=77, pool_size=3, prec=P)
        for k, a in enumerate(bank):
            lenv.set_slot(k, a)
        lenv.tally[:2].copy_(torch.tensor([[40, 30, 5], [25, 5, 15]]))
        lenv.weights(2, power=2, mix=0.1, prior=1.0)
        lenv.draw_all()
        bufs = _bufs()
        nobs, nd = _start(lenv, bufs)
        LeagueStepRollout(learner, flat, lenv, T, P)(*bufs, nobs, nd, eps=eps, opp_eps=oeps)
        return bufs + [nobs, nd, lenv.opp_id, lenv.draw_count, lenv.tally, lenv.venv.buf["obs"]], lenv
    a, b = _both(run)
    _same(a, b, NAMES + ("opp_id", "draw_count", "tally", "env_obs"))
    assert int((a[3][1:] != 0).sum()) >= N5 and len(torch.unique(a[8])) == 2


def test_match_steps():
    from rx.league import Match, PolicyBank, all_pairs, seating
    agents = _agents((41, 42, 43))
    bank = PolicyBank(agents, device=DEV)
    seat = seating(all_pairs(3), N5 // 6, 3)[:N5]

    def run(mode):
        m = Match(_venv5(mode), chunk=T)
        m.set_seat(seat, 3)
        m.begin()
        torch.manual_seed(60)  # the call's noise tensor: the same draws for both handles
        left = m.steps(bank, T)
        rec = torch.from_numpy(np.ascontiguousarray(m.fe.record())).to(DEV)
        return [rec, m.fe.actions[:T], m.fe.active, m.venv.buf["obs"], torch.tensor([left], device=DEV)], m.venv
    a, b = _both(run)
    _same(a, b, ("record", "actions", "active", "env_obs", "left"))
    assert int((a[2] == 0).sum()) == N5  # max_steps = 12: every episode ended


# ---- 6. pool changes --------------------------------------------------------------------------------
def test_pool_changes_keep_the_mode_and_auto_follows_the_pool():
    """256 envs on the 130-track pool: 7 slots group into 7 waves (at most 2 x 4: grouped), 130 slots into
    130 (lane-varying).  lane_cars=0 follows the redraws 7 -> 130 -> 7; lane_cars=1 stays on through
    reassign_tracks and set_tracks; the grouped twin sees the same outputs throughout."""
    from rx.track import TrackSet
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    N, S = 256, 130
    pool, widths = _pool(S, "distinct")
    ts = TrackSet.build(pool, widths)
    few = (np.arange(N) % 7).astype(np.int32)
    many = ((np.arange(N) * 37) % S).astype(np.int32)
    mk = lambda m: RacingVectorEnv([pool[k] for k in few], [widths[k] for k in few], n_agents=2, device=DEV, seed=9,  # noqa: E731
                                   max_steps=40, track_set=ts, lane_cars=m)
    vg, va, v1 = mk(-1), mk(0), mk(1)
    assert (vg.lane_cars, va.lane_cars, v1.lane_cars) == (-1, 0, 1)
    g = torch.Generator(device=DEV).manual_seed(3)
    want = [0, 1, 0]
    for i, toe in enumerate((few, many, few)):
        if i:
            obs = [v.reassign_tracks(toe) for v in (vg, va, v1)]
        else:
            obs = [v.reset_device() for v in (vg, va, v1)]
        assert torch.equal(obs[0], obs[1]) and torch.equal(obs[0], obs[2]), i
        lt = [v.schedule()["lane_tracks"] for v in (vg, va, v1)]
        assert lt == [0, want[i], 1], (i, lt)
        assert va.assign_plan()["schedule"]["lane_tracks"] == want[i] and (va.lane_cars, v1.lane_cars) == (0, 1)
        g2 = torch.Generator(device=DEV).manual_seed(int(g.initial_seed()) + i)
        assert _same_steps(vg, va, 45, g2, state_every=15) >= N
        g2 = torch.Generator(device=DEV).manual_seed(100 + i)
        vg.reassign_tracks(toe)
        v1.reassign_tracks(toe)
        assert _same_steps(vg, v1, 45, g2, state_every=15) >= N
    # set_tracks: a new table, the mode stays
    ys, yw = _pool(S, "distinct", seed=2)
    ty = TrackSet.build(ys, yw, backend="native")
    oa = vg.set_tracks(DeviceTrackTable.from_arrays(ty.arrays(), DEV), many)
    ob = v1.set_tracks(DeviceTrackTable.from_arrays(ty.arrays(), DEV), many)
    assert torch.equal(oa, ob) and v1.schedule()["lane_tracks"] == 1 and vg.schedule()["lane_tracks"] == 0
    assert _same_steps(vg, v1, 45, torch.Generator(device=DEV).manual_seed(5), state_every=15) >= N
    for v in (vg, va, v1):
        v.close()


def test_replace_tracks_equals_the_grouped_twin():
    """New tracks in some slots of the live pool (rx_replace_tracks_device rewrites those slots' headers,
    which every lane of the lane-varying kernels reads): obs, mask and the next 20 steps."""
    N = 130
    va, vb = _pair(N, "distinct", max_steps=30)
    assert torch.equal(va.reset_device(), vb.reset_device())
    g = torch.Generator(device=DEV).manual_seed(11)
    _same_steps(va, vb, 25, g)
    slots = np.array([0, 5, 64, 65, 129])
    cps = [np.asarray(va.tracks.geoms[k].control_points, dtype=np.float64) for k in slots]
    new = [c[::-1].copy() * 1.07 for c in cps]  # the slot's point count, another track
    ws = [7.0, 6.0, 9.0, 8.0, 6.5]
    (oa, ma), (ob, mb) = va.replace_tracks(slots, new, ws), vb.replace_tracks(slots, new, ws)
    assert torch.equal(oa, ob) and torch.equal(ma, mb) and int(ma.sum()) == len(slots)
    assert vb.schedule()["lane_tracks"] == 1
    _same_steps(va, vb, 20, g, state_every=10)
    va.close()
    vb.close()


# ---- 7. the default and the refusals ----------------------------------------------------------------
def test_default_is_off_and_the_schedule_words():
    from rx import _lib
    from rx.track import TrackSet
    from rx.vector_env import RacingVectorEnv
    N = 130
    pool, widths = _pool(N, "distinct")
    ts = TrackSet.build(pool, widths)
    v0 = RacingVectorEnv(pool, widths, n_agents=2, device=DEV, track_set=ts)  # no keyword: no call
    s = v0.schedule()
    assert s["lane_tracks"] == 0 and s["dyn_waves"] == 130 and v0.lane_cars == -1
    # rx_config.lane_tracks does not reach two-car envs
    vf = RacingVectorEnv(pool, widths, n_agents=2, device=DEV, track_set=ts, sched=dict(lane_tracks=1))
    assert vf.schedule()["lane_tracks"] == 0 and vf.schedule()["dyn_waves"] == 130
    v1 = RacingVectorEnv(pool, widths, n_agents=2, device=DEV, track_set=ts, lane_cars=1)
    s = v1.schedule()
    # the last block's 2 x 2 x 11 = 44 tasks fill one ray wave, the others have 22 each
    assert s["lane_tracks"] == 1 and s["dyn_waves"] == 3 and s["ray_waves"] == 3 * 22 - 21 and s["reserved"] == 0
    assert (s["ray_lpr"], s["reward_lpe"], s["ray_dispatch"], s["ray_tail"]) == (1, 1, 0, 0)
    assert v1.env_order()[1] == 0  # no re-sort bins
    p = v1.assign_plan()
    assert p["schedule"] == dict(s, dyn_calls=0) and np.array_equal(p["perm"], v1.env_order()[0])
    assert np.array_equal(p["ray_waves"].reshape(-1), np.stack(
        [v1.ray_wave_table()[k] for k in ("track", "perm_start", "task_start", "count")], 1).reshape(-1))
    va = RacingVectorEnv(pool, widths, n_agents=2, device=DEV, track_set=ts, lane_cars=0)
    assert va.schedule()["lane_tracks"] == 1  # 130 waves > 2 x 3
    # refusals
    L = _lib.load()
    single = RacingVectorEnv(pool[:4], widths[:4], device=DEV)
    assert L.rx_set_lane_cars(single._h, 1) == _lib.RX_EINVAL and b"lane_tracks governs" in L.rx_last_error()
    with pytest.raises(_lib.RxError, match="lane_tracks governs"):
        _lib.check(L.rx_set_lane_cars(single._h, 1), "rx_set_lane_cars")
    assert L.rx_set_lane_cars(v1._h, 2) == _lib.RX_EINVAL and b"lane_cars" in L.rx_last_error()
    with pytest.raises(ValueError, match="lane_cars"):
        RacingVectorEnv(pool[:4], widths[:4], device=DEV, lane_cars=1)
    with pytest.raises(ValueError, match="lane_cars"):
        RacingVectorEnv(pool[:4], widths[:4], n_agents=2, device=DEV, lane_cars=2)
    v1.reset_device()
    with pytest.raises(_lib.RxError, match="two-car"):
        v1.regroup_slots()
    with pytest.raises(_lib.RxError, match="two-car"):
        v1.lane_layout()
    import ctypes
    q = _lib.ptr
    tally = torch.zeros((N, 4), dtype=torch.int64, device=DEV)
    cdf = torch.arange(1, N + 1, dtype=torch.int64, device=DEV)
    p, draws = torch.zeros(N, dtype=torch.float64, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    tc = _lib.RxTrackIO(N, 0, q(v1._st["track"]), q(tally), q(cdf), q(p), None, 0)
    ep = _lib.RxTrackEpisodeIO(q(draws), None, None, None, 0.1)
    assert L.rx_track_episode_step(v1._h, ctypes.byref(tc), ctypes.byref(ep), v1._io_info(), None, None) == _lib.RX_EINVAL
    assert b"single-agent" in L.rx_last_error()
    from rx.track_episodic import check_episodic
    with pytest.raises(ValueError, match="single-agent"):
        check_episodic(v1)
    for v in (v0, vf, v1, va, single):
        v.close()


# ---- 8. training ------------------------------------------------------------------------------------
def test_selfplay_training_is_unchanged():
    """SelfPlayPPO at 256 envs x 16 steps on a 64-slot pool, 2 updates and one update_opponent:
    config["lane_cars"] = 1 against the key absent -- identical parameters after each update (the trainer
    keeps no loss log: every minibatch loss of the run went into them) and identical logged steps,
    pool sizes and episode counts."""
    from rx.configs import self_play_config
    from rx.envs import MultiRacingEnv
    from rx.selfplay import SelfPlayPPO
    n, slots = 256, 64
    res = []
    for lane_cars in (None, 1):
        over = {} if lane_cars is None else {"lane_cars": lane_cars}
        cfg = self_play_config(num_envs=n, num_steps=16, shuffle="device", checkpoint=False, snapshot_freq=1,
                               pool_size=2, num_minibatches=4, **over)
        cfg["total_timesteps"] = 2 * cfg["batch_size"]
        pool, _ = _pool(slots, "distinct", seed=cfg["seed"])
        pool = [pool[i % slots] for i in range(n)]
        widths = [6 + (i % slots) % 4 for i in range(n)]
        random.seed(cfg["seed"])
        np.random.seed(cfg["seed"])
        torch.manual_seed(cfg["seed"])
        t = SelfPlayPPO(lambda i: MultiRacingEnv(2, 11, pool, i, widths), cfg, device=DEV)
        assert t.envs.venv.schedule()["lane_tracks"] == int(lane_cars == 1)
        assert len(np.unique(t.envs.venv.track_of_env)) == slots
        params, logs, rets = [], [], []
        for update, _, gstep, ep, info in t.train_iter():  # update 1 follows a snapshot and an update_opponent
            torch.cuda.synchronize()
            params.append(torch.cat([p.detach().reshape(-1) for p in t.agent.parameters()]).clone())
            logs.append((gstep, ep.count, ep.sum_length, list(info["steps"]), list(info["opponent_pool_size"])))
            rets.append(float(ep.sum_return))
        assert update == 1 and len(t.opponent_pool) == 1 and t.curr_opponent is not None
        res.append((params, logs, rets))
        t.envs.close()
    (pa, la, ra), (pb, lb, rb) = res
    # the parameters after each update are functions of every minibatch loss and gradient of the run
    assert len(pa) == 2 and all(torch.equal(x, y) for x, y in zip(pa, pb)), "the schedule changed the training run"
    assert la == lb, "the logged steps / episode counts differ"
    # the episode statistics' shards add other env sets: tests/test_lane_tracks_gpu.py's bound
    assert all(abs(x - y) <= 1e-9 * max(1.0, abs(x)) for x, y in zip(ra, rb)), (ra, rb)
