"""Episodic track draws on the GPU: k_track_episode against its host twin byte for byte;
the env on the tracks it draws against the oracle, step by step; the draw in that loop
against the twin; rx_track_episodic_rollout_steps against the eager per-step loop and,
on a one-slot pool, against rx_track_rollout_steps; a captured graph of the call; and
EpisodicCurriculumPPO.  Everything compared is an integer or a bit pattern.

Every device output buffer of the kernel tests carries a guard element past its end.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from oracle.orc import sensor_angles, single_state
from tests.test_curriculum_cpu import tally_case, track_io
from tests.test_track_episodic_cpu import episode_io, host_episode, py_episode

pytestmark = pytest.mark.gpu

GUARD = -77
NAMES = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")
REL1 = sensor_angles(11, np.pi / 3)
LANE = dict(lane_tracks=1)                        # above 2,048 envs: one lane per env already
LANE_SMALL = dict(wide_n=-1, dyn_lpe=1, lane_tracks=1)


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(a):
    """A device copy of int array ``a`` with one guard element past its end."""
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a
    return _dev(np.concatenate([a, np.array([GUARD], dtype=a.dtype)]))


def _skewed_cdf(n_tracks, seed):
    """A hand-made table: weights over 12 orders of magnitude, slots 3 and n - 2 and a run of four weigh nothing."""
    rs = np.random.RandomState(seed)
    w = (2.0 ** rs.uniform(0, 40, size=n_tracks)).astype(np.int64)
    w[[3, n_tracks - 2]] = 0
    w[20:24] = 0
    return np.cumsum(w).astype(np.int64)


# ---------------------------------------------------------------- 1. kernel == host twin
@pytest.mark.parametrize("wave_order", [True, False])
@pytest.mark.parametrize("mode", ["none", "one_slot", "distinct", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4200])
def test_episode_kernel_equals_host_twin(L, n, mode, wave_order):
    """none: nobody ended, every output but slot_out untouched; one_slot: every env ended on ONE slot;
    distinct: 64 distinct slots in every full wave (67 slots); random: a mixed pattern with slots -1 and
    n_tracks, which are left alone.  env_pos: a random permutation, or null together with pos_slot."""
    from rx import _lib
    n_tracks, seed, mix = 67, 0xABCDEF0123456789, 0.1
    track, done, terminated, info = tally_case(n, n_tracks, 100 + n, mode)
    if mode == "random" and n >= 63:  # both kinds of slot outside the table end an episode at every size
        track[5], track[6], done[5], done[6] = -1, n_tracks, 1.0, 1.0
    rs = np.random.RandomState(n)
    cdf = _skewed_cdf(n_tracks, 3)
    env_pos = rs.permutation(n).astype(np.int32) if wave_order else None
    start = dict(tally=rs.randint(0, 1000, size=(n_tracks + 1, 4)).astype(np.int64), track=track,
                 draws=rs.randint(0, 7, size=n).astype(np.uint32), pos_slot=np.full(n, -9, dtype=np.int32),
                 slot_out=np.full(n, -5, dtype=np.int32))
    want = {k: v.copy() for k, v in start.items()}
    host_episode(L, n_tracks, want["tally"], want["track"], want["draws"], cdf, seed, mix, done, terminated, info,
                 env_pos, want["pos_slot"] if wave_order else None, want["slot_out"])
    if n <= 65:  # the twin itself against the restatement at the small sizes
        ref = {k: v.copy() for k, v in start.items()}
        ref["slot_out"] = py_episode(ref["tally"][:n_tracks], ref["track"], ref["draws"], cdf.tolist(), seed, mix,
                                     done, terminated, info, env_pos, ref["pos_slot"] if wave_order else None)
        for k in ref:
            assert np.array_equal(want[k], ref[k]), k
    d = {k: (_dev(v) if k == "tally" else _guarded(v)) for k, v in start.items()}
    rows = {k: _dev(v) for k, v in dict(done=done, terminated=terminated, info=info, cdf=cdf).items()}
    pos_d = _dev(env_pos) if wave_order else None
    host_episode(L, n_tracks, d["tally"], d["track"], d["draws"], rows["cdf"], seed, mix, rows["done"],
                 rows["terminated"], rows["info"], pos_d, d["pos_slot"] if wave_order else None, d["slot_out"],
                 fn="rx_track_episode", stream=_lib.stream_ptr())
    torch.cuda.synchronize()
    for k in start:
        got = d[k].cpu().numpy()
        if k != "tally":
            assert got[n] == GUARD, f"guard of {k}"
            got = got[:n].view(start[k].dtype)
        assert got.tobytes() == want[k].tobytes(), k
    assert np.array_equal(d["tally"].cpu().numpy()[n_tracks], start["tally"][n_tracks]), "guard row"
    assert np.array_equal(want["slot_out"], track)
    ended = (done != 0) & (track >= 0) & (track < n_tracks)
    assert np.array_equal(want["track"][~ended], track[~ended])
    if mode == "none":
        for k in ("tally", "track", "draws", "pos_slot"):
            assert np.array_equal(want[k], start[k]), k
    if mode == "one_slot":
        assert want["tally"][n_tracks // 2, 0] - start["tally"][n_tracks // 2, 0] == n
    if mode == "distinct" and n >= 64:
        assert len(set(track[:64].tolist())) == 64
    if mode == "random" and n >= 63:
        assert ((track == -1) & (done != 0)).any() and ((track == n_tracks) & (done != 0)).any()
    if ended.sum() > 100:
        assert (want["track"][ended] != track[ended]).mean() > 0.5


# ---------------------------------------------------------------- 2, 3. the env on the swapped track
def _golden_venv(golden, tracks, **kw):
    from rx.track import DEFAULT_CONTROL_POINTS
    from rx.vector_env import RacingVectorEnv
    cps = [DEFAULT_CONTROL_POINTS if golden.tracks[k]["label"] == "default" else golden.tracks[k]["cp"] for k in tracks]
    return RacingVectorEnv(cps, [golden.tracks[k]["width"] for k in tracks], **kw)


@pytest.fixture(scope="module")
def played(L, golden, oracle_dev):
    """200 steps of tests/test_env_gpu.py's random play on 4,200 envs over the 21 golden tracks with
    rx_track_episode_step after every step.  The oracle steps 320 of the envs: wave-order positions
    0-127, the 64 around the block boundary at 2,048 and the ragged last 128; the host twin draws for all
    4,200.  The env's table holds each distinct (control points, width) pair once, so the 21 golden tracks
    share 11 device slots: a drawn slot goes to the oracle as a golden track of that geometry.
    -> the first mismatch of each kind (None = none) and the counts the tests condition on."""
    from rx.curriculum import TrackCurriculum
    N, T = 4200, 200
    tracks = (np.arange(N) % golden.n_tracks).astype(np.int32)
    v = _golden_venv(golden, tracks, autoreset="next_step", sched=LANE)
    assert v.schedule()["lane_tracks"] == 1
    cur = TrackCurriculum(v, seed=11, mix=0.25)
    slot0 = v.track_of_env.copy()  # device slot of every env at the start; env k < 21 runs golden track k
    gold_of = np.full(cur.n_tracks, -1, dtype=np.int32)
    gold_of[slot0[:golden.n_tracks]] = np.arange(golden.n_tracks)
    assert (gold_of >= 0).all() and 2 <= cur.n_tracks <= golden.n_tracks
    assert np.array_equal(slot0[gold_of[slot0]], slot0), "a slot's golden track has that slot's geometry"
    cur.scores()  # fresh tallies: a uniform table; refreshed below as the tallies fill
    perm = v.env_order()[0]
    sub = perm[np.r_[0:128, 2016:2080, N - 128:N]].astype(np.int64)
    n_sub = len(sub)
    assert n_sub == 320 == len(set(sub.tolist()))
    tab = golden.table()
    st = single_state(n_sub)
    st["track"][:] = tracks[sub]
    o_obs = oracle_dev.single_reset(tab, st, REL1)
    res = dict(reset_equal=np.array_equal(v.reset_device().cpu().numpy()[sub], o_obs), env=None, draw=None,
               ends=np.zeros(n_sub, dtype=np.int64), changed=0, all_ends=0)
    h = dict(tally=np.zeros((cur.n_tracks, 4), dtype=np.int64), track=slot0.copy(),
             draws=np.zeros(N, dtype=np.uint32))
    rng = np.random.default_rng(7)
    pending, new_slot = np.zeros(n_sub, bool), slot0[sub]
    cdf = cur.cdf.cpu().numpy()
    for t in range(T):
        if t in (50, 120):  # the table follows the tallies; the twin reads the same bytes
            cur.scores()
            cdf = cur.cdf.cpu().numpy()
        a = np.stack([rng.uniform(-1, 1, N), rng.uniform(0.3, 1.0, N)], 1).astype(np.float32)
        obs, rew, done = v.step_device(torch.from_numpy(a).cuda(), full_info=True)
        cur.episode_step(done)
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        before = h["track"].copy()
        host_episode(L, cur.n_tracks, h["tally"], h["track"], h["draws"], cdf, cur.seed, cur.mix, done,
                     v.buf["terminated"].cpu().numpy(), v.buf["info"].cpu().numpy().reshape(N, 4))
        dev_track = v._st["track"].cpu().numpy()
        if res["draw"] is None and not np.array_equal(dev_track, h["track"]):
            res["draw"] = t
        res["all_ends"] += int((done != 0).sum())
        # the oracle with next-step autoreset: an env that ended last step resets on the slot it drew
        o_obs, o_rew, o_term, o_trunc, _ = oracle_dev.single_step(tab, st, a[sub], REL1)
        if pending.any():
            st["track"][pending] = gold_of[new_slot[pending]]
            r_obs = oracle_dev.single_reset(tab, st, REL1, mask=pending)
            o_obs[pending] = r_obs[pending]
            o_rew[pending] = 0.0
            o_term[pending] = False
            o_trunc[pending] = False
        o_done = o_term | o_trunc
        if res["env"] is None:
            for name, got, want in (("obs", obs[sub], o_obs), ("reward", rew[sub], o_rew.astype(np.float32)),
                                    ("done", done[sub].astype(bool), o_done)):
                if got.tobytes() != want.tobytes():
                    res["env"] = (t, name, int(np.argwhere(got != want)[0][0]))
                    break
        pending = o_done
        new_slot = dev_track[sub]  # what the device drew for the envs that ended in this step
        res["ends"] += o_done
        res["changed"] += int((o_done & (new_slot != before[sub])).sum())
    g = v.get_state()
    res["state"] = [k for k in ("x", "y", "angle", "vx", "vy", "steps", "flags")
                    if g[k][sub].tobytes() != st[k].tobytes()]
    res["track_state"] = np.array_equal(g["track"][sub], np.where(pending, new_slot, slot0[st["track"]]))
    res["tally"] = (cur.tally.cpu().numpy(), h["tally"])
    res["draws"] = (cur.draws.cpu().numpy().view(np.uint32), h["draws"])
    res["track_ids"] = (v.track_ids().copy(), h["track"])
    v.close()
    return res


def test_env_on_the_swapped_tracks_is_bit_exact_vs_oracle_dev(played):
    """obs, reward and done of the 320 oracle envs are bit-identical at every step and the state at the
    end, with every env that ended restarted on the slot the device drew for it.

    Conditioned so that it cannot pass vacuously: at least 400 episode ends in the subset, at least 20
    subset envs with three or more, at least half of the ends on a new slot (expected from the oracle
    alone with uniform new slots: about 890 ends in a 320-env subset, 95 % of them slot changes)."""
    r = played
    print("subset ends", int(r["ends"].sum()), "envs with >= 3", int((r["ends"] >= 3).sum()), "slot changes",
          r["changed"], "ends of all envs", r["all_ends"])
    assert r["reset_equal"]
    assert r["ends"].sum() >= 400
    assert (r["ends"] >= 3).sum() >= 20
    assert 2 * r["changed"] >= r["ends"].sum()
    assert r["env"] is None, f"first mismatch (step, output, subset row): {r['env']}"
    assert r["state"] == [], r["state"]
    assert r["track_state"]


def test_the_draw_in_the_loop_equals_the_host_twin(played):
    """The device's track array after every step equals the host twin fed the same done, terminated and
    info rows, on all 4,200 envs; so do the tally and the counters at the end, and track_ids()."""
    r = played
    assert r["draw"] is None, f"first step with a different draw: {r['draw']}"
    assert r["all_ends"] >= 4200
    for k in ("tally", "draws", "track_ids"):
        assert np.array_equal(*r[k]), k
    assert r["tally"][0][:, 0].sum() == r["all_ends"] == r["draws"][0].sum()


# ---------------------------------------------------------------- 4. rollout entry == eager loop
def _pool(n_tracks, seed):
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    return gen_tracks(n_tracks, seed=None, rng=rng), [int(rng.randint(6, 10)) for _ in range(n_tracks)]


def _agent():
    from rx.agent import Agent
    from rx.optim import FlatAdam
    from rx.spaces import Box
    torch.manual_seed(9)
    ag = Agent(Box(-1, 1, (15,)), Box(-1, 1, (2,))).cuda()
    with torch.no_grad():
        ag.log_std.fill_(-0.3)
    return ag, FlatAdam(ag, torch.optim.Adam(ag.parameters(), lr=1e-3, eps=1e-5), 0.5)


def _bufs(venv, T):
    N = venv.num_envs
    obs = torch.zeros((T, N, 15), device="cuda")
    actions = torch.zeros((T, N, 2), device="cuda")
    logprobs, dones, rewards, values = (torch.zeros((T, N), device="cuda") for _ in range(4))
    nobs = venv.reset_device().clone()
    nd = torch.zeros(N, device="cuda")
    obs[0].copy_(nobs)
    dones[0].copy_(nd)
    return (obs, actions, logprobs, dones, rewards, values, nobs, nd)


def _eager(L, venv, cur, ag, fl, bufs, eps, slots=None, episodic=True):
    """rx_policy_act + step + rx_track_episode_step (or the plain tally) per step."""
    from rx import _lib
    obs, actions, logprobs, dones, rewards, values, nobs, nd = bufs
    T, N = obs.shape[0], obs.shape[1]
    for s in range(T):
        io = _lib.RxPolicyIO(15, N, _lib.ptr(obs[s]), _lib.ptr(eps[s]), _lib.ptr(fl.flat_param), _lib.ptr(ag.log_std),
                             _lib.ptr(actions[s]), _lib.ptr(logprobs[s]), _lib.ptr(values[s]), 0, 0)
        _lib.check(L.rx_policy_act(io, _lib.stream_ptr()), "rx_policy_act")
        last = s + 1 == T
        _, _, d = venv.step_device(actions[s], obs_out=nobs if last else obs[s + 1], reward_out=rewards[s],
                                   done_out=nd if last else dones[s + 1], full_info=True)
        if slots is not None:
            slots[s].copy_(venv._st["track"])
        cur.episode_step(d) if episodic else cur.tally_step(d)


@pytest.mark.parametrize("n_tracks", [64, 1])
def test_episodic_rollout_steps_equals_the_eager_loop(L, n_tracks):
    """4,160 envs x 8 steps with max_steps = 3: every env ends an episode at steps 2 and 6.  From the same state on the
    same noise, every rollout buffer, the tally, track, draws and slots[T][N] of the one call equal the
    per-step eager path's.  On a one-slot pool every draw is slot 0, and every rollout output and the tally
    equal rx_track_rollout_steps' bit for bit."""
    from rx.curriculum import CurriculumStepRollout, TrackCurriculum
    from rx.track_episodic import EpisodicStepRollout
    from rx.vector_env import RacingVectorEnv
    N, T = 4160, 8
    pool, widths = _pool(n_tracks, 5)
    cps, ws = [pool[i % n_tracks] for i in range(N)], [widths[i % n_tracks] for i in range(N)]
    ag, fl = _agent()
    g = torch.Generator(device="cuda").manual_seed(6)
    eps = torch.randn((T, N, 2), device="cuda", generator=g) * 1.5
    runs = {}
    for path in ("call", "eager") + (("tally",) if n_tracks == 1 else ()):
        venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=3, sched=LANE)
        assert venv.schedule()["lane_tracks"] == 1
        cur = TrackCurriculum(venv, seed=3, mix=0.3)
        cur.tally[:, 1] = torch.arange(n_tracks, device="cuda") % 5  # a table that is not uniform
        cur.tally[:, 0] = 6
        cur.scores()
        bufs = _bufs(venv, T)
        slots = torch.full((T, N), GUARD, dtype=torch.int32, device="cuda")
        if path == "call":
            sr = EpisodicStepRollout(ag, fl, venv, T, cur, record_slots=True)
            sr(*bufs, eps=eps)
            slots = sr.slots
        elif path == "eager":
            _eager(L, venv, cur, ag, fl, bufs, eps, slots)
        else:
            CurriculumStepRollout(ag, fl, venv, T, cur)(*bufs, eps=eps)
        torch.cuda.synchronize()
        runs[path] = dict(bufs=[x.clone() for x in bufs], tally=cur.tally.clone(), track=venv._st["track"].clone(),
                          draws=cur.draws.clone() if path != "tally" else None, slots=slots.clone(),
                          ids=venv.track_ids().copy())
        venv.close()
    a, b = runs["call"], runs["eager"]
    for k, x, y in zip(NAMES, a["bufs"], b["bufs"]):
        assert torch.equal(x, y), k
    for k in ("tally", "track", "draws", "slots"):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["ids"], a["track"].cpu().numpy())
    ends = int(a["bufs"][3].sum().item() + a["bufs"][7].sum().item())
    assert ends == int(a["draws"].sum().item()) == int(a["tally"][:, 0].sum().item()) - 6 * n_tracks and ends >= 2 * N
    assert (a["slots"] >= 0).all() and (a["slots"] < n_tracks).all()
    if n_tracks > 1:
        assert (a["slots"][0].cpu().numpy() == np.arange(N) % n_tracks).all(), "row 0: the slots of the assignment"
        assert (a["slots"][3] != a["slots"][0]).float().mean() > 0.5, "the envs that ended at step 2 moved"
        assert torch.equal(a["slots"][3], a["slots"][4])
    else:
        c = runs["tally"]
        for k, x, y in zip(NAMES, a["bufs"], c["bufs"]):
            assert torch.equal(x, y), k
        assert torch.equal(a["tally"], c["tally"]) and not a["track"].any()


# ---------------------------------------------------------------- 5. graph
def test_a_captured_graph_of_the_call_keeps_drawing(L):
    """A captured graph of rx_track_episodic_rollout_steps replayed twice equals two eager calls: the
    draw counters live on the device, so the second replay draws at the next generation."""
    from rx.curriculum import TrackCurriculum
    from rx.track_episodic import EpisodicStepRollout
    from rx.vector_env import RacingVectorEnv
    N, T, n_tracks = 200, 4, 16
    pool, widths = _pool(n_tracks, 8)
    cps, ws = [pool[i % n_tracks] for i in range(N)], [widths[i % n_tracks] for i in range(N)]
    ag, fl = _agent()
    g = torch.Generator(device="cuda").manual_seed(2)
    eps = torch.randn((T, N, 2), device="cuda", generator=g) * 1.5
    runs = []
    for graph in (False, True):
        venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=3, sched=LANE_SMALL)
        assert venv.schedule()["lane_tracks"] == 1
        cur = TrackCurriculum(venv, seed=5, mix=0.2)
        cur.scores()
        bufs = _bufs(venv, T)
        sr = EpisodicStepRollout(ag, fl, venv, T, cur, record_slots=True)

        def body():
            bufs[0][0].copy_(bufs[6])
            bufs[3][0].copy_(bufs[7])
            sr(*bufs, eps=eps)
        draws = []
        if graph:
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, capture_error_mode="thread_local"):
                body()
            assert not cur.draws.any(), "the capture records, it draws nothing"
        for _ in range(2):
            cg.replay() if graph else body()
            torch.cuda.synchronize()
            draws.append(cur.draws.clone())
        runs.append(dict(bufs=[x.clone() for x in bufs], tally=cur.tally.clone(), track=venv._st["track"].clone(),
                         draws=draws, slots=sr.slots.clone()))
        venv.close()
    a, b = runs
    for k, x, y in zip(NAMES, a["bufs"], b["bufs"]):
        assert torch.equal(x, y), k
    for k in ("tally", "track", "slots"):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a["draws"], b["draws"]):
        assert torch.equal(x, y)
    first, second = (int(x.sum().item()) for x in b["draws"])
    assert first >= N and second > first, "the counters advance on replay"


# ---------------------------------------------------------------- 6. trainer
@pytest.mark.parametrize("rollout_steps", ["auto", "off"])
def test_episodic_curriculum_ppo_tallies_every_episode(L, monkeypatch, rollout_steps):
    """2 updates at 4,160 envs x 16 steps on a 64-slot pool, max_steps = 12: the tally's episode sum is the
    count of done flags in the rollouts and episode_stats' count; no env was reset by the curriculum;
    track_ids() is the device array.  Once through rx_track_episodic_rollout_steps and once through the
    per-step loop (rx_track_episode_step after every step)."""
    from rx import track_episodic
    from rx.configs import base_config
    from rx.envs import RacingEnv
    build = track_episodic.build_vector_env
    monkeypatch.setattr(track_episodic, "build_vector_env", lambda *a, **kw: build(*a, max_steps=12, **kw))
    config = base_config(num_envs=4160, num_steps=16, kl_target=1e9, update_epochs=1, track_resample_every=1,
                         curriculum_refresh=0.0, episodic_slots=True, rollout_steps=rollout_steps)
    config["total_timesteps"] = 2 * config["batch_size"]
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    pool, widths = _pool(64, 21)
    t = track_episodic.EpisodicCurriculumPPO(
        lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 64, track_width=widths[i % 64]), config,
        device="cuda")
    assert t.envs.schedule()["lane_tracks"] == 1 and t.envs.sched == dict(lane_tracks=1)
    flags, counted, collect = [], [], t.collect_rollout
    monkeypatch.setattr(t.envs, "reassign_tracks", lambda *a: pytest.fail("reassign_tracks was called"))
    monkeypatch.setattr(t.envs, "set_tracks", lambda *a: pytest.fail("set_tracks was called"))

    def recording(*a):
        out = collect(*a)
        flags.append(int((out[3][1:] != 0).sum().item() + (out[7] != 0).sum().item()))
        counted.append(len(out[8]))
        return out
    t.collect_rollout = recording
    assert [u for u, _, _, _ in t.train_iter()] == [0, 1]
    episodes = int(t.curriculum.tally[:, 0].sum().item())
    assert episodes == sum(flags) == sum(counted) and episodes >= 2 * 4160
    assert int(t.curriculum.draws.sum().item()) == episodes
    assert t.envs.track_generation == 0 and t.retired == [[]]
    dev = t.envs._st["track"].cpu().numpy()
    assert t.envs._track_ids_stale
    assert np.array_equal(t.envs.track_ids(), dev) and np.array_equal(t.envs.track_of_env, dev)
    assert not np.array_equal(dev, np.arange(4160) % 64), "the envs moved"
    if rollout_steps == "off":
        assert t.slots() is None, "the per-step loop was not taken"
    else:
        s = t.slots().cpu().numpy()
        assert s.shape == (16, 4160) and s.min() >= 0 and s.max() < 64
    for p in t.agent.parameters():
        assert torch.isfinite(p).all()
    t.envs.close()


def test_refusals_that_need_a_handle(L):
    from rx import _lib
    from rx.configs import base_config
    from rx.curriculum import TrackCurriculum
    from rx.envs import RacingEnv
    from rx.track_episodic import EpisodicCurriculumPPO, check_episodic
    from rx.vector_env import RacingVectorEnv
    pool, widths = _pool(4, 2)
    cps, ws = [pool[i % 4] for i in range(130)], [widths[i % 4] for i in range(130)]
    # a slot-uniform schedule: 64 envs run the wide kernels, which lane_tracks = 1 cannot override
    with pytest.raises(ValueError, match="lane-varying"):
        EpisodicCurriculumPPO(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 4,
                                                  track_width=widths[i % 4]), base_config(num_envs=64, num_steps=16))
    v = RacingVectorEnv(cps, ws, device="cuda", sched=dict(wide_n=-1, dyn_lpe=1, lane_tracks=-1))
    assert v.schedule()["lane_tracks"] == 0
    with pytest.raises(_lib.RxError, match="lane_tracks = 1"):
        TrackCurriculum(v, seed=1).episode_step()
    with pytest.raises(ValueError, match="lane-varying"):
        check_episodic(v)
    assert not v._track_ids_stale
    v.close()
    v = RacingVectorEnv(cps, ws, device="cuda", autoreset="same_step", sched=LANE_SMALL)
    assert v.schedule()["lane_tracks"] == 1
    with pytest.raises(_lib.RxError, match="autoreset"):
        TrackCurriculum(v, seed=1).episode_step()
    with pytest.raises(ValueError, match="next_step"):
        check_episodic(v)
    v.close()
    v = RacingVectorEnv(cps, ws, device="cuda", sched=LANE_SMALL)
    cur = TrackCurriculum(v, seed=1)
    other = torch.zeros(130, dtype=torch.int32, device="cuda")
    tc = track_io(_lib, cur.n_tracks, track=other, tally=cur.tally, cdf=cur.cdf, seed=1)
    rc = L.rx_track_episode_step(v._h, ctypes.byref(tc), ctypes.byref(cur.episodic()), v._io_info(), None, None)
    assert rc == _lib.RX_EINVAL and b"rx_state.track" in L.rx_last_error()
    v.close()
    v2 = RacingVectorEnv(cps, ws, n_agents=2, device="cuda")
    draws = torch.zeros(130, dtype=torch.int32, device="cuda")
    tc = track_io(_lib, 4, track=v2._st["track"], tally=torch.zeros((4, 4), dtype=torch.int64, device="cuda"),
                  cdf=torch.ones(4, dtype=torch.int64, device="cuda"))
    rc = L.rx_track_episode_step(v2._h, ctypes.byref(tc), ctypes.byref(episode_io(_lib, draws)), v2._io(), None, None)
    assert rc == _lib.RX_EINVAL and b"single-agent" in L.rx_last_error()
    v2.close()
