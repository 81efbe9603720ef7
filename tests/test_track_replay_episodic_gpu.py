"""The replay scores on episodic draws on the GPU: k_track_adv_tally_slots and
k_track_learn_episode against their host twins byte for byte;
rx_track_learn_episodic_rollout_steps against the eager per-step loop; a captured graph of
the call against the twin's prediction of its slots; EpisodicReplayCurriculumPPO's scores
against the twins run on its own advantages, slots and dones; the handle refusals.
Everything compared is an integer or a bit pattern.

Every device output buffer of the kernel tests carries a guard element past its end.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.test_curriculum_cpu import tally_case, track_io
from tests.test_track_episodic_cpu import episode_io
from tests.test_track_episodic_gpu import GUARD, LANE, LANE_SMALL, NAMES, _agent, _bufs, _dev, _guarded, _pool
from tests.test_track_replay_cpu import host_tables, learn_io, score_case
from tests.test_track_replay_episodic_cpu import (NS, PATTERNS, TRACKS, TS, host_learn_episode, host_tally_slots,
                                                  py_learn_episode, slots_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _tables(L, n_tracks, power=2, now=9):
    """Replay tables of a mixed score case: ties, zeros, never-scored slots, some staleness."""
    score, seen = score_case("mixed", n_tracks, now=now)
    _, cs, ct = host_tables(L, score, seen, power, now)
    return score, seen, np.ascontiguousarray(cs), np.ascontiguousarray(ct)


# ---------------------------------------------------------------- 1. tally kernel == host twin
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n_tracks", TRACKS)
def test_tally_slots_kernel_equals_host_twin(L, n_tracks, kind):
    """The grid of the CPU test (T x n x slot pattern, dones null and a mask) plus 70 x 4,200: more than one
    env block and more than one row chunk.  learn starts from non-zero rows and carries a guard row."""
    from rx import _lib
    for T, n in [(T, n) for T in TS for n in NS] + [(70, 4200)]:
        for p, pattern in enumerate(PATTERNS):
            adv, slots, mask = slots_case(T, n, n_tracks, pattern, 1000 * T + 10 * n + p)
            d_adv, d_slots, d_mask = _dev(adv), _dev(slots), _dev(mask)
            for dones, d_dones in ((None, None), (mask, d_mask)):
                start = np.random.RandomState(T + n).randint(0, 9, size=(n_tracks + 1, 2)).astype(np.int64)
                want = start.copy()
                host_tally_slots(L, n_tracks, kind, want, adv, slots, dones)
                got = _dev(start)
                host_tally_slots(L, n_tracks, kind, got, d_adv, d_slots, d_dones, fn="rx_track_learn_tally_slots",
                                 stream=_lib.stream_ptr())
                torch.cuda.synchronize()
                assert got.cpu().numpy().tobytes() == want.tobytes(), (T, n, pattern, dones is not None)
                assert np.array_equal(want[n_tracks], start[n_tracks]), "guard row"
                assert T * n == 1 or not np.array_equal(want, start), "a case of 31 elements or more counts some"


@pytest.mark.parametrize("kind", [0, 1])
def test_tally_slots_kernel_with_constant_columns_is_the_tally_kernel(L, kind):
    """slots[t][e] == track[e] and dones null: rx_track_learn_tally's learn, kernel against kernel."""
    from rx import _lib
    from tests.test_track_replay_cpu import adv_case
    T, n, n_tracks = 70, 4200, 300
    track, adv = adv_case(T, n, n_tracks, 11)
    start = np.random.RandomState(3).randint(0, 9, size=(n_tracks, 2)).astype(np.int64)
    a, b = _dev(start), _dev(start)
    d_adv, d_track = _dev(adv), _dev(track)
    d_slots = d_track[None, :].expand(T, n).contiguous()
    lt = learn_io(_lib, n_tracks, kind, track=d_track, learn=a)
    assert L.rx_track_learn_tally(ctypes.byref(lt), T, n, _lib.ptr(d_adv), _lib.stream_ptr()) == 0, L.rx_last_error()
    host_tally_slots(L, n_tracks, kind, b, d_adv, d_slots, None, fn="rx_track_learn_tally_slots",
                     stream=_lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not np.array_equal(a.cpu().numpy(), start)


# ---------------------------------------------------------------- 2. episode kernel == host twin
@pytest.mark.parametrize("wave_order", [True, False])
@pytest.mark.parametrize("mode", ["none", "one_slot", "distinct", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4200])
def test_learn_episode_kernel_equals_host_twin(L, n, mode, wave_order):
    """The cases of tests/test_track_episodic_gpu.py's kernel test on replay tables, without staleness
    (cdf_stale null) and with stale_mix = 0.3."""
    from rx import _lib
    n_tracks, seed, mix = 67, 0xABCDEF0123456789, 0.1
    track, done, terminated, info = tally_case(n, n_tracks, 100 + n, mode)
    if mode == "random" and n >= 63:  # both kinds of slot outside the table end an episode at every size
        track[5], track[6], done[5], done[6] = -1, n_tracks, 1.0, 1.0
    rs = np.random.RandomState(n)
    _, _, cs, ct = _tables(L, n_tracks)
    assert ct[-1] > 0 and cs[-1] > 0
    env_pos = rs.permutation(n).astype(np.int32) if wave_order else None
    start = dict(tally=rs.randint(0, 1000, size=(n_tracks + 1, 4)).astype(np.int64), track=track,
                 draws=rs.randint(0, 7, size=n).astype(np.uint32), pos_slot=np.full(n, -9, dtype=np.int32),
                 slot_out=np.full(n, -5, dtype=np.int32))
    rows = {k: _dev(v) for k, v in dict(done=done, terminated=terminated, info=info, cs=cs, ct=ct).items()}
    pos_d = _dev(env_pos) if wave_order else None
    ended = (done != 0) & (track >= 0) & (track < n_tracks)
    for stale_mix in (0.0, 0.3):
        want = {k: v.copy() for k, v in start.items()}
        host_learn_episode(L, n_tracks, want["tally"], want["track"], want["draws"], cs, ct if stale_mix else None,
                           seed, mix, stale_mix, done, terminated, info, env_pos,
                           want["pos_slot"] if wave_order else None, want["slot_out"])
        if n <= 65:  # the twin itself against the restatement at the small sizes
            ref = {k: v.copy() for k, v in start.items()}
            ref["slot_out"], _ = py_learn_episode(ref["tally"][:n_tracks], ref["track"], ref["draws"], cs.tolist(),
                                                  ct.tolist(), seed, mix, stale_mix, done, terminated, info, env_pos,
                                                  ref["pos_slot"] if wave_order else None)
            for k in ref:
                assert np.array_equal(want[k], ref[k]), k
        d = {k: (_dev(v) if k == "tally" else _guarded(v)) for k, v in start.items()}
        host_learn_episode(L, n_tracks, d["tally"], d["track"], d["draws"], rows["cs"],
                           rows["ct"] if stale_mix else None, seed, mix, stale_mix, rows["done"], rows["terminated"],
                           rows["info"], pos_d, d["pos_slot"] if wave_order else None, d["slot_out"],
                           fn="rx_track_learn_episode", stream=_lib.stream_ptr())
        torch.cuda.synchronize()
        for k in start:
            got = d[k].cpu().numpy()
            if k != "tally":
                assert got[n] == GUARD, f"guard of {k}"
                got = got[:n].view(start[k].dtype)
            assert got.tobytes() == want[k].tobytes(), (k, stale_mix)
        assert np.array_equal(d["tally"].cpu().numpy()[n_tracks], start["tally"][n_tracks]), "guard row"
        assert np.array_equal(want["slot_out"], track)
        assert np.array_equal(want["track"][~ended], track[~ended])
        if mode == "none":
            for k in ("tally", "track", "draws", "pos_slot"):
                assert np.array_equal(want[k], start[k]), k
        if mode == "one_slot":
            assert want["tally"][n_tracks // 2, 0] - start["tally"][n_tracks // 2, 0] == n
        if ended.sum() > 100:
            assert (want["track"][ended] != track[ended]).mean() > 0.5


# ---------------------------------------------------------------- 3. rollout entry == eager loop
def _replay(L, venv, seed, n_tracks, mix, stale_mix=0.3):
    """A TrackReplay with the scores of a mixed case in place and its tables built."""
    from rx.track_replay import TrackReplay
    rep = TrackReplay(venv, seed, power=2, mix=mix, stale_mix=stale_mix)
    score, seen = score_case("mixed", n_tracks, now=9)
    rep.score.copy_(torch.from_numpy(score))
    rep.seen.copy_(torch.from_numpy(seen))
    rep.tables(9)
    return rep


def _eager(L, venv, cur, rep, ag, fl, bufs, eps, slots):
    """rx_policy_act + step + rx_track_learn_episode_step per step, slot_out into slots[s]."""
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
        rep.episode_step(cur, d, slot_out=slots[s])


@pytest.mark.parametrize("n_tracks", [64, 1])
def test_learn_episodic_rollout_steps_equals_the_eager_loop(L, n_tracks):
    """4,160 envs x 8 steps with max_steps = 3: every env ends an episode at steps 2 and 6.  From the same
    state on the same noise, every rollout buffer, the tally, track, draws and slots[T][N] of the one call
    equal the per-step eager path's.  The finish table (tc->cdf) is left all zero: it is not read."""
    from rx.curriculum import TrackCurriculum
    from rx.track_replay_episodic import ReplayEpisodicStepRollout
    from rx.vector_env import RacingVectorEnv
    N, T = 4160, 8
    pool, widths = _pool(n_tracks, 5)
    cps, ws = [pool[i % n_tracks] for i in range(N)], [widths[i % n_tracks] for i in range(N)]
    ag, fl = _agent()
    g = torch.Generator(device="cuda").manual_seed(6)
    eps = torch.randn((T, N, 2), device="cuda", generator=g) * 1.5
    runs = {}
    for path in ("call", "eager"):
        venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=3, sched=LANE)
        assert venv.schedule()["lane_tracks"] == 1
        cur = TrackCurriculum(venv, seed=3, mix=0.3)
        rep = _replay(L, venv, 3, n_tracks, 0.3)
        assert not cur.cdf.any()
        bufs = _bufs(venv, T)
        slots = torch.full((T, N), GUARD, dtype=torch.int32, device="cuda")
        if path == "call":
            sr = ReplayEpisodicStepRollout(ag, fl, venv, T, cur, rep)
            sr(*bufs, eps=eps)
            slots = sr.slots
        else:
            _eager(L, venv, cur, rep, ag, fl, bufs, eps, slots)
        torch.cuda.synchronize()
        assert venv._track_ids_stale
        runs[path] = dict(bufs=[x.clone() for x in bufs], tally=cur.tally.clone(), track=venv._st["track"].clone(),
                          draws=cur.draws.clone(), slots=slots.clone(), ids=venv.track_ids().copy())
        venv.close()
    a, b = runs["call"], runs["eager"]
    for k, x, y in zip(NAMES, a["bufs"], b["bufs"]):
        assert torch.equal(x, y), k
    for k in ("tally", "track", "draws", "slots"):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["ids"], a["track"].cpu().numpy())
    ends = int(a["bufs"][3].sum().item() + a["bufs"][7].sum().item())
    assert ends == int(a["draws"].sum().item()) == int(a["tally"][:, 0].sum().item()) and ends >= 2 * N
    assert (a["slots"] >= 0).all() and (a["slots"] < n_tracks).all()
    if n_tracks > 1:
        assert (a["slots"][0].cpu().numpy() == np.arange(N) % n_tracks).all(), "row 0: the slots of the assignment"
        assert (a["slots"][3] != a["slots"][0]).float().mean() > 0.5, "the envs that ended at step 2 moved"
        assert torch.equal(a["slots"][3], a["slots"][4])
    else:
        assert not a["track"].any()


# ---------------------------------------------------------------- 4. graph
def test_a_captured_graph_of_the_call_keeps_drawing_on_replay(L):
    """A captured graph of rx_track_learn_episodic_rollout_steps replayed twice: the draw counters live on
    the device, so the second replay draws at the next generations.  After each replay slots, track and
    draws equal the host twin stepped over the replay's own done rows from the state before it (the draw
    reads neither terminated nor info, so the twin gets zeros there)."""
    from rx.curriculum import TrackCurriculum
    from rx.track_replay_episodic import ReplayEpisodicStepRollout
    from rx.vector_env import RacingVectorEnv
    N, T, n_tracks, seed, mix, stale_mix = 200, 4, 16, 5, 0.2, 0.3
    pool, widths = _pool(n_tracks, 8)
    cps, ws = [pool[i % n_tracks] for i in range(N)], [widths[i % n_tracks] for i in range(N)]
    ag, fl = _agent()
    g = torch.Generator(device="cuda").manual_seed(2)
    eps = torch.randn((T, N, 2), device="cuda", generator=g) * 1.5
    venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=3, sched=LANE_SMALL)
    assert venv.schedule()["lane_tracks"] == 1
    cur = TrackCurriculum(venv, seed=seed, mix=mix)
    rep = _replay(L, venv, seed, n_tracks, mix, stale_mix)
    cs, ct = rep.cdf_score.cpu().numpy(), rep.cdf_stale.cpu().numpy()
    bufs = _bufs(venv, T)
    sr = ReplayEpisodicStepRollout(ag, fl, venv, T, cur, rep)

    def body():
        bufs[0][0].copy_(bufs[6])
        bufs[3][0].copy_(bufs[7])
        sr(*bufs, eps=eps)
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, capture_error_mode="thread_local"):
        body()
    assert not cur.draws.any(), "the capture records, it draws nothing"
    h_track = venv._st["track"].cpu().numpy().copy()
    h_draws = np.zeros(N, dtype=np.uint32)
    zeros_t, zeros_i = np.zeros(N, dtype=np.uint8), np.zeros((N, 4))
    seen_slots, totals = [], []
    for _ in range(2):
        cg.replay()
        torch.cuda.synchronize()
        dones, next_done = bufs[3].cpu().numpy(), bufs[7].cpu().numpy()
        want = np.zeros((T, N), dtype=np.int32)
        for t in range(T):
            row = np.ascontiguousarray(next_done if t + 1 == T else dones[t + 1])
            host_learn_episode(L, n_tracks, np.zeros((n_tracks, 4), dtype=np.int64), h_track, h_draws, cs, ct,
                               rep.seed, mix, stale_mix, row, zeros_t, zeros_i, slot_out=want[t])
        assert np.array_equal(sr.slots.cpu().numpy(), want)
        assert np.array_equal(venv._st["track"].cpu().numpy(), h_track)
        assert np.array_equal(cur.draws.cpu().numpy().view(np.uint32), h_draws)
        seen_slots.append(want)
        totals.append(int(h_draws.sum()))
    assert totals[0] >= N and totals[1] > totals[0], "the counters advance on replay"
    assert int(cur.tally[:, 0].sum().item()) == totals[1]
    assert not np.array_equal(seen_slots[0], seen_slots[1]), "the second replay runs other slots"
    venv.close()


# ---------------------------------------------------------------- 5. trainer
@pytest.mark.parametrize("rollout_steps", ["auto", "off"])
def test_episodic_replay_ppo_scores_equal_the_twins(L, monkeypatch, rollout_steps):
    """3 updates at 4,160 envs x 16 steps on a 64-slot pool, max_steps = 12, once through
    rx_track_learn_episodic_rollout_steps and once through the per-step loop.  After every update
    replay.score and replay.seen equal the host twins (tally_slots + fold) run on the downloaded advantages,
    slots() and dones; the finish tallies count every done flag; track_ids() is the device array; nobody is
    reset by the curriculum."""
    from rx import _lib, track_episodic
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.track_replay_episodic import EpisodicReplayCurriculumPPO
    build = track_episodic.build_vector_env
    monkeypatch.setattr(track_episodic, "build_vector_env", lambda *a, **kw: build(*a, max_steps=12, **kw))
    config = base_config(num_envs=4160, num_steps=16, kl_target=1e9, update_epochs=1, track_resample_every=1,
                         curriculum_refresh=0.0, rollout_steps=rollout_steps, replay_alpha=0.5, replay_power=2)
    config["total_timesteps"] = 3 * config["batch_size"]
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    pool, widths = _pool(64, 21)
    t = EpisodicReplayCurriculumPPO(
        lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 64, track_width=widths[i % 64]), config,
        device="cuda")
    assert t.envs.schedule()["lane_tracks"] == 1
    monkeypatch.setattr(t.envs, "reassign_tracks", lambda *a: pytest.fail("reassign_tracks was called"))
    monkeypatch.setattr(t.envs, "set_tracks", lambda *a: pytest.fail("set_tracks was called"))
    flags, collect, advantages = [], t.collect_rollout, t.compute_advantages
    h = dict(learn=np.zeros((64, 2), dtype=np.int64), score=np.zeros(64), seen=np.full(64, -1, dtype=np.int32))
    lt = learn_io(_lib, 64, 0, **h)
    moved = []

    def recording(*a):
        out = collect(*a)
        flags.append(int((out[3][1:] != 0).sum().item() + (out[7] != 0).sum().item()))
        return out

    def checking(rewards, dones, values, next_value, next_done):
        u = t.replay_updates
        adv, ret = advantages(rewards, dones, values, next_value, next_done)
        a, s, d = adv.cpu().numpy(), t.slots().cpu().numpy(), dones.cpu().numpy()
        assert s.shape == (16, 4160) and s.min() >= 0 and s.max() < 64
        assert L.rx_track_learn_tally_slots_host(ctypes.byref(lt), 16, 4160, _lib.ptr(a), _lib.ptr(s), _lib.ptr(d),
                                                 None) == 0, L.rx_last_error()
        assert L.rx_track_learn_fold_host(ctypes.byref(lt), u, 0.5, None) == 0, L.rx_last_error()
        assert t.replay.score.cpu().numpy().tobytes() == h["score"].tobytes(), u
        assert np.array_equal(t.replay.seen.cpu().numpy(), h["seen"]) and not t.replay.learn.any()
        # update 0 starts with 65 envs on every slot; later a low-ranked slot may go without samples
        assert (h["seen"] >= 0).all() and (h["score"] > 0).all() and 2 * (h["seen"] == u).sum() > 64
        moved.append(int((s[1:] != s[:-1]).sum()))
        assert moved[-1] == int(((s[1:] != s[:-1]) & (d[1:] != 0)).sum()), "a slot changes on an autoreset row only"
        return adv, ret
    t.collect_rollout, t.compute_advantages = recording, checking
    for u, _, _, _ in t.train_iter():
        dev = t.envs._st["track"].cpu().numpy()
        assert t.envs._track_ids_stale
        assert np.array_equal(t.envs.track_ids(), dev) and np.array_equal(t.envs.track_of_env, dev)
    assert u == 2 and t.replay_updates == 3 and len(moved) == 3 and min(moved) > 1000
    episodes = int(t.curriculum.tally[:, 0].sum().item())
    assert episodes == sum(flags) == int(t.curriculum.draws.sum().item()) and episodes >= 3 * 4160
    assert t.envs.track_generation == 0 and t.retired == [[], []]
    tab = t.track_table()
    assert np.array_equal(tab["score"], h["score"]) and sorted(tab["rank"].tolist()) == list(range(1, 65))
    assert abs(tab["prob"].sum() - 1.0) < 1e-9 and "prob_finishes" in tab
    for p in t.agent.parameters():
        assert torch.isfinite(p).all()
    t.envs.close()


# ---------------------------------------------------------------- 6. handle refusals
def test_refusals_that_need_a_handle(L):
    from rx import _lib
    from rx.curriculum import TrackCurriculum
    from rx.track_replay import TrackReplay
    from rx.vector_env import RacingVectorEnv
    pool, widths = _pool(4, 2)
    cps, ws = [pool[i % 4] for i in range(130)], [widths[i % 4] for i in range(130)]
    v = RacingVectorEnv(cps, ws, device="cuda", sched=dict(wide_n=-1, dyn_lpe=1, lane_tracks=-1))
    assert v.schedule()["lane_tracks"] == 0
    with pytest.raises(_lib.RxError, match="lane_tracks = 1"):
        TrackReplay(v, 1).episode_step(TrackCurriculum(v, seed=1))
    assert not v._track_ids_stale
    v.close()
    v = RacingVectorEnv(cps, ws, device="cuda", autoreset="same_step", sched=LANE_SMALL)
    assert v.schedule()["lane_tracks"] == 1
    with pytest.raises(_lib.RxError, match="autoreset"):
        TrackReplay(v, 1).episode_step(TrackCurriculum(v, seed=1))
    v.close()
    v = RacingVectorEnv(cps, ws, device="cuda", sched=LANE_SMALL)
    cur, rep = TrackCurriculum(v, seed=1), TrackReplay(v, 1)
    other = torch.zeros(130, dtype=torch.int32, device="cuda")
    tc = track_io(_lib, cur.n_tracks, track=other, tally=cur.tally, seed=1)
    rc = L.rx_track_learn_episode_step(v._h, ctypes.byref(tc), ctypes.byref(rep.lt), ctypes.byref(cur.episodic()),
                                       0.1, v._io_info(), None, None)
    assert rc == _lib.RX_EINVAL and b"rx_state.track" in L.rx_last_error()
    r = _lib.RxRolloutIO()
    rc = L.rx_track_learn_episodic_rollout_steps(v._h, v._io_info(), ctypes.byref(r), ctypes.byref(tc),
                                                 ctypes.byref(rep.lt), ctypes.byref(cur.episodic()), 0.1, None, 0, None)
    assert rc == _lib.RX_EINVAL and b"rx_state.track" in L.rx_last_error()
    v.close()
    v2 = RacingVectorEnv(cps, ws, n_agents=2, device="cuda")
    draws = torch.zeros(130, dtype=torch.int32, device="cuda")
    cdf = torch.ones(4, dtype=torch.int64, device="cuda")
    tc = track_io(_lib, 4, track=v2._st["track"], tally=torch.zeros((4, 4), dtype=torch.int64, device="cuda"))
    lt = learn_io(_lib, 4, cdf_score=cdf)
    rc = L.rx_track_learn_episode_step(v2._h, ctypes.byref(tc), ctypes.byref(lt), ctypes.byref(episode_io(_lib, draws)),
                                       0.0, v2._io(), None, None)
    assert rc == _lib.RX_EINVAL and b"single-agent" in L.rx_last_error()
    v2.close()
