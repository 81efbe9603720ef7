"""The track curriculum for self-play without a GPU: the host twins rx_track_tally2_host
and rx_track_duel_scores_host against a Python restatement of csrc/rx_track_duel.h written
here (bit for bit: float64 operations separately rounded in a fixed order, integer weights
and sums), scores 0 and 1 against rx_track_scores_host, every argument check that runs
before a HIP call, and the refusals of DuelTrackCurriculum and the two trainers."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_curriculum_cpu import py_scores, track_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rx_track_tally2", "rx_track_tally2_host", "rx_track_duel_scores", "rx_track_duel_scores_host",
       "rx_track_duel_rollout_steps")
PROGRESS, PLACEMENT = 1, 3  # RX_INFO_PROGRESS, RX_INFO_PLACEMENT
C = 1024  # RX_TRACK_SCORES_CHUNK


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the Python restatement (shared with tests/test_track_selfplay_gpu.py) -------------------------
def py_tally2(tally, duel, agent, track, done, terminated, info):
    """In place, env by env; tally and duel int64 [n_tracks, 4], info float64 [n, 2, 4]."""
    n_tracks = len(tally)
    a, o = agent, 1 - agent
    for e in range(len(done)):
        k = int(track[e])
        if done[e] == 0 or not 0 <= k < n_tracks:
            continue
        pa, po, la = np.float64(info[e, a, PROGRESS]), np.float64(info[e, o, PROGRESS]), info[e, a, PLACEMENT]
        tally[k, 0] += 1
        tally[k, 1] += int(pa == 1.0)
        tally[k, 2] += int(terminated[e] != 0 and pa != 1.0 and po != 1.0)
        tally[k, 3] += int(pa * np.float64(1048576.0))  # truncation
        duel[k, 0] += int(la == 1.0)
        duel[k, 1] += int(po == 1.0)
        duel[k, 2] += int(po * np.float64(1048576.0))
        duel[k, 3] += int(terminated[e] == 0)


def py_duel_scores(tally, duel, score, power, prior):
    """-> (cdf as Python ints, p float64 [n], W as Python ints): the four scores written out."""
    f8 = np.float64
    prior = f8(prior)
    cdf, p, W, c = [], np.zeros(len(tally), dtype=f8), [], 0
    for k in range(len(tally)):
        n = f8(int(tally[k, 0]))
        good = f8(int(duel[k, 0] if score >= 2 else tally[k, 1]))  # wins for lose / contested, finishes else
        pk = (good + prior) / (n + f8(2.0) * prior)
        rest = f8(1.0) - pk
        q = (f8(4.0) * pk) * rest if score in (1, 3) else rest
        f = f8(1.0)
        for _ in range(power):
            f = f * q
        w = f * f8(4294967296.0)
        w = int(w) if w > 0.0 else 0
        c += w
        p[k] = pk
        W.append(w)
        cdf.append(c)
    assert c < 1 << 63
    return cdf, p, W


def duel_io(_lib, agent, duel):
    return _lib.RxTrackDuelIO(agent, _lib.ptr(duel))


MODES = ("random", "one_slot", "distinct", "none")


def tally2_case(n, n_tracks, seed, mode="random"):
    """Synthetic terminal-step buffers of n two-car envs -> (track, done, terminated, info [n, 2, 4]).
    random: slots outside the table (-1 and n_tracks), finishes by either car (progress exactly 1.0,
    terminated, placement 1 to the finisher), both-crashed terminations (neither finished,
    terminated), timeouts (not terminated), progress values next to 1.0 and 0.0."""
    rs = np.random.RandomState(seed)
    track = rs.randint(-1, n_tracks + 1, size=n).astype(np.int32)
    done = (rs.rand(n) < 0.6).astype(np.float32)
    kind = rs.randint(0, 5, size=n)  # 0: car 0 finished, 1: car 1 finished, 2: both crashed, 3 / 4: timeout
    vals = np.array([0.0, 0.25, 1.0 - 2.0 ** -53, 0.999999, 1e-7, 0.7312345678])
    prog = np.where(rs.rand(n, 2) < 0.5, rs.rand(n, 2), rs.choice(vals, size=(n, 2)))
    prog[kind == 0, 0] = 1.0
    prog[kind == 1, 1] = 1.0
    terminated = (kind <= 2).astype(np.uint8)
    lead = np.where(prog[:, 0] >= prog[:, 1], 0, 1)  # placement 1 to the car further along
    info = np.zeros((n, 2, 4), dtype=np.float64)
    info[:, :, 0], info[:, :, 2] = rs.rand(n, 2), rs.rand(n, 2)
    info[:, :, PROGRESS] = prog
    info[np.arange(n), lead, PLACEMENT] = 1.0
    info[np.arange(n), 1 - lead, PLACEMENT] = 2.0
    if mode == "one_slot":  # full contention: every env ended on ONE slot
        track[:] = n_tracks // 2
        done[:] = 1.0
    elif mode == "distinct":  # every lane of a wave on a different slot (while n_tracks >= 64)
        track[:] = np.arange(n) % n_tracks
        done[:] = 1.0
    elif mode == "none":
        done[:] = 0.0
    return track, done, terminated, info


def start_tables(n_tracks, seed=3):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 9, size=(n_tracks + 1, 4)).astype(np.int64), \
        rs.randint(0, 9, size=(n_tracks + 1, 4)).astype(np.int64)  # the last row is the guard


def make_duel_tally(kind, n, seed=5):
    """(tally, duel).  fresh: no episode; mastered: 1,000 episodes all finished and all won (W_k == 0 at
    power 4 for fail and lose, prior 1); mixed: random counts with wins <= episodes, slot 1 mastered."""
    rs = np.random.RandomState(seed)
    t, d = np.zeros((n, 4), dtype=np.int64), np.zeros((n, 4), dtype=np.int64)
    if kind == "mastered":
        t[:] = (1000, 1000, 0, 1000 << 20)
        d[:] = (1000, 0, 500 << 20, 0)
    elif kind == "mixed":
        t[:, 0] = rs.randint(0, 50, size=n)
        t[:, 1] = (rs.rand(n) * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
        t[:, 2] = (rs.rand(n) * (t[:, 0] - t[:, 1] + 1)).astype(np.int64).clip(0, t[:, 0] - t[:, 1])
        t[:, 3] = rs.randint(0, 1 << 30, size=n)
        d[:, 0] = (rs.rand(n) * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
        d[:, 1] = (rs.rand(n) * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
        d[:, 2] = rs.randint(0, 1 << 30, size=n)
        d[:, 3] = t[:, 0] - t[:, 1] - t[:, 2]
        if n > 2:
            t[1], d[1] = (1000, 1000, 0, 1000 << 20), (1000, 0, 500 << 20, 0)
    return t, d


# ---- 1: the ABI, the layout, the build lists ------------------------------------------------------
def test_abi_is_still_25_and_the_new_symbols_are_exported(L):
    from rx import _build, _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name
    T = _lib.RxTrackDuelIO
    assert ctypes.sizeof(T) == 16 and T.agent.offset == 0 and T.duel.offset == 8
    assert ctypes.sizeof(_lib.RxTrackIO) == 56  # additive: rx_track_io is unchanged
    assert _lib.RX_TRACK_DUEL_W == 4 and "#define RX_TRACK_DUEL_W 4" in hdr
    assert _lib.TRACK_SCORES == {"fail": 0, "potential": 1}  # the single-agent calls keep their two
    assert _lib.TRACK_DUEL_SCORES == {"fail": 0, "potential": 1, "lose": 2, "contested": 3}
    assert "rx_track_duel.h" in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, "rx_track_duel.h"))


# ---- 2: rx_track_tally2_host ----------------------------------------------------------------------
def test_random_case_holds_every_outcome():
    n_tracks = 7
    track, done, terminated, info = tally2_case(300, n_tracks, 11)
    ended = done != 0
    pa, po = info[:, 0, PROGRESS], info[:, 1, PROGRESS]
    assert (track[ended] == -1).any() and (track[ended] == n_tracks).any()
    assert (ended & (pa == 1.0)).any() and (ended & (po == 1.0)).any()
    assert (ended & (terminated != 0) & (pa != 1.0) & (po != 1.0)).any(), "both crashed"
    assert (ended & (terminated == 0)).any(), "timeout"
    assert (ended & (terminated != 0) & (po == 1.0) & (pa != 1.0)).any(), "a lost race: terminated, no crash"


@pytest.mark.parametrize("agent", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_tally2_host_equals_the_restatement(L, n, mode, agent):
    from rx import _lib
    n_tracks = 67
    track, done, terminated, info = tally2_case(n, n_tracks, 11 + n, mode)
    want_t, want_d = start_tables(n_tracks)  # not from zero
    got_t, got_d = want_t.copy(), want_d.copy()
    py_tally2(want_t[:-1], want_d[:-1], agent, track, done, terminated, info)
    tc = track_io(_lib, n_tracks, track=track, tally=got_t)
    td = duel_io(_lib, agent, got_d)
    q = _lib.ptr
    assert L.rx_track_tally2_host(ctypes.byref(tc), ctypes.byref(td), n, q(done), q(terminated), q(info), None) == 0, \
        L.rx_last_error()
    assert np.array_equal(got_t, want_t) and np.array_equal(got_d, want_d)
    t0, d0 = start_tables(n_tracks)
    assert np.array_equal(got_t[-1], t0[-1]) and np.array_equal(got_d[-1], d0[-1]), "the guard row"
    if mode == "none":
        assert np.array_equal(got_t, t0) and np.array_equal(got_d, d0)
    else:
        counted = int(((done != 0) & (track >= 0) & (track < n_tracks)).sum())
        assert int((got_t[:, 0] - t0[:, 0]).sum()) == counted
        # losses are episodes - wins: wins never exceed the episodes of a slot
        assert ((got_d[:, 0] - d0[:, 0]) <= (got_t[:, 0] - t0[:, 0])).all()


def test_a_lost_race_is_not_a_crash(L):
    """One env: the opponent finished (terminated), the learner did not.  rx_tc_outcome would book a crash."""
    from rx import _lib
    info = np.zeros((1, 2, 4))
    info[0, 0, PROGRESS], info[0, 1, PROGRESS] = 0.5, 1.0
    info[0, 0, PLACEMENT], info[0, 1, PLACEMENT] = 2.0, 1.0
    track, done, term = np.zeros(1, np.int32), np.ones(1, np.float32), np.ones(1, np.uint8)
    q = _lib.ptr
    for agent, want_t, want_d in ((0, [1, 0, 0, 1 << 19], [0, 1, 1 << 20, 0]), (1, [1, 1, 0, 1 << 20], [1, 0, 1 << 19, 0])):
        t, d = np.zeros((1, 4), np.int64), np.zeros((1, 4), np.int64)
        tc, td = track_io(_lib, 1, track=track, tally=t), duel_io(_lib, agent, d)
        assert L.rx_track_tally2_host(ctypes.byref(tc), ctypes.byref(td), 1, q(done), q(term), q(info), None) == 0
        assert t[0].tolist() == want_t and d[0].tolist() == want_d


# ---- 3: rx_track_duel_scores_host -----------------------------------------------------------------
def _host_scores(L, tally, duel, score, power, prior=1.0):
    from rx import _lib
    n = len(tally)
    cdf, p = np.full(n + 1, -7, dtype=np.int64), np.full(n + 1, -7.0)
    tc, td = track_io(_lib, n, score=score, tally=tally, cdf=cdf, p=p), duel_io(_lib, 0, duel)
    assert L.rx_track_duel_scores_host(ctypes.byref(tc), ctypes.byref(td), power, prior, None) == 0, L.rx_last_error()
    assert cdf[-1] == -7 and p[-1] == -7.0, "the guard element"
    return cdf[:-1], p[:-1]


@pytest.mark.parametrize("power", [0, 1, 4])
@pytest.mark.parametrize("score", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 64, 65, C - 1, C, C + 1])
def test_duel_scores_host_equals_the_restatement(L, n, score, power):
    from rx import _lib
    assert C == _lib.RX_TRACK_SCORES_CHUNK
    tally, duel = make_duel_tally("mixed", n, seed=5 + n)
    cdf, p = _host_scores(L, tally, duel, score, power)
    want_cdf, want_p, W = py_duel_scores(tally, duel, score, power, 1.0)
    assert cdf.tolist() == want_cdf and np.array_equal(p.view(np.uint64), want_p.view(np.uint64))
    assert (cdf >= 0).all() and (np.diff(cdf) >= 0).all()
    if power == 0:
        assert W == [1 << 32] * n
    if score >= 2:  # p is the win rate with the prior
        assert np.array_equal(p, (duel[:, 0] + 1.0) / (tally[:, 0] + 2.0))
    if score <= 1:  # identical bits to rx_track_scores_host on the same tally
        c1, p1 = np.zeros(n, dtype=np.int64), np.zeros(n)
        tc = track_io(_lib, n, score=score, tally=tally, cdf=c1, p=p1)
        assert L.rx_track_scores_host(ctypes.byref(tc), power, 1.0, None) == 0
        assert np.array_equal(c1, cdf) and np.array_equal(p1.view(np.uint64), p.view(np.uint64))
        assert cdf.tolist() == py_scores(tally, score, power, 1.0)[0]


@pytest.mark.parametrize("score", [0, 2])
def test_duel_scores_host_all_zero_weights(L, score):
    tally, duel = make_duel_tally("mastered", 9)
    cdf, p = _host_scores(L, tally, duel, score, 4)
    assert not cdf.any(), "(1/1002)^4 * 2^32 < 1: F == 0"
    assert cdf.tolist() == py_duel_scores(tally, duel, score, 4, 1.0)[0]
    fresh = make_duel_tally("fresh", 9)
    for s in range(4):
        cdf, p = _host_scores(L, *fresh, s, 1)
        assert (p == 0.5).all() and cdf[0] == (1 << 32 if s in (1, 3) else 1 << 31)


# ---- 4: the argument checks -----------------------------------------------------------------------
def test_argument_checks_name_the_field(L):
    from rx import _lib
    n, nt = 8, 3
    buf = dict(track=np.zeros(n, dtype=np.int32), tally=np.zeros((nt, 4), dtype=np.int64),
               cdf=np.zeros(nt, dtype=np.int64), p=np.zeros(nt), track_of_env=np.zeros(n, dtype=np.int32))
    duel = np.zeros((nt, 4), dtype=np.int64)
    done, term, info = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros((n, 2, 4))
    q = _lib.ptr

    def tc(n_tracks=nt, score=0, **over):
        return ctypes.byref(track_io(_lib, n_tracks, score, **{**buf, **over}))

    def td(agent=0, d=duel):
        return ctypes.byref(duel_io(_lib, agent, d))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        Ta, Sc = getattr(L, "rx_track_tally2" + sfx), getattr(L, "rx_track_duel_scores" + sfx)
        rest = (n, q(done), q(term), q(info), None)
        refused(Ta(None, td(), *rest), "null track io")
        refused(Sc(None, td(), 1, 1.0, None), "null track io")
        refused(Ta(tc(), None, *rest), "null track duel io")
        refused(Sc(tc(), None, 1, 1.0, None), "null track duel io")
        for bad in (0, -4):
            refused(Ta(tc(n_tracks=bad), td(), *rest), "n_tracks")
            refused(Sc(tc(n_tracks=bad), td(), 1, 1.0, None), "n_tracks")
        for k in ("track", "tally"):
            refused(Ta(tc(**{k: None}), td(), *rest), k)
        refused(Ta(tc(), td(d=None), *rest), "null duel")
        refused(Sc(tc(), td(d=None), 1, 1.0, None), "null duel")
        for bad in (-1, 2):
            refused(Ta(tc(), td(agent=bad), *rest), "agent")
            refused(Sc(tc(), td(agent=bad), 1, 1.0, None), "agent")
        refused(Ta(tc(), td(), n, None, q(term), q(info), None), "done")
        refused(Ta(tc(), td(), n, q(done), None, q(info), None), "terminated")
        refused(Ta(tc(), td(), n, q(done), q(term), None, None), "info")
        for bad in (0, -3):
            refused(Ta(tc(), td(), bad, q(done), q(term), q(info), None), "n=")
        for k in ("tally", "cdf", "p"):
            refused(Sc(tc(**{k: None}), td(), 1, 1.0, None), f"null {k}")
        for bad in (-1, 4):
            refused(Sc(tc(score=bad), td(), 1, 1.0, None), "score")
        for bad in (-1, 5):
            refused(Sc(tc(), td(), bad, 1.0, None), "power")
        for bad in (0.0, -1.0, float("nan")):
            refused(Sc(tc(), td(), 1, bad, None), "prior")
    # rx_track_scores itself keeps accepting 0 and 1 only
    for bad in (2, 3):
        refused(L.rx_track_scores_host(tc(score=bad), 1, 1.0, None), "score")
    for ok in range(4):
        assert L.rx_track_duel_scores_host(tc(score=ok, track=None, track_of_env=None), td(), 1, 1.0, None) == 0

    R = L.rx_track_duel_rollout_steps
    io, r, sp = _lib.RxIO(), _lib.RxRolloutIO(), _lib.RxSelfplayIO()
    args = (ctypes.byref(io), ctypes.byref(r), ctypes.byref(sp))
    ids = np.zeros(n, dtype=np.int32)
    lg_buf = dict(params=np.zeros(16, np.float32), log_std=np.zeros(2, np.float32), opp_id=ids, draw_count=ids.copy(),
                  tally=np.zeros((1, 3), np.int64), cdf=np.ones(1))

    def lg(agent=0, **over):
        b = {**lg_buf, **over}
        return ctypes.byref(_lib.RxLeagueIO(1, agent, q(b["params"]), q(b["log_std"]), L.rx_ppo_n_params(19),
                                            q(b["opp_id"]), q(b["draw_count"]), q(b["tally"]), q(b["cdf"]), 0, 0))
    assert R(None, None, None, None, None, None, None, 0, None) == _lib.RX_EINVAL
    refused(R(None, *args, None, None, td(), 0, None), "null track io")
    refused(R(None, *args, None, tc(n_tracks=0), td(), 0, None), "n_tracks")
    refused(R(None, *args, None, tc(track=None), td(), 0, None), "track")
    refused(R(None, *args, None, tc(tally=None), td(), 0, None), "tally")
    refused(R(None, *args, None, tc(), None, 0, None), "null track duel io")
    refused(R(None, *args, None, tc(), td(agent=2), 0, None), "agent=2")
    refused(R(None, *args, None, tc(), td(d=None), 0, None), "null duel")
    refused(R(None, *args, lg(opp_id=None), tc(), td(), 0, None), "opp_id")
    refused(R(None, *args, lg(agent=3), tc(), td(), 0, None), "agent=3")
    refused(R(None, *args, None, tc(), td(), 7, None), "precision=7")
    refused(R(None, *args, None, tc(), td(), 0, None), "null handle")  # no handle without a device: the
    refused(R(None, *args, lg(), tc(), td(), 0, None), "null handle")  # handle's own refusals are in the GPU tests


# ---- 5: the Python side's refusals ----------------------------------------------------------------
class _FakeVenv:
    n_agents = 1


def test_duel_curriculum_refuses_a_single_agent_env_and_bad_rules():
    from rx.track_selfplay import DuelTrackCurriculum, check_duel_rules
    with pytest.raises(ValueError, match="two-car"):
        DuelTrackCurriculum(_FakeVenv(), 0, seed=1)
    with pytest.raises(ValueError, match="score"):
        check_duel_rules(1, 0.1, 1.0, "advantage")
    with pytest.raises(ValueError, match="curriculum_power"):
        check_duel_rules(5, 0.1, 1.0, "lose")
    assert check_duel_rules(1, 0.1, 1.0, "contested") == (1, 0.1, 1.0, 3)


@pytest.mark.parametrize("cls", ["SelfPlayCurriculumPPO", "LeagueCurriculumPPO"])
def test_trainers_refuse_before_they_touch_a_device(monkeypatch, cls):
    from rx import dist as rdist
    from rx import track_selfplay
    from rx.configs import self_play_config
    from rx.envs import RacingEnv
    Trainer = getattr(track_selfplay, cls)
    assert Trainer.resamples_tracks is True

    def env_fn(i):
        raise AssertionError("no env may be built")
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        Trainer(env_fn, self_play_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    state = np.random.get_state()
    with pytest.raises(ValueError, match="two-car"):
        Trainer(lambda i: RacingEnv(num_sensors=11), self_play_config(num_envs=64, num_steps=16))
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    for key, bad in (("curriculum_power", 5), ("curriculum_mix", 1.5), ("curriculum_prior", 0.0),
                     ("curriculum_score", "advantage"), ("curriculum_refresh", 1.5)):
        with pytest.raises(ValueError, match=key.replace("curriculum_score", "score")):
            Trainer(env_fn, self_play_config(num_envs=64, num_steps=16, **{key: bad}))


def test_the_parents_keep_their_refusals():
    from rx.league_train import LeagueSelfPlayPPO
    from rx.selfplay import SelfPlayPPO
    assert SelfPlayPPO.resamples_tracks is False and LeagueSelfPlayPPO.resamples_tracks is False
