"""The track curriculum without a GPU: the host twins rx_track_tally_host,
rx_track_scores_host and rx_track_draw_host against a Python restatement of
csrc/rx_curriculum.h written here (bit for bit: the scores are separately rounded
IEEE operations in a fixed order, the weights and every sum are integers), the
pinned layout of rx_track_io, every argument check that runs before a HIP call,
and CurriculumPPO's refusals."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
NEW = ("rx_track_tally", "rx_track_tally_host", "rx_track_scores", "rx_track_scores_host", "rx_track_draw",
       "rx_track_draw_host", "rx_track_rollout_steps")


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the Python restatement (shared with tests/test_curriculum_gpu.py) -----------------------------
def py_tally(tally, track, done, terminated, info):
    """In place, env by env; tally int64 [n_tracks, 4], info [n, 4]."""
    n_tracks = len(tally)
    for e in range(len(done)):
        k = int(track[e])
        if done[e] == 0 or not 0 <= k < n_tracks:
            continue
        progress = np.float64(info[e, 1])
        finished = progress == 1.0
        tally[k, 0] += 1
        tally[k, 1] += int(finished)
        tally[k, 2] += int(terminated[e] != 0 and not finished)
        tally[k, 3] += int(progress * np.float64(1048576.0))  # truncation


def py_scores(tally, score, power, prior):
    """-> (cdf as Python ints, p float64 [n], W as Python ints)."""
    f8 = np.float64
    prior = f8(prior)
    cdf, p, W, c = [], np.zeros(len(tally), dtype=f8), [], 0
    for k in range(len(tally)):
        n, fin = f8(int(tally[k, 0])), f8(int(tally[k, 1]))
        pk = (fin + prior) / (n + f8(2.0) * prior)
        fail = f8(1.0) - pk
        q = (f8(4.0) * pk) * fail if score == 1 else fail
        f = f8(1.0)
        for _ in range(power):
            f = f * q
        w = int(f * f8(4294967296.0))
        c += w
        p[k] = pk
        W.append(w)
        cdf.append(c)
    assert c < 1 << 63
    return cdf, p, W


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_draw(cdf, n, seed, generation, mix):
    """-> (slots int32 [n], whether each draw took the uniform branch)."""
    n_tracks, F = len(cdf), int(cdf[-1])
    out, uniform = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    for e in range(n):
        h1 = splitmix64(seed ^ splitmix64((((generation & 0xFFFFFFFF) << 32) ^ e) & M64))
        h2 = splitmix64(h1)
        u = float(h1 >> 11) * 2.0 ** -53
        if F == 0 or u < mix:
            out[e], uniform[e] = (h2 * n_tracks) >> 64, True
            continue
        r = (h2 * F) >> 64
        lo, hi = 0, n_tracks - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if r < int(cdf[mid]):
                hi = mid
            else:
                lo = mid + 1
        out[e] = lo
    return out, uniform


def track_io(_lib, n_tracks, score=0, track=None, tally=None, cdf=None, p=None, track_of_env=None, seed=0):
    q = _lib.ptr
    return _lib.RxTrackIO(n_tracks, score, q(track), q(tally), q(cdf), q(p), q(track_of_env), seed)


def tally_case(n, n_tracks, seed, mode="random"):
    """Synthetic step buffers -> (track, done, terminated, info): progress values include exact 1.0 and
    0.0, some slots lie outside the table, some envs are finished and terminated at once."""
    rs = np.random.RandomState(seed)
    track = rs.randint(-1, n_tracks + 1, size=n).astype(np.int32)  # -1 and n_tracks: outside
    done = (rs.rand(n) < 0.6).astype(np.float32)
    terminated = (rs.rand(n) < 0.5).astype(np.uint8)
    progress = rs.choice([0.0, 1.0, 0.25, 1.0 - 2.0 ** -53, 0.999999, 1e-7, 0.7312345678], size=n)
    progress = np.where(rs.rand(n) < 0.4, rs.rand(n), progress)
    if mode == "one_slot":  # full contention: every env ended on ONE slot
        track[:] = n_tracks // 2
        done[:] = 1.0
    elif mode == "distinct":  # every lane of a wave on a different slot
        track[:] = np.arange(n) % n_tracks
        done[:] = 1.0
    elif mode == "none":
        done[:] = 0.0
    info = np.zeros((n, 4), dtype=np.float64)
    info[:, 0], info[:, 1], info[:, 2] = rs.rand(n), progress, rs.rand(n)
    return track, done, terminated, info


TALLIES = ("fresh", "mixed", "mastered")


def make_tally(kind, n, seed=5):
    """fresh: no episode yet; mastered: every slot 1,000 episodes all finished (W_k == 0 at power 4, score
    fail, prior 1: F == 0); mixed: random counts with slot 1 such a mastered one."""
    rs = np.random.RandomState(seed)
    t = np.zeros((n, 4), dtype=np.int64)
    if kind == "mastered":
        t[:] = (1000, 1000, 0, 1000 << 20)
    elif kind == "mixed":
        t[:, 0] = rs.randint(0, 50, size=n)
        t[:, 1] = (rs.rand(n) * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
        t[:, 2] = t[:, 0] - t[:, 1]
        t[:, 3] = rs.randint(0, 1 << 30, size=n)
        if n > 2:
            t[1] = (1000, 1000, 0, 1000 << 20)
    return t


# ---- 1-3: the ABI, the layout, the build lists ----------------------------------------------------
def test_abi_is_still_25_and_the_new_symbols_are_exported(L):
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert "#define RX_ABI_VERSION 25" in hdr
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name


def test_rx_track_io_layout_is_pinned():
    from rx import _lib
    T = _lib.RxTrackIO
    assert ctypes.sizeof(T) == 56
    assert T.n_tracks.offset == 0 and T.score.offset == 4 and T.track.offset == 8
    assert T.tally.offset == 16 and T.track_of_env.offset == 40 and T.seed.offset == 48
    assert [f[0] for f in T._fields_] == ["n_tracks", "score", "track", "tally", "cdf", "p", "track_of_env", "seed"]
    # the pinned sizes of the existing structs stay (additive)
    assert ctypes.sizeof(_lib.RxPolicyIO) == 112 and ctypes.sizeof(_lib.RxLeagueIO) == 80
    assert ctypes.sizeof(_lib.RxEvalIO) == 80


def test_sources_are_in_the_build_lists():
    from rx import _build
    assert "rx_curriculum.hip" in _build.SOURCES and "rx_curriculum_host.cpp" in _build.SOURCES
    assert "rx_curriculum_host.cpp" in _build.HOST_ONLY and "rx_curriculum.hip" not in _build.HOST_ONLY
    assert "rx_curriculum.h" in _build.HEADERS
    for f in ("rx_curriculum.hip", "rx_curriculum_host.cpp", "rx_curriculum.h"):
        assert os.path.exists(os.path.join(_build.CSRC, f))


# ---- 4: rx_track_tally_host -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["random", "one_slot", "distinct", "none"])
def test_tally_host_equals_the_restatement(L, mode):
    from rx import _lib
    n, n_tracks = 200, 7
    track, done, terminated, info = tally_case(n, n_tracks, 11, mode)
    if mode == "random":
        ended = done != 0
        assert (track[ended] == -1).any() and (track[ended] == n_tracks).any()
        assert (info[ended, 1] == 1.0).any() and (info[ended, 1] == 0.0).any()
        assert ((info[:, 1] == 1.0) & (terminated != 0) & ended).any(), "finished and terminated at once"
        assert ((info[:, 1] == 1.0) & (terminated == 0) & ended).any(), "finished and truncated at once"
    want = np.random.RandomState(3).randint(0, 9, size=(n_tracks, 4)).astype(np.int64)  # not from zero
    got = want.copy()
    py_tally(want, track, done, terminated, info)
    tc = track_io(_lib, n_tracks, track=track, tally=got)
    q = _lib.ptr
    assert L.rx_track_tally_host(ctypes.byref(tc), n, q(done), q(terminated), q(info), None) == 0, L.rx_last_error()
    assert np.array_equal(got, want)
    if mode == "none":
        assert np.array_equal(got, np.random.RandomState(3).randint(0, 9, size=(n_tracks, 4)))


# ---- 5: rx_track_scores_host ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(TALLIES))
@pytest.mark.parametrize("power", [0, 1, 4])
@pytest.mark.parametrize("score", [0, 1])
def test_scores_host_equals_the_restatement(L, score, power, kind):
    from rx import _lib
    n = 9
    tally = make_tally(kind, n)
    cdf, p = np.full(n, -7, dtype=np.int64), np.full(n, -7.0)
    tc = track_io(_lib, n, score=score, tally=tally, cdf=cdf, p=p)
    assert L.rx_track_scores_host(ctypes.byref(tc), power, 1.0, None) == 0, L.rx_last_error()
    want_cdf, want_p, W = py_scores(tally, score, power, 1.0)
    assert cdf.tolist() == want_cdf and np.array_equal(p, want_p)
    assert (cdf >= 0).all() and (np.diff(cdf) >= 0).all()
    if power == 0:
        assert W == [1 << 32] * n
    if kind == "fresh" and score == 0:
        assert W == [1 << (32 - power)] * n  # p = 0.5 exactly
    if power == 4 and score == 0:
        if kind == "mixed":
            assert W[1] == 0 and cdf[-1] > 0  # (1/1002)^4 * 2^32 < 1
        if kind == "mastered":
            assert W == [0] * n and cdf[-1] == 0  # F == 0


# ---- 6: rx_track_draw_host --------------------------------------------------------------------------
def _host_draw(L, cdf, n, seed, generation, mix):
    from rx import _lib
    cdf = np.ascontiguousarray(cdf, dtype=np.int64)
    out = np.full(n, -5, dtype=np.int32)
    tc = track_io(_lib, len(cdf), cdf=cdf, track_of_env=out, seed=seed)
    assert L.rx_track_draw_host(ctypes.byref(tc), n, generation, mix, None) == 0, L.rx_last_error()
    return out


@pytest.mark.parametrize("mix", [0.0, 0.1, 1.0])
def test_draw_host_equals_the_restatement(L, mix):
    seed, n = 0x1234567890ABCDEF, 500
    cdf, _, W = py_scores(make_tally("mixed", 9), 0, 4, 1.0)
    assert W[1] == 0
    for g in (1, 2, 0xFFFFFFFF):
        want, uniform = py_draw(cdf, n, seed, g, mix)
        got = _host_draw(L, cdf, n, seed, g, mix)
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < 9
        if mix == 0.0:
            assert not uniform.any() and not (got == 1).any(), "a W_k == 0 slot was drawn without the uniform part"
        if mix == 1.0:
            assert uniform.all()
    a, b = _host_draw(L, cdf, n, seed, 1, mix), _host_draw(L, cdf, n, seed, 2, mix)
    assert not np.array_equal(a, b), "a new generation must give a new assignment"
    assert not np.array_equal(a, _host_draw(L, cdf, n, seed + 1, 1, mix))


def test_draw_host_edge_tables(L):
    seed = 77
    zero, _, _ = py_scores(make_tally("mastered", 9), 0, 4, 1.0)
    assert zero[-1] == 0
    want, uniform = py_draw(zero, 300, seed, 3, 0.0)
    assert uniform.all()  # F == 0: every draw is the uniform branch
    got = _host_draw(L, zero, 300, seed, 3, 0.0)
    assert np.array_equal(got, want) and len(set(got.tolist())) == 9
    one, _, _ = py_scores(make_tally("fresh", 1), 0, 1, 1.0)
    for mix in (0.0, 0.5, 1.0):
        assert not _host_draw(L, one, 300, seed, 1, mix).any()  # n_tracks = 1: every id is 0
    # the distribution follows the weights: a slot never finished is drawn more often than a half-solved one
    t = np.zeros((2, 4), dtype=np.int64)
    t[0], t[1] = (98, 0, 98, 0), (98, 49, 49, 0)
    cdf, p, W = py_scores(t, 0, 1, 1.0)
    got = _host_draw(L, cdf, 20000, seed, 1, 0.0)
    share = (got == 0).mean()
    want = W[0] / cdf[-1]  # 0.99 / 1.49
    assert abs(share - want) < 4 * np.sqrt(want * (1 - want) / 20000)


# ---- 7: the argument checks -------------------------------------------------------------------------
def test_argument_checks_name_the_field(L):
    from rx import _lib
    n, nt = 8, 3
    buf = dict(track=np.zeros(n, dtype=np.int32), tally=np.zeros((nt, 4), dtype=np.int64),
               cdf=np.zeros(nt, dtype=np.int64), p=np.zeros(nt), track_of_env=np.zeros(n, dtype=np.int32))
    done, term, info = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros((n, 4))
    q = _lib.ptr

    def tc(n_tracks=nt, score=0, **over):
        return ctypes.byref(track_io(_lib, n_tracks, score, **{**buf, **over}))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        Ta, Sc, Dr = (getattr(L, f"rx_track_{k}{sfx}") for k in ("tally", "scores", "draw"))
        refused(Ta(None, n, q(done), q(term), q(info), None), "null track io")
        refused(Sc(None, 1, 1.0, None), "null track io")
        refused(Dr(None, n, 1, 0.1, None), "null track io")
        for bad in (0, -4):
            refused(Ta(tc(n_tracks=bad), n, q(done), q(term), q(info), None), "n_tracks")
            refused(Sc(tc(n_tracks=bad), 1, 1.0, None), "n_tracks")
            refused(Dr(tc(n_tracks=bad), n, 1, 0.1, None), "n_tracks")
        for k in ("track", "tally"):
            refused(Ta(tc(**{k: None}), n, q(done), q(term), q(info), None), k)
        refused(Ta(tc(), n, None, q(term), q(info), None), "done")
        refused(Ta(tc(), n, q(done), None, q(info), None), "terminated")
        refused(Ta(tc(), n, q(done), q(term), None, None), "info")
        for bad in (0, -3):
            refused(Ta(tc(), bad, q(done), q(term), q(info), None), "n=")
            refused(Dr(tc(), bad, 1, 0.1, None), "n=")
        for k in ("tally", "cdf", "p"):
            refused(Sc(tc(**{k: None}), 1, 1.0, None), f"null {k}")
        for bad in (-1, 2):
            refused(Sc(tc(score=bad), 1, 1.0, None), "score")
        for bad in (-1, 5):
            refused(Sc(tc(), bad, 1.0, None), "power")
        for bad in (0.0, -1.0, float("nan")):
            refused(Sc(tc(), 1, bad, None), "prior")
        for k in ("cdf", "track_of_env"):
            refused(Dr(tc(**{k: None}), n, 1, 0.1, None), k)
        for bad in (-0.01, 1.01, float("nan")):
            refused(Dr(tc(), n, 1, bad, None), "mix")
        # what an entry point does not read may be null
        assert getattr(L, "rx_track_scores_host")(tc(track=None, track_of_env=None), 1, 1.0, None) == 0
        assert getattr(L, "rx_track_draw_host")(tc(track=None, tally=None, p=None), n, 1, 0.1, None) == 0

    R = L.rx_track_rollout_steps
    io, r = _lib.RxIO(), _lib.RxRolloutIO()
    args = (ctypes.byref(io), ctypes.byref(r))
    assert R(None, None, None, None, 0, None) == _lib.RX_EINVAL
    refused(R(None, *args, None, 0, None), "null track io")
    refused(R(None, *args, tc(n_tracks=0), 0, None), "n_tracks")
    refused(R(None, *args, tc(track=None), 0, None), "track")
    refused(R(None, *args, tc(tally=None), 0, None), "tally")
    refused(R(None, *args, tc(), 7, None), "precision=7")
    refused(R(None, *args, tc(), 0, None), "null handle")


# ---- 8: the trainer's refusals ----------------------------------------------------------------------
def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import MultiRacingEnv

    def env_fn(i):
        raise AssertionError("no env may be built")
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        CurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    state = np.random.get_state()
    with pytest.raises(ValueError, match="two-car"):
        CurriculumPPO(lambda i: MultiRacingEnv(num_agents=2, num_sensors=11), base_config(num_envs=64, num_steps=16))
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    for key, bad in (("curriculum_power", 5), ("curriculum_mix", 1.5), ("curriculum_prior", 0.0),
                     ("curriculum_score", "advantage"), ("curriculum_refresh", 1.5)):
        with pytest.raises(ValueError, match=key.replace("curriculum_score", "score")):
            CurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, **{key: bad}))
