"""The curriculum's replay scores without a GPU: the host twins
rx_track_learn_tally_host, _fold_host, _tables_host and _draw_host against a Python
restatement of csrc/rx_track_replay.h written here (bit for bit: float64 with
separately rounded operations in a fixed order, integer sums), the pinned layout of
rx_track_learn_io, every argument check that runs before a HIP call, and
ReplayCurriculumPPO's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_curriculum_cpu import M64, make_tally, py_scores, splitmix64, track_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = tuple(f"rx_track_learn_{k}{sfx}" for k in ("tally", "fold", "tables", "draw") for sfx in ("", "_host"))
FIELDS = ["n_tracks", "kind", "track", "learn", "score", "seen", "rank", "cdf_score", "cdf_stale", "track_of_env",
          "seed"]
f4, f8 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the Python restatement (shared with tests/test_track_replay_gpu.py) ---------------------------
def py_learn_tally(learn, track, adv, kind):
    """In place, value by value; learn: a list of [samples, mag_q] Python ints, adv float32 [T, n]."""
    T, n = adv.shape
    for t in range(T):
        for e in range(n):
            k, a = int(track[e]), adv[t, e]
            if not 0 <= k < len(learn) or not np.isfinite(a):
                continue
            m = abs(a) if kind == 0 else max(a, f4(0.0))
            m = min(f4(m), f4(1048576.0))
            learn[k][0] += 1
            learn[k][1] += int(f8(m) * f8(1048576.0))  # truncation


def py_fold(learn, score, seen, update, alpha):
    """In place; score float64 [n], seen int32 [n]."""
    alpha = f8(alpha)
    for k in range(len(learn)):
        samples, mag_q = learn[k]
        if samples <= 0:
            continue
        mean = (f8(mag_q) / f8(1048576.0)) / f8(samples)
        score[k] = mean if seen[k] < 0 else score[k] + alpha * (mean - score[k])
        seen[k] = update
        learn[k][0] = learn[k][1] = 0


def py_rank(score, seen):
    key = np.where(seen < 0, np.inf, score)
    order = np.lexsort((np.arange(len(key)), -key))  # the key descending, ties by slot
    rank = np.zeros(len(key), dtype=np.int32)
    rank[order] = np.arange(1, len(key) + 1)
    return rank


def py_tables(rank, seen, power, now):
    """-> (cdf_score, cdf_stale, W) as Python ints."""
    cs, ct, W, a, b = [], [], [], 0, 0
    for k in range(len(rank)):
        h = f8(1.0) / f8(int(rank[k]))
        f = f8(1.0)
        for _ in range(power):
            f = f * h
        w = int(f * f8(4294967296.0))
        a += w
        b += 0 if seen[k] < 0 else max(int(now) - int(seen[k]), 0)
        W.append(w)
        cs.append(a)
        ct.append(b)
    assert a < 1 << 63 and b < 1 << 63
    return cs, ct, W


def _search(cdf, r):
    lo, hi = 0, len(cdf) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if r < int(cdf[mid]):
            hi = mid
        else:
            lo = mid + 1
    return lo


def py_learn_draw(cdf_score, cdf_stale, n, seed, generation, mix, stale_mix):
    """-> (slots int32 [n], the branch of each draw: 0 uniform, 1 staleness, 2 score)."""
    n_tracks, F, Fs = len(cdf_score), int(cdf_score[-1]), int(cdf_stale[-1])
    out, branch = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int8)
    for e in range(n):
        h1 = splitmix64(seed ^ splitmix64((((generation & 0xFFFFFFFF) << 32) ^ e) & M64))
        h2 = splitmix64(h1)
        u = float(h1 >> 11) * 2.0 ** -53
        if u < mix:
            out[e] = (h2 * n_tracks) >> 64
        elif u < mix + stale_mix and Fs > 0:
            out[e], branch[e] = _search(cdf_stale, (h2 * Fs) >> 64), 1
        elif F == 0:
            out[e] = (h2 * n_tracks) >> 64
        else:
            out[e], branch[e] = _search(cdf_score, (h2 * F) >> 64), 2
    return out, branch


def learn_io(_lib, n_tracks, kind=0, seed=0, **arrays):
    assert set(arrays) <= set(_lib.TRACK_LEARN_FIELDS)
    return _lib.RxTrackLearnIO(n_tracks, kind, *(_lib.ptr(arrays.get(k)) for k in _lib.TRACK_LEARN_FIELDS), seed)


SPECIAL = np.array([-2.5, 0.0, -0.0, 1e-45, -1e-40, 1.1754942e-38, 1e9, -1e9, 1048576.0, 1048577.0, np.nan, np.inf,
                    -np.inf, 0.7312345, -3.4028235e38, 2.0 ** -21, 2.0 ** -20, 1.0 - 2.0 ** -24], dtype=np.float32)


def adv_case(T, n, n_tracks, seed, mode="random"):
    """-> (track int32 [n], adv float32 [T, n]): advantages with negatives, zeros, subnormals, values past
    the clamp, NaN and both infinities; slots -1 and n_tracks lie outside the table."""
    rs = np.random.RandomState(seed)
    track = rs.randint(-1, n_tracks + 1, size=n).astype(np.int32)
    adv = (rs.standard_normal((T, n)) * 3.0).astype(np.float32)
    pick = rs.rand(T, n) < 0.3
    adv[pick] = rs.choice(SPECIAL, size=int(pick.sum()))
    if mode == "one_slot":  # full contention: every env on ONE slot
        track[:] = n_tracks // 2
    elif mode == "distinct":  # every lane of a wave on a different slot
        track[:] = np.arange(n) % n_tracks
    elif mode == "none":  # every env outside the table
        track[:] = np.where(np.arange(n) % 2 == 0, -1, n_tracks)
    return track, adv


SCORES = ("equal", "three", "mixed", "unseen")


def score_case(kind, n, seed=7, now=9):
    """-> (score float64 [n], seen int32 [n]).  equal: every score the same; three: three distinct values
    (ties everywhere); mixed: ties, zeros and never-scored slots; unseen: no slot scored yet."""
    rs = np.random.RandomState(seed + n)
    seen = rs.randint(0, now + 1, size=n).astype(np.int32)
    if kind == "equal":
        score = np.full(n, 0.375)
    elif kind == "three":
        score = rs.choice([0.0, 0.25, 1.5], size=n)
    elif kind == "mixed":
        score = np.where(rs.rand(n) < 0.5, rs.choice([0.0, 0.125, 2.0, 1048576.0], size=n), rs.rand(n))
        seen[rs.rand(n) < 0.3] = -1
    else:
        score, seen[:] = rs.rand(n), -1
    return np.ascontiguousarray(score, dtype=np.float64), seen


def host_tables(L, score, seen, power, now):
    """rx_track_learn_tables_host -> (rank, cdf_score, cdf_stale), each with a guard element."""
    from rx import _lib
    n = len(score)
    rank = np.full(n + 1, -7, dtype=np.int32)
    cs, ct = np.full(n + 1, -7, dtype=np.int64), np.full(n + 1, -7, dtype=np.int64)
    lt = learn_io(_lib, n, score=score, seen=seen, rank=rank, cdf_score=cs, cdf_stale=ct)
    assert L.rx_track_learn_tables_host(ctypes.byref(lt), power, now, None) == 0, L.rx_last_error()
    assert rank[n] == -7 and cs[n] == -7 and ct[n] == -7
    return rank[:n], cs[:n], ct[:n]


def host_draw(L, cdf_score, cdf_stale, n, seed, generation, mix, stale_mix):
    from rx import _lib
    cs = np.ascontiguousarray(cdf_score, dtype=np.int64)
    ct = np.ascontiguousarray(cdf_stale, dtype=np.int64)
    out = np.full(n + 1, -5, dtype=np.int32)
    lt = learn_io(_lib, len(cs), seed=seed, cdf_score=cs, cdf_stale=ct, track_of_env=out)
    assert L.rx_track_learn_draw_host(ctypes.byref(lt), n, generation, mix, stale_mix, None) == 0, L.rx_last_error()
    assert out[n] == -5
    return out[:n]


# ---- 1: the ABI, the layout, the build lists ------------------------------------------------------
def test_abi_is_still_25_and_the_new_symbols_are_exported(L):
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert "#define RX_ABI_VERSION 25" in hdr
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name


def test_rx_track_learn_io_layout_matches_the_header():
    from rx import _lib
    T = _lib.RxTrackLearnIO
    assert [f[0] for f in T._fields_] == FIELDS
    assert ctypes.sizeof(T) == 80
    assert [getattr(T, k).offset for k in FIELDS] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    body = re.search(r"typedef struct rx_track_learn_io \{(.*?)\} rx_track_learn_io;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert [re.search(r"(\w+)$", d).group(1) for d in decl] == FIELDS
    kinds = ["*" if "*" in d else d.split()[0] for d in decl]
    assert kinds == ["int32_t", "int32_t"] + ["*"] * 8 + ["uint64_t"]
    # the pinned layouts beside it stay (additive)
    assert ctypes.sizeof(_lib.RxTrackIO) == 56 and _lib.TRACK_SCORES == {"fail": 0, "potential": 1}
    assert _lib.RX_TRACK_MAX_POWER == 4


def test_sources_are_in_the_build_lists():
    from rx import _build
    assert "rx_track_replay.hip" in _build.SOURCES and "rx_track_replay_host.cpp" in _build.SOURCES
    assert "rx_track_replay_host.cpp" in _build.HOST_ONLY and "rx_track_replay.hip" not in _build.HOST_ONLY
    assert "rx_track_replay.h" in _build.HEADERS
    for f in ("rx_track_replay.hip", "rx_track_replay_host.cpp", "rx_track_replay.h"):
        assert os.path.exists(os.path.join(_build.CSRC, f))


# ---- 2: rx_track_learn_tally_host -------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("mode", ["random", "one_slot", "distinct", "none"])
def test_tally_host_equals_the_restatement(L, mode, kind):
    from rx import _lib
    T, n, n_tracks = 6, 90, 7
    track, adv = adv_case(T, n, n_tracks, 11, mode)
    if mode == "random":
        assert (track == -1).any() and (track == n_tracks).any()
        inside = adv[:, (track >= 0) & (track < n_tracks)]
        assert np.isnan(inside).any() and (inside == np.inf).any() and (inside == -np.inf).any()
        assert (inside < 0).any() and (inside == 0).any() and (inside >= 1e9).any()
        assert ((inside != 0) & (np.abs(inside) < 1.1754944e-38)).any(), "subnormals"
    start = np.random.RandomState(3).randint(0, 9, size=(n_tracks + 1, 2)).astype(np.int64)  # not from zero
    want = [[int(a), int(b)] for a, b in start[:n_tracks]]
    py_learn_tally(want, track, adv, kind)
    got = start.copy()
    lt = learn_io(_lib, n_tracks, kind, track=track, learn=got)
    assert L.rx_track_learn_tally_host(ctypes.byref(lt), T, n, _lib.ptr(adv), None) == 0, L.rx_last_error()
    assert got[:n_tracks].tolist() == want and np.array_equal(got[n_tracks], start[n_tracks])
    if mode == "none":
        assert np.array_equal(got, start)
    if mode == "one_slot":
        k = n_tracks // 2
        assert got[k, 0] - start[k, 0] == int(np.isfinite(adv).sum())
        assert np.array_equal(np.delete(got, k, 0), np.delete(start, k, 0))


def test_tally_host_clamps_and_truncates(L):
    from rx import _lib
    adv = np.array([[1e9, -1e9, 1048576.0, 0.5, -0.5, 2.0 ** -21, 1e-45, np.nan]], dtype=np.float32)
    track = np.zeros(8, dtype=np.int32)
    for kind, want in ((0, [7, (3 << 40) + (1 << 20)]), (1, [7, (2 << 40) + (1 << 19)])):
        learn = np.zeros((1, 2), dtype=np.int64)
        lt = learn_io(_lib, 1, kind, track=track, learn=learn)
        assert L.rx_track_learn_tally_host(ctypes.byref(lt), 1, 8, _lib.ptr(adv), None) == 0
        assert learn[0].tolist() == want  # 2^-21 * 2^20 truncates to 0


# ---- 3: rx_track_learn_fold_host --------------------------------------------------------------------
def test_fold_host_equals_the_restatement(L):
    from rx import _lib
    # slot 0 never seen; 1 seen (alpha 1 replaces, alpha 0.5 averages); 2 without samples; 3 seen, zero magnitude
    for alpha in (1.0, 0.5, 0.3):
        learn = np.array([[3, 7 << 18], [5, 123456789], [0, 0], [4, 0], [0, 0]], dtype=np.int64)
        score = np.array([99.0, 0.7, 0.3, 2.5, -8.0])
        seen = np.array([-1, 2, 1, 0, -1], dtype=np.int32)
        py_l, py_s, py_n = learn[:4].tolist(), score.copy(), seen.copy()
        py_fold(py_l, py_s[:4], py_n[:4], 6, alpha)
        lt = learn_io(_lib, 4, learn=learn, score=score, seen=seen)
        assert L.rx_track_learn_fold_host(ctypes.byref(lt), 6, alpha, None) == 0, L.rx_last_error()
        assert np.array_equal(score, py_s) and np.array_equal(seen, py_n)
        assert not learn.any(), "the learn rows start again"
        assert seen.tolist() == [6, 6, 1, 6, -1] and score[2] == 0.3 and score[4] == -8.0
        assert score[0] == (7 << 18) / 1048576.0 / 3
        if alpha == 1.0:
            assert score[3] == 0.0
        if alpha == 0.5:
            assert score[3] == 1.25


# ---- 4: rank and tables -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SCORES))
@pytest.mark.parametrize("power", [0, 1, 4, 10])
def test_tables_host_equals_the_restatement(L, power, kind):
    n, now = 37, 9
    score, seen = score_case(kind, n, now=now)
    rank, cs, ct = host_tables(L, score, seen, power, now)
    want_rank = py_rank(score, seen)
    assert np.array_equal(rank, want_rank)
    assert sorted(rank.tolist()) == list(range(1, n + 1)), "the ranks are a permutation of 1..n"
    want_cs, want_ct, W = py_tables(want_rank, seen, power, now)
    assert cs.tolist() == want_cs and ct.tolist() == want_ct
    if power == 0:
        assert W == [1 << 32] * n
    if power == 1:
        assert W[int(np.argmin(rank))] == 1 << 32 and W[int(np.argmax(rank))] == int(f8(1.0) / f8(n) * f8(2.0 ** 32))
    if kind == "equal":
        assert rank.tolist() == list(range(1, n + 1))  # ties by slot
    if kind == "unseen":
        assert rank.tolist() == list(range(1, n + 1)) and ct[-1] == 0
    if kind == "mixed":
        unseen = seen < 0
        assert unseen.any() and not unseen.all() and rank[unseen].max() == unseen.sum(), "never scored: first"
    if kind == "three":
        assert (np.diff(score[np.argsort(rank)]) <= 0).all()


def test_stale_table_is_zero_when_every_slot_was_just_seen(L):
    score, seen = score_case("three", 12)
    seen[:] = 5
    _, cs, ct = host_tables(L, score, seen, 4, 5)
    assert not ct.any() and cs[-1] > 0
    _, _, ct = host_tables(L, score, seen, 4, 8)
    assert ct.tolist() == [3 * (k + 1) for k in range(12)]


# ---- 5: rx_track_learn_draw_host --------------------------------------------------------------------
@pytest.mark.parametrize("mix", [0.0, 0.1, 1.0])
def test_draw_host_without_staleness_is_rx_track_draw(L, mix):
    """On a table rx_track_scores_host produced: bit for bit rx_track_draw_host's assignment."""
    from rx import _lib
    n, n_tracks, seed = 4097, 9, 0x1234567890ABCDEF
    for kind, power in (("mixed", 4), ("mastered", 4), ("fresh", 1)):
        tally = make_tally(kind, n_tracks)
        cdf, p = np.zeros(n_tracks, dtype=np.int64), np.zeros(n_tracks)
        tc = track_io(_lib, n_tracks, tally=tally, cdf=cdf, p=p)
        assert L.rx_track_scores_host(ctypes.byref(tc), power, 1.0, None) == 0
        assert cdf.tolist() == py_scores(tally, 0, power, 1.0)[0] and (kind != "mastered" or cdf[-1] == 0)
        for g in (1, 0xFFFFFFFF):
            want = np.zeros(n, dtype=np.int32)
            td = track_io(_lib, n_tracks, cdf=cdf, track_of_env=want, seed=seed)
            assert L.rx_track_draw_host(ctypes.byref(td), n, g, mix, None) == 0
            stale = np.arange(1, n_tracks + 1, dtype=np.int64)  # present, never reached
            assert np.array_equal(host_draw(L, cdf, stale, n, seed, g, mix, 0.0), want)
    # and with no staleness table at all
    out = np.zeros(n, dtype=np.int32)
    lt = learn_io(_lib, n_tracks, seed=seed, cdf_score=cdf, track_of_env=out)
    assert L.rx_track_learn_draw_host(ctypes.byref(lt), n, 0xFFFFFFFF, mix, 0.0, None) == 0
    assert np.array_equal(out, want)


@pytest.mark.parametrize("mixes", [(0.0, 0.0), (0.1, 0.1), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7)])
def test_draw_host_equals_the_restatement(L, mixes):
    mix, stale_mix = mixes
    n, n_tracks, seed, now = 600, 37, 0xC0FFEE, 9
    for kind in ("mixed", "three"):
        score, seen = score_case(kind, n_tracks, now=now)
        if kind == "three":
            seen[:] = now  # F_stale == 0: the staleness part falls through to the scores
        _, cs, ct = host_tables(L, score, seen, 4, now)
        assert (ct[-1] == 0) == (kind == "three")
        for g in (1, 2):
            want, branch = py_learn_draw(cs, ct, n, seed, g, mix, stale_mix)
            got = host_draw(L, cs, ct, n, seed, g, mix, stale_mix)
            assert np.array_equal(got, want) and got.min() >= 0 and got.max() < n_tracks
            if kind == "three":
                assert not (branch == 1).any()
            elif stale_mix == 1.0:
                assert (branch == 1).all()
            elif (mix, stale_mix) == (0.1, 0.1):
                assert {0, 1, 2} == set(branch.tolist())
            if mix == 1.0:
                assert (branch == 0).all()
    assert not np.array_equal(host_draw(L, cs, ct, n, seed, 1, mix, stale_mix),
                              host_draw(L, cs, ct, n, seed, 2, mix, stale_mix))


def test_draw_host_is_exact(L):
    # staleness only, exactly one stale slot: every env lands on it
    n_tracks, now = 11, 20
    score = np.linspace(0.1, 1.0, n_tracks)
    seen = np.full(n_tracks, now, dtype=np.int32)
    seen[6] = now - 3
    _, cs, ct = host_tables(L, score, seen, 4, now)
    assert ct[-1] == 3
    assert (host_draw(L, cs, ct, 5000, 5, 1, 0.0, 1.0) == 6).all()
    # rank only at power 10: the share of the rank-1 slot follows W_1 / F
    n, n_tracks = 65536, 64
    score, seen = score_case("mixed", n_tracks)
    seen[seen < 0] = 0
    score[17] = 5e6
    rank, cs, ct = host_tables(L, score, seen, 10, now)
    assert rank[17] == 1
    W1, F = int(cs[17] - cs[16]), int(cs[-1])
    assert W1 == 1 << 32
    p = W1 / F
    got = host_draw(L, cs, ct, n, 77, 1, 0.0, 0.0)
    assert abs((got == 17).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n)
    assert (got != 17).any()


# ---- 6: the argument checks -------------------------------------------------------------------------
def test_argument_checks_name_the_field(L):
    from rx import _lib
    T, n, nt = 3, 8, 3
    buf = dict(track=np.zeros(n, dtype=np.int32), learn=np.zeros((nt, 2), dtype=np.int64), score=np.zeros(nt),
               seen=np.zeros(nt, dtype=np.int32), rank=np.zeros(nt, dtype=np.int32),
               cdf_score=np.zeros(nt, dtype=np.int64), cdf_stale=np.zeros(nt, dtype=np.int64),
               track_of_env=np.zeros(n, dtype=np.int32))
    adv_rows = np.zeros((T, n), dtype=np.float32)
    adv, nan = _lib.ptr(adv_rows), float("nan")

    def lt(n_tracks=nt, kind=0, **over):
        return ctypes.byref(learn_io(_lib, n_tracks, kind, **{**buf, **over}))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        Ta, Fo, Tb, Dr = (getattr(L, f"rx_track_learn_{k}{sfx}") for k in ("tally", "fold", "tables", "draw"))
        calls = ((Ta, (T, n, adv, None), ("track", "learn")), (Fo, (1, 1.0, None), ("learn", "score", "seen")),
                 (Tb, (4, 1, None), ("score", "seen", "rank", "cdf_score", "cdf_stale")),
                 (Dr, (n, 1, 0.1, 0.1, None), ("cdf_score", "cdf_stale", "track_of_env")))
        for fn, rest, reads in calls:
            refused(fn(None, *rest), "null track learn io")
            for bad in (0, -4):
                refused(fn(lt(n_tracks=bad), *rest), "n_tracks")
            for k in reads:
                refused(fn(lt(**{k: None}), *rest), f"null {k}")
        refused(Ta(lt(), T, n, None, None), "null adv")
        for bad in (-1, 2):
            refused(Ta(lt(kind=bad), T, n, adv, None), "kind")
        for bad in (0, -3):
            refused(Ta(lt(), bad, n, adv, None), "T=")
            refused(Ta(lt(), T, bad, adv, None), "n=")
            refused(Dr(lt(), bad, 1, 0.1, 0.1, None), "n=")
        for bad in (0.0, -0.5, 1.5, nan):
            refused(Fo(lt(), 1, bad, None), "alpha")
        for bad in (-1, 11):
            refused(Tb(lt(), bad, 1, None), "power")
        refused(Tb(lt(), 4, -1, None), "now")
        for bad in (-0.01, 1.01, nan):
            refused(Dr(lt(), n, 1, bad, 0.0, None), "mix=")
            refused(Dr(lt(), n, 1, 0.0, bad, None), "stale_mix=")
        refused(Dr(lt(), n, 1, 0.6, 0.5, None), "mix + stale_mix")
    # what an entry point does not read may be null
    only = lambda *keep: lt(**{k: None for k in buf if k not in keep})  # noqa: E731
    assert L.rx_track_learn_tally_host(only("track", "learn"), T, n, adv, None) == 0
    assert L.rx_track_learn_fold_host(only("learn", "score", "seen"), 1, 1.0, None) == 0
    assert L.rx_track_learn_tables_host(only("score", "seen", "rank", "cdf_score", "cdf_stale"), 10, 0, None) == 0
    assert L.rx_track_learn_draw_host(only("cdf_score", "cdf_stale", "track_of_env"), n, 1, 0.5, 0.5, None) == 0
    assert L.rx_track_learn_draw_host(only("cdf_score", "track_of_env"), n, 1, 1.0, 0.0, None) == 0


# ---- 7: the trainer's refusals ----------------------------------------------------------------------
def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import base_config
    from rx.envs import MultiRacingEnv
    from rx.track_replay import ReplayCurriculumPPO

    def env_fn(i):
        raise AssertionError("no env may be built")
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        ReplayCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    state = np.random.get_state()
    with pytest.raises(ValueError, match="two-car"):
        ReplayCurriculumPPO(lambda i: MultiRacingEnv(num_agents=2, num_sensors=11),
                            base_config(num_envs=64, num_steps=16))
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    bad_keys = (("replay_kind", "advantage"), ("replay_kind", 0), ("replay_power", 11), ("replay_power", -1),
                ("replay_alpha", 0.0), ("replay_alpha", 1.5), ("replay_stale_mix", -0.1), ("replay_stale_mix", 1.5),
                ("curriculum_mix", 1.5), ("curriculum_power", 5), ("curriculum_prior", 0.0),
                ("curriculum_refresh", 1.5))
    for key, bad in bad_keys:
        with pytest.raises(ValueError, match=key):
            ReplayCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, **{key: bad}))
    with pytest.raises(ValueError, match="score"):  # CurriculumPPO's own scores stay the two it has
        ReplayCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, curriculum_score="advantage"))
    with pytest.raises(ValueError, match="curriculum_mix \\+ replay_stale_mix"):
        ReplayCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, curriculum_mix=0.6, replay_stale_mix=0.5))
