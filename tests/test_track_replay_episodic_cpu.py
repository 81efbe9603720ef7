"""The replay scores on episodic draws without a GPU: the host twins
rx_track_learn_tally_slots_host and rx_track_learn_episode_host against restatements of
csrc/rx_track_replay.h written here (integers throughout, so bit for bit), the two
reductions to the calls they extend (rx_track_learn_tally_host with constant slots,
rx_track_episode_host with the shared table), every argument check that needs no handle,
and EpisodicReplayCurriculumPPO's refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_curriculum_cpu import M64, py_tally, splitmix64, tally_case, track_io
from tests.test_track_episodic_cpu import SALT, SKEWED, episode_io, host_episode
from tests.test_track_replay_cpu import SPECIAL, _search, learn_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rx_track_learn_tally_slots", "rx_track_learn_tally_slots_host", "rx_track_learn_episode",
       "rx_track_learn_episode_host", "rx_track_learn_episode_step", "rx_track_learn_episodic_rollout_steps")
TS, NS, TRACKS = (1, 31, 32, 33, 70), (1, 63, 64, 65), (1, 7, 300)
PATTERNS = ("constant", "every_row", "edge", "one_slot", "outside")
STALE = [0, 3, 3, 3, 3, 3, 4]  # cdf_stale beside SKEWED: only slots 1 and 6 are stale (4 stays out of reach)
f4, f8 = np.float32, np.float64


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the restatements (shared with tests/test_track_replay_episodic_gpu.py) --------------------------
def slots_case(T, n, n_tracks, pattern, seed):
    """-> (adv float32 [T, n], slots int32 [T, n], dones float32 [T, n]).  adv: adv_case's values (NaN,
    both infinities, zeros, negatives, subnormals, values past the clamp at 1048576).  slots: constant per
    column; a change every row; one change per column at row 31, 32 or 33 (the chunk edge); all on one
    slot; random with -1 and n_tracks among them.  dones: ones in about one element in ten."""
    rs = np.random.RandomState(seed)
    adv = (rs.standard_normal((T, n)) * 3.0).astype(f4)
    pick = rs.rand(T, n) < 0.3
    adv[pick] = rs.choice(SPECIAL, size=int(pick.sum()))
    a, b = rs.randint(0, n_tracks, size=n), rs.randint(0, n_tracks, size=n)
    t, e = np.arange(T)[:, None], np.arange(n)[None, :]
    if pattern == "constant":
        slots = np.broadcast_to(a, (T, n))
    elif pattern == "every_row":
        slots = (a[None, :] + t) % n_tracks
    elif pattern == "edge":
        slots = np.where(t < 31 + e % 3, a[None, :], b[None, :])
    elif pattern == "one_slot":
        slots = np.full((T, n), n_tracks // 2)
    else:
        slots = rs.randint(0, n_tracks, size=(T, n))
        out = rs.rand(T, n) < 0.15
        slots[out] = rs.choice([-1, n_tracks], size=int(out.sum()))
    dones = (rs.rand(T, n) < 0.1).astype(f4)
    return adv, np.ascontiguousarray(slots, dtype=np.int32), dones


def py_tally_slots(learn, adv, slots, dones, kind):
    """In place on learn int64 [n_tracks, 2], whole arrays at a time -> the exclusion masks
    (not finite, outside the table, autoreset row) and the counted mask."""
    n_tracks = len(learn)
    finite = np.isfinite(adv)
    inside = (slots >= 0) & (slots < n_tracks)
    open_ = np.ones(adv.shape, dtype=bool) if dones is None else dones == 0
    counted = finite & inside & open_
    a = np.where(finite, adv, f4(0.0)).astype(f4)
    m = np.abs(a) if kind == 0 else np.maximum(a, f4(0.0))
    m = np.minimum(m, f4(1048576.0)).astype(f4)
    q = (m.astype(f8) * f8(1048576.0)).astype(np.int64)  # truncation of a value >= 0
    np.add.at(learn[:, 0], slots[counted], 1)
    np.add.at(learn[:, 1], slots[counted], q[counted])
    return ~finite, ~inside, ~open_, counted


def host_tally_slots(L, n_tracks, kind, learn, adv, slots, dones, fn="rx_track_learn_tally_slots_host", stream=None):
    from rx import _lib
    lt = learn_io(_lib, n_tracks, kind, learn=learn)  # track stays null: it is not read
    T, n = adv.shape
    rc = getattr(L, fn)(ctypes.byref(lt), T, n, _lib.ptr(adv), _lib.ptr(slots), _lib.ptr(dones), stream)
    assert rc == 0, L.rx_last_error()


def py_learn_draw_one(cdf_score, cdf_stale, seed, g, e, mix, stale_mix):
    """rx_tl_draw for one (generation, env) key -> (slot, branch: 0 uniform, 1 staleness, 2 score)."""
    n_tracks, F = len(cdf_score), int(cdf_score[-1])
    h1 = splitmix64(seed ^ splitmix64((((g & 0xFFFFFFFF) << 32) ^ e) & M64))
    h2 = splitmix64(h1)
    u = float(h1 >> 11) * 2.0 ** -53
    if u < mix:
        return (h2 * n_tracks) >> 64, 0
    if u < mix + stale_mix:
        Fs = int(cdf_stale[-1])
        if Fs > 0:
            return _search(cdf_stale, (h2 * Fs) >> 64), 1
    if F == 0:
        return (h2 * n_tracks) >> 64, 0
    return _search(cdf_score, (h2 * F) >> 64), 2


def py_learn_episode(tally, track, draws, cdf_score, cdf_stale, seed, mix, stale_mix, done, terminated, info,
                     env_pos=None, pos_slot=None):
    """In place: tally, track, draws, pos_slot.  -> (slot_out, the branches taken)."""
    n, n_tracks = len(done), len(tally)
    slot_out = np.array(track[:n], dtype=np.int32)
    old = slot_out.copy()
    py_tally(tally, old, done, terminated, info)  # on the slots the envs ran
    branches = []
    for e in range(n):
        k = int(old[e])
        if done[e] == 0 or not 0 <= k < n_tracks:
            continue
        g = int(draws[e])
        new, br = py_learn_draw_one(cdf_score, cdf_stale, seed ^ SALT, g, e, mix, stale_mix)
        branches.append(br)
        draws[e] = (g + 1) & 0xFFFFFFFF
        track[e] = new
        if env_pos is not None:
            pos_slot[env_pos[e]] = new
    return slot_out, branches


def host_learn_episode(L, n_tracks, tally, track, draws, cdf_score, cdf_stale, seed, mix, stale_mix, done,
                       terminated, info, env_pos=None, pos_slot=None, slot_out=None,
                       fn="rx_track_learn_episode_host", stream=None):
    """One call of the twin (or, with device tensors and a stream, of the kernel) on the caller's arrays."""
    from rx import _lib
    q = _lib.ptr
    tc = track_io(_lib, n_tracks, track=track, tally=tally, seed=seed ^ 0x5555)  # tc->seed and cdf are not read
    lt = learn_io(_lib, n_tracks, seed=seed, cdf_score=cdf_score, cdf_stale=cdf_stale)
    ep = episode_io(_lib, draws, env_pos, pos_slot, slot_out, mix)
    rc = getattr(L, fn)(ctypes.byref(tc), ctypes.byref(lt), ctypes.byref(ep), stale_mix, len(done), q(done),
                        q(terminated), q(info), stream)
    assert rc == 0, L.rx_last_error()


# ---- 1: exports --------------------------------------------------------------------------------------
def test_the_six_exports_exist_and_the_abi_stays_25(L):
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert "#define RX_ABI_VERSION 25" in hdr
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name
    assert ctypes.sizeof(_lib.RxTrackLearnIO) == 80 and ctypes.sizeof(_lib.RxTrackEpisodeIO) == 40  # additive


# ---- 2: the tally by per-step slot -------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n_tracks", TRACKS)
def test_tally_slots_host_equals_the_restatement(L, n_tracks, kind):
    """Every T x n x pattern, with dones null and with the mask.  Over the cases of one parameter pair:
    each exclusion reason occurs, and at least half of the elements are counted."""
    total = counted_all = 0
    reasons = np.zeros(3, dtype=np.int64)
    for T in TS:
        for n in NS:
            for p, pattern in enumerate(PATTERNS):
                adv, slots, mask = slots_case(T, n, n_tracks, pattern, 1000 * T + 10 * n + p)
                for dones in (None, mask):
                    start = np.random.RandomState(T + n).randint(0, 9, size=(n_tracks + 1, 2)).astype(np.int64)
                    want, got = start.copy(), start.copy()
                    nf, out, auto, counted = py_tally_slots(want[:n_tracks], adv, slots, dones, kind)
                    host_tally_slots(L, n_tracks, kind, got, adv, slots, dones)
                    assert np.array_equal(got, want), (T, n, pattern, dones is not None)
                    assert got[:n_tracks, 0].sum() - start[:n_tracks, 0].sum() == counted.sum()
                    total += counted.size
                    counted_all += int(counted.sum())
                    reasons += (nf.sum(), out.sum(), auto.sum())
                    if pattern == "edge" and T > 33 and n_tracks > 1:
                        assert (slots[30] != slots[33]).any() and (slots[31] != slots[30]).any()
                    if pattern == "every_row" and T > 1 and n_tracks > 1:
                        assert (slots[1:] != slots[:-1]).all()
    assert (reasons > 0).all(), reasons
    assert 2 * counted_all >= total, (counted_all, total)


def test_tally_slots_host_special_values(L):
    """The magnitudes of rx_track_learn_tally (clamp at 1048576, truncation), row by row on two slots; a
    done row, a slot outside and a NaN are left out."""
    adv = np.array([[1e9], [-1e9], [1048577.0], [0.5], [-0.5], [2.0 ** -21], [np.nan], [3.0], [5.0], [-np.inf]], f4)
    slots = np.array([[0], [1], [0], [1], [0], [1], [0], [2], [0], [1]], dtype=np.int32)
    dones = np.zeros((10, 1), dtype=f4)
    dones[8] = 1.0
    for kind, want in ((0, [[3, (2 << 40) + (1 << 19)], [3, (1 << 40) + (1 << 19)]]), (1, [[3, 2 << 40], [3, 1 << 19]])):
        learn = np.zeros((2, 2), dtype=np.int64)
        host_tally_slots(L, 2, kind, learn, adv, slots, dones)
        assert learn.tolist() == want, kind


@pytest.mark.parametrize("kind", [0, 1])
def test_constant_slots_and_null_dones_equal_rx_track_learn_tally(L, kind):
    from rx import _lib
    from tests.test_track_replay_cpu import adv_case
    for T, n, n_tracks in ((70, 65, 7), (33, 64, 300), (6, 90, 1)):
        track, adv = adv_case(T, n, n_tracks, 11)  # slots -1 and n_tracks among the columns
        start = np.random.RandomState(3).randint(0, 9, size=(n_tracks, 2)).astype(np.int64)
        want, got = start.copy(), start.copy()
        lt = learn_io(_lib, n_tracks, kind, track=track, learn=want)
        assert L.rx_track_learn_tally_host(ctypes.byref(lt), T, n, _lib.ptr(adv), None) == 0, L.rx_last_error()
        slots = np.ascontiguousarray(np.broadcast_to(track, (T, n)))
        host_tally_slots(L, n_tracks, kind, got, adv, slots, None)
        assert got.tobytes() == want.tobytes() and not np.array_equal(got, start)


# ---- 3: the episode-end draw from the replay tables --------------------------------------------------
@pytest.mark.parametrize("stale_mix", [0.0, 0.3])
@pytest.mark.parametrize("mode", ["random", "one_slot", "distinct", "none"])
@pytest.mark.parametrize("wave_order", [True, False])
def test_learn_episode_host_equals_the_restatement(L, mode, wave_order, stale_mix):
    n, n_tracks, seed, mix = 200, len(SKEWED), 0xFEEDFACE12345, 0.1
    track, done, terminated, info = tally_case(n, n_tracks, 11, mode)
    rs = np.random.RandomState(4)
    cs, ct = np.array(SKEWED, dtype=np.int64), np.array(STALE, dtype=np.int64)
    env_pos = rs.permutation(n).astype(np.int32) if wave_order else None
    start_tally = rs.randint(0, 9, size=(n_tracks, 4)).astype(np.int64)
    start_draws = rs.randint(0, 5, size=n).astype(np.uint32)
    start_draws[:3] = (0xFFFFFFFF, 0xFFFFFFFE, 0)  # the counter wraps like the uint32 it is
    start_pos = np.full(n, -9, dtype=np.int32)

    want = dict(tally=start_tally.copy(), track=track.copy(), draws=start_draws.copy(), pos_slot=start_pos.copy())
    want["slot_out"], branches = py_learn_episode(want["tally"], want["track"], want["draws"], SKEWED, STALE, seed, mix,
                                                  stale_mix, done, terminated, info, env_pos,
                                                  want["pos_slot"] if wave_order else None)
    got = dict(tally=start_tally.copy(), track=track.copy(), draws=start_draws.copy(), pos_slot=start_pos.copy(),
               slot_out=np.full(n, -5, dtype=np.int32))
    host_learn_episode(L, n_tracks, got["tally"], got["track"], got["draws"], cs, ct if stale_mix else None, seed, mix,
                       stale_mix, done, terminated, info, env_pos, got["pos_slot"] if wave_order else None,
                       got["slot_out"])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["slot_out"], track), "slot_out is the slot of every env during the step"
    ended = (done != 0) & (track >= 0) & (track < n_tracks)
    assert np.array_equal(got["draws"], (start_draws + ended.astype(np.uint32)))
    assert np.array_equal(got["track"][~ended], track[~ended]), "an env that did not end, or outside the table, stays"
    assert (got["track"][ended] >= 0).all() and (got["track"][ended] < n_tracks).all()
    if wave_order:
        assert np.array_equal(got["pos_slot"][env_pos[ended]], got["track"][ended])
        assert (got["pos_slot"][env_pos[~ended]] == -9).all()
    else:
        assert (got["pos_slot"] == -9).all()
    if mode == "none":
        assert np.array_equal(got["tally"], start_tally) and np.array_equal(got["draws"], start_draws)
    else:
        assert set(branches) == ({0, 1, 2} if stale_mix else {0, 2}), "every part of the mix draws"
    if mode == "random":
        assert ((track == -1) & (done != 0)).any() and ((track == n_tracks) & (done != 0)).any()


def test_a_zero_weight_slot_is_drawn_by_the_uniform_and_stale_parts_only(L):
    """Slots 1 and 4 weigh nothing in the score table; slot 1 is stale, slot 4 is not."""
    n, n_tracks, seed = 4000, len(SKEWED), 99
    cs, ct = np.array(SKEWED, dtype=np.int64), np.array(STALE, dtype=np.int64)
    done, term, info = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros((n, 4))
    for mix, stale_mix, reached in ((0.0, 0.0, set()), (0.5, 0.0, {1, 4}), (0.0, 0.5, {1}), (0.0, 1.0, {1})):
        track, draws = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        host_learn_episode(L, n_tracks, np.zeros((n_tracks, 4), dtype=np.int64), track, draws, cs, ct, seed, mix,
                           stale_mix, done, term, info)
        assert set(track.tolist()) & {1, 4} == reached, (mix, stale_mix)
        if stale_mix == 1.0:
            assert set(track.tolist()) == {1, 6}, "the stale slots only"


def test_a_second_call_continues_the_counters(L):
    n, n_tracks, seed, mix, stale_mix = 300, len(SKEWED), 31337, 0.1, 0.3
    cs, ct = np.array(SKEWED, dtype=np.int64), np.array(STALE, dtype=np.int64)
    done, term = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.uint8)
    info = np.zeros((n, 4))
    info[:, 1] = np.random.RandomState(1).rand(n)
    tally, track, draws = np.zeros((n_tracks, 4), dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, np.uint32)
    w_tally, w_track, w_draws = tally.copy(), track.copy(), draws.copy()
    seen = []
    for call in range(2):
        host_learn_episode(L, n_tracks, tally, track, draws, cs, ct, seed, mix, stale_mix, done, term, info)
        py_learn_episode(w_tally, w_track, w_draws, SKEWED, STALE, seed, mix, stale_mix, done, term, info)
        assert np.array_equal(track, w_track) and np.array_equal(draws, w_draws) and np.array_equal(tally, w_tally)
        assert (draws == call + 1).all()
        seen.append(track.copy())
    assert not np.array_equal(seen[0], seen[1]), "the second call must not repeat the first call's keys"
    assert tally[:, 0].sum() == 2 * n


@pytest.mark.parametrize("mode", ["random", "one_slot"])
def test_the_shared_table_gives_rx_track_episode(L, mode):
    """cdf_score pointing at tc->cdf, the same seed, stale_mix 0 (cdf_stale null): every output of
    rx_track_episode_host, bit for bit."""
    from rx import _lib
    n, n_tracks, seed, mix = 500, len(SKEWED), 0xFEEDFACE12345, 0.1
    track, done, terminated, info = tally_case(n, n_tracks, 12, mode)
    cdf = np.array(SKEWED, dtype=np.int64)
    env_pos = np.random.RandomState(2).permutation(n).astype(np.int32)
    outs = []
    for learn in (False, True):
        o = dict(tally=np.zeros((n_tracks, 4), dtype=np.int64), track=track.copy(), draws=np.arange(n, dtype=np.uint32),
                 pos_slot=np.full(n, -9, dtype=np.int32), slot_out=np.full(n, -5, dtype=np.int32))
        if learn:
            tc = track_io(_lib, n_tracks, track=o["track"], tally=o["tally"], cdf=cdf, seed=seed)
            lt = learn_io(_lib, n_tracks, seed=seed, cdf_score=cdf)
            ep = episode_io(_lib, o["draws"], env_pos, o["pos_slot"], o["slot_out"], mix)
            q = _lib.ptr
            assert L.rx_track_learn_episode_host(ctypes.byref(tc), ctypes.byref(lt), ctypes.byref(ep), 0.0, n, q(done),
                                                 q(terminated), q(info), None) == 0, L.rx_last_error()
        else:
            host_episode(L, n_tracks, o["tally"], o["track"], o["draws"], cdf, seed, mix, done, terminated, info,
                         env_pos, o["pos_slot"], o["slot_out"])
        outs.append(o)
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert not np.array_equal(outs[1]["track"], track)


# ---- 4: the argument checks --------------------------------------------------------------------------
def test_argument_checks_name_the_field(L):
    from rx import _lib
    T, n, nt, nan = 3, 8, 3, float("nan")
    q = _lib.ptr
    lbuf = dict(learn=np.zeros((nt, 2), dtype=np.int64), cdf_score=np.array([1, 2, 3], dtype=np.int64),
                cdf_stale=np.array([0, 1, 2], dtype=np.int64))
    tbuf = dict(track=np.zeros(n, dtype=np.int32), tally=np.zeros((nt, 4), dtype=np.int64))
    ebuf = dict(draws=np.zeros(n, dtype=np.uint32), env_pos=np.arange(n, dtype=np.int32),
                pos_slot=np.zeros(n, dtype=np.int32), slot_out=np.zeros(n, dtype=np.int32))
    adv, slots = np.zeros((T, n), dtype=np.float32), np.zeros((T, n), dtype=np.int32)
    dones = np.zeros((T, n), dtype=np.float32)
    done, term, info = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros((n, 4))

    def lt(n_tracks=nt, kind=0, **over):
        return ctypes.byref(learn_io(_lib, n_tracks, kind, **{**lbuf, **over}))

    def tc(n_tracks=nt, **over):
        return ctypes.byref(track_io(_lib, n_tracks, 0, **{**tbuf, **over}))

    def ep(mix=0.1, **over):
        return ctypes.byref(episode_io(_lib, mix=mix, **{**ebuf, **over}))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        Ta = getattr(L, "rx_track_learn_tally_slots" + sfx)
        refused(Ta(None, T, n, q(adv), q(slots), None, None), f"rx_track_learn_tally_slots{sfx}: null track learn io")
        for bad in (0, -4):
            refused(Ta(lt(n_tracks=bad), T, n, q(adv), q(slots), None, None), "n_tracks")
        for bad in (-1, 2):
            refused(Ta(lt(kind=bad), T, n, q(adv), q(slots), None, None), "kind")
        refused(Ta(lt(learn=None), T, n, q(adv), q(slots), None, None), "null learn")
        for bad in (0, -3):
            refused(Ta(lt(), bad, n, q(adv), q(slots), None, None), "T=")
        for bad in (0, -3, 1 << 31):
            refused(Ta(lt(), T, bad, q(adv), q(slots), None, None), "n=")
        refused(Ta(lt(), T, n, None, q(slots), None, None), "null adv")
        refused(Ta(lt(), T, n, q(adv), None, None, None), "null slots")
    # track, the tables and dones may be null: the tally reads learn only
    only = ctypes.byref(learn_io(_lib, nt, 1, learn=lbuf["learn"]))
    assert L.rx_track_learn_tally_slots_host(only, T, n, q(adv), q(slots), None, None) == 0
    assert L.rx_track_learn_tally_slots_host(only, T, n, q(adv), q(slots), q(dones), None) == 0

    rows = (q(done), q(term), q(info), None)
    for sfx in ("", "_host"):
        E = getattr(L, "rx_track_learn_episode" + sfx)
        refused(E(None, lt(), ep(), 0.1, n, *rows), "null track io")
        refused(E(tc(), None, ep(), 0.1, n, *rows), "null track learn io")
        refused(E(tc(), lt(), None, 0.1, n, *rows), "null episode io")
        for bad in (0, -4):
            refused(E(tc(n_tracks=bad), lt(), ep(), 0.1, n, *rows), "n_tracks")
            refused(E(tc(), lt(n_tracks=bad), ep(), 0.1, n, *rows), "n_tracks")
        refused(E(tc(), lt(n_tracks=nt + 1), ep(), 0.1, n, *rows), f"n_tracks={nt + 1} of the track learn io")
        for k in ("track", "tally"):
            refused(E(tc(**{k: None}), lt(), ep(), 0.1, n, *rows), f"null {k}")
        refused(E(tc(), lt(cdf_score=None), ep(), 0.1, n, *rows), "null cdf_score")
        refused(E(tc(), lt(cdf_stale=None), ep(), 0.1, n, *rows), "null cdf_stale")
        refused(E(tc(), lt(), ep(draws=None), 0.1, n, *rows), "null draws")
        refused(E(tc(), lt(), ep(env_pos=None), 0.1, n, *rows), "null env_pos")
        refused(E(tc(), lt(), ep(pos_slot=None), 0.1, n, *rows), "null pos_slot")
        for bad in (-0.01, 1.01, nan):
            refused(E(tc(), lt(), ep(mix=bad), 0.0, n, *rows), "mix=")
            refused(E(tc(), lt(), ep(mix=0.0), bad, n, *rows), "stale_mix=")
        refused(E(tc(), lt(), ep(mix=0.6), 0.5, n, *rows), "mix + stale_mix")
        for bad in (0, -3, 1 << 31):
            refused(E(tc(), lt(), ep(), 0.1, bad, *rows), "n=")
        refused(E(tc(), lt(), ep(), 0.1, n, None, q(term), q(info), None), "done")
        refused(E(tc(), lt(), ep(), 0.1, n, q(done), None, q(info), None), "terminated")
        refused(E(tc(), lt(), ep(), 0.1, n, q(done), q(term), None, None), "info")
    # tc->cdf is not read; without staleness neither is cdf_stale; the wave-order arrays and slot_out may be null
    assert L.rx_track_learn_episode_host(tc(), lt(cdf_stale=None, learn=None),
                                         ep(env_pos=None, pos_slot=None, slot_out=None), 0.0, n, *rows) == 0

    S, R = L.rx_track_learn_episode_step, L.rx_track_learn_episodic_rollout_steps
    io, r = _lib.RxIO(), _lib.RxRolloutIO()
    tail = (ctypes.byref(io), None, None)
    refused(S(None, None, lt(), ep(), 0.1, *tail), "null track io")
    refused(S(None, tc(), None, ep(), 0.1, *tail), "null track learn io")
    refused(S(None, tc(), lt(), None, 0.1, *tail), "null episode io")
    refused(S(None, tc(), lt(), ep(draws=None), 0.1, *tail), "null draws")
    refused(S(None, tc(), lt(), ep(mix=2.0), 0.1, *tail), "mix")
    refused(S(None, tc(), lt(), ep(), 1.5, *tail), "stale_mix")
    refused(S(None, tc(), lt(cdf_score=None), ep(), 0.1, *tail), "null cdf_score")
    refused(S(None, tc(), lt(n_tracks=nt + 2), ep(), 0.1, *tail), "n_tracks")
    refused(S(None, tc(), lt(), ep(), 0.1, *tail), "null handle")
    args = (ctypes.byref(io), ctypes.byref(r))
    refused(R(None, *args, None, lt(), ep(), 0.1, None, 0, None), "null track io")
    refused(R(None, *args, tc(n_tracks=0), lt(), ep(), 0.1, None, 0, None), "n_tracks")
    refused(R(None, *args, tc(), None, ep(), 0.1, None, 0, None), "null track learn io")
    refused(R(None, *args, tc(), lt(), None, 0.1, None, 0, None), "null episode io")
    refused(R(None, *args, tc(), lt(), ep(draws=None), 0.1, None, 0, None), "null draws")
    refused(R(None, *args, tc(), lt(cdf_stale=None), ep(), 0.1, None, 0, None), "null cdf_stale")
    refused(R(None, *args, tc(), lt(), ep(mix=0.7), 0.4, None, 0, None), "mix + stale_mix")
    refused(R(None, *args, tc(), lt(), ep(), 0.1, None, 7, None), "precision=7")
    refused(R(None, *args, tc(), lt(), ep(), 0.1, None, 0, None), "null handle")


# ---- 5: the trainer's and the tool's refusals --------------------------------------------------------
def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import base_config
    from rx.envs import MultiRacingEnv
    from rx.track_replay_episodic import EpisodicReplayCurriculumPPO as PPO

    def env_fn(i):
        raise AssertionError("no env may be built")
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        PPO(env_fn, base_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    with pytest.raises(ValueError, match="two-car"):
        PPO(lambda i: MultiRacingEnv(num_agents=2, num_sensors=11), base_config(num_envs=64, num_steps=16))
    bad_keys = (("episodic_scores_every", 0), ("replay_kind", "advantage"), ("replay_power", 11), ("replay_power", -1),
                ("replay_alpha", 0.0), ("replay_alpha", 1.5), ("replay_stale_mix", -0.1), ("replay_stale_mix", 1.5),
                ("curriculum_mix", 1.5), ("curriculum_power", 5), ("curriculum_prior", 0.0),
                ("curriculum_refresh", 1.5))
    for key, bad in bad_keys:
        with pytest.raises(ValueError, match=key):
            PPO(env_fn, base_config(num_envs=64, num_steps=16, **{key: bad}))
    with pytest.raises(ValueError, match="curriculum_mix \\+ replay_stale_mix"):
        PPO(env_fn, base_config(num_envs=64, num_steps=16, curriculum_mix=0.6, replay_stale_mix=0.5))


def test_curriculum_train_still_refuses_episodic_with_evolve():
    """Before it looks for a device; --episodic --replay is no longer refused by the argument check."""
    tool = os.path.join(ROOT, "tools", "curriculum_train.py")
    for extra in ((), ("--replay", "value_l1")):
        p = subprocess.run([sys.executable, tool, "--episodic", "--evolve", *extra], capture_output=True, text=True)
        assert p.returncode != 0 and "--evolve" in p.stderr and "--episodic" in p.stderr, p.stderr
    src = open(tool).read()
    assert "EpisodicReplayCurriculumPPO" in src and "not with --replay" not in src
