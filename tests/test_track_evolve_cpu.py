"""Track evolution without a GPU: the host twins rx_track_evolve_plan_host and
rx_track_evolve_host against a Python restatement of csrc/rx_track_evolve.h written
here (byte for byte: float64 with separately rounded operations in a fixed order;
rx_sincos through the oracle's device-libm build of rx_math.h), the invariants of
every spawned slot, the pinned layout of rx_track_evolve_io, every argument check
that runs before a HIP call, and EvolvingCurriculumPPO's refusals."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests.test_curriculum_cpu import M64, splitmix64
from tests.test_track_replay_cpu import host_tables, score_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rx_track_evolve_plan", "rx_track_evolve_plan_host", "rx_track_evolve", "rx_track_evolve_host")
FIELDS = ["n_tracks", "n_spawn", "slots", "cp_off", "cp", "width", "cdf_score", "plan", "cp_off_new", "cp_new",
          "width_new", "seed"]
TWO_PI = 2 * np.pi
R_MIN, R_MAX, CHORD2 = 36.0, 107.0, 23.04
SEED = 0xACCE1_5EED_0123
GUARD = -7.5


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


_ORACLE = []


def sincos(angles):
    """rx_sincos of every angle, from the oracle's own (gcc, device-libm) build of rx_math.h."""
    if not _ORACLE:
        from oracle.orc import Oracle
        _ORACLE.append(Oracle(device_libm=True))
    return _ORACLE[0].sincos_dev(np.asarray(angles, dtype=np.float64))


# ---- the Python restatement (Python floats are IEEE doubles; one rounding per operation) ----------
def unit(h):
    return float(h >> 11) * 2.0 ** -53


def mulhi(h, n):
    return (h * n) >> 64


def stream(seed, g, k):
    h = splitmix64(seed ^ splitmix64((((g & 0xFFFFFFFF) << 32) ^ k) & M64))
    while True:
        yield h
        h = splitmix64(h)


def clip(x, lo, hi):
    y = lo if x < lo else x
    return hi if y > hi else y


def div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def search(cdf, r):
    lo, hi = 0, len(cdf) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if r < int(cdf[mid]):
            hi = mid
        else:
            lo = mid + 1
    return lo


def cross(a, b):
    return a[0] * b[1] - a[1] * b[0]


def chord2(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    return dx * dx + dy * dy


def py_fresh(hs):
    """-> (points [P][2], width, (P, base, var)); hs: the slot's stream after the kind draw."""
    P = 10 + mulhi(next(hs), 5)
    base = 50 + mulhi(next(hs), 30)
    var = 10 + mulhi(next(hs), base // 2 - 20)
    jitter = 0.2 + 0.5 * unit(next(hs))
    smooth = 0.2 + 0.5 * unit(next(hs))
    width = float(6 + mulhi(next(hs), 4))
    spacing = TWO_PI / float(P)
    half = (jitter * spacing) / 2.0
    angles = [float(i) * spacing + (-half + (2.0 * half) * unit(next(hs))) for i in range(P)]
    r = []
    for i in range(P):
        v = float(base) + (-float(var) + (2.0 * float(var)) * unit(next(hs)))
        r.append(v if i == 0 else (1.0 - smooth) * v + smooth * r[i - 1])
    r[0] = (r[0] + r[-1]) / 2.0
    s, c = sincos(angles)
    return [[r[i] * float(c[i]), r[i] * float(s[i])] for i in range(P)], width, (P, base, var)


def py_edit(hs, parent_points, parent_width):
    """-> (points, width, edits applied, the indices of the points moved)."""
    pts = [[float(x), float(y)] for x, y in parent_points]
    P = len(pts)
    width = clip((float(parent_width) + float(mulhi(next(hs), 3))) - 1.0, 6.0, 9.0)
    n_edits = 1 + mulhi(next(hs), 3)
    applied, moved = 0, []
    for _ in range(n_edits):
        i = mulhi(next(hs), P)
        angular = next(hs) >> 63
        forward = next(hs) >> 63
        u = unit(next(hs))
        p, prev, nxt = pts[i], pts[(i - 1) % P], pts[(i + 1) % P]
        r = math.sqrt(p[0] * p[0] + p[1] * p[1])
        if angular:
            t, b = 0.35 * u, nxt if forward else prev
            q = [p[0] + t * (b[0] - p[0]), p[1] + t * (b[1] - p[1])]
            f = div(r, math.sqrt(q[0] * q[0] + q[1] * q[1]))
        else:
            q = list(p)
            f = div(clip(r * (0.8 + 0.4 * u), R_MIN, R_MAX), r)
        q = [q[0] * f, q[1] * f]
        if (q[0] != p[0] or q[1] != p[1]) and cross(prev, q) > 0.0 and cross(q, nxt) > 0.0 \
                and chord2(prev, q) >= CHORD2 and chord2(q, nxt) >= CHORD2:
            pts[i] = q
            applied += 1
            moved.append(i)
    return pts, width, applied, moved


def py_evolve(slots, cp_off, cp, width, cdf, seed, g, edit_frac):
    """-> (plan int32 [n_spawn, 4], cp_off_new, cp_new, width_new, details of the spawned slots)."""
    n, F = len(width), int(cdf[-1])
    tracks = [np.array(cp[cp_off[k]:cp_off[k + 1]], dtype=np.float64) for k in range(n)]
    widths = [float(w) for w in width]
    plan, details = np.zeros((len(slots), 4), dtype=np.int32), []
    for j, k in enumerate(slots):
        hs = stream(seed, g, int(k))
        if unit(next(hs)) < edit_frac and F > 0:
            parent = search(cdf, mulhi(next(hs), F))
            pts, w, applied, moved = py_edit(hs, cp[cp_off[parent]:cp_off[parent + 1]], width[parent])
            plan[j] = (1, parent, len(pts), applied)
            details.append(("edit", moved))
        else:
            pts, w, params = py_fresh(hs)
            plan[j] = (0, -1, len(pts), 0)
            details.append(("fresh", params))
        tracks[k], widths[k] = np.array(pts, dtype=np.float64).reshape(-1, 2), w
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    return plan, off, np.concatenate(tracks), np.array(widths, dtype=np.float64), details


# ---- the host twins ------------------------------------------------------------------------------------
def evolve_io(_lib, n_tracks, n_spawn, seed=0, **arrays):
    assert set(arrays) <= set(_lib.TRACK_EVOLVE_FIELDS)
    return _lib.RxTrackEvolveIO(n_tracks, n_spawn, *(_lib.ptr(arrays.get(k)) for k in _lib.TRACK_EVOLVE_FIELDS), seed)


def host_evolve(L, slots, cp_off, cp, width, cdf, seed, g, edit_frac):
    """The two host twins as TrackEvolver.spawn chains them -> (plan, cp_off_new, cp_new, width_new); every
    output carries a guard element."""
    from rx import _lib
    n, ns = len(width), len(slots)
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    cp_off = np.ascontiguousarray(cp_off, dtype=np.int32)
    cp, width = np.ascontiguousarray(cp, dtype=np.float64), np.ascontiguousarray(width, dtype=np.float64)
    cdf = np.ascontiguousarray(cdf, dtype=np.int64)
    plan = np.full((ns + 1, 4), -9, dtype=np.int32)
    ev = evolve_io(_lib, n, ns, seed, slots=slots, cp_off=cp_off, cdf_score=cdf, plan=plan)
    assert L.rx_track_evolve_plan_host(ctypes.byref(ev), g, edit_frac, None) == 0, L.rx_last_error()
    assert (plan[ns] == -9).all() and (plan[:ns, 3] == 0).all()
    points = np.diff(cp_off)
    points[slots] = plan[:ns, 2]
    off_new = np.concatenate([[0], np.cumsum(points)]).astype(np.int32)
    cp_new = np.full((int(off_new[-1]) + 1, 2), GUARD)
    width_new = np.full(n + 1, GUARD)
    ev = evolve_io(_lib, n, ns, seed, slots=slots, cp_off=cp_off, cp=cp, width=width, plan=plan, cp_off_new=off_new,
                   cp_new=cp_new, width_new=width_new)
    assert L.rx_track_evolve_host(ctypes.byref(ev), g, None) == 0, L.rx_last_error()
    assert (plan[ns] == -9).all() and (cp_new[-1] == GUARD).all() and width_new[n] == GUARD
    return plan[:ns].copy(), off_new, cp_new[:-1].copy(), width_new[:n].copy()


# ---- pools and rank tables (shared with tests/test_track_evolve_gpu.py) ----------------------------
def pool_case(n, seed):
    """-> (cp_off int32 [n + 1], cp float64 [total, 2], width float64 [n]) of the host generator."""
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    cps = gen_tracks(n, seed=None, rng=rng)
    width = np.array([rng.randint(6, 10) for _ in range(n)], dtype=np.float64)
    return pack(cps), np.ascontiguousarray(np.concatenate(cps)), width


def pack(cps):
    return np.concatenate([[0], np.cumsum([len(c) for c in cps])]).astype(np.int32)


def hand_made_pool():
    """Five slots: a triangle (P = 3) and a 64-gon (P = 64), the limits of rx_build_tracks, among three of
    the generator's; the rank table gives the two nearly all the weight."""
    off, cp, width = pool_case(3, 5)
    a3, a64 = np.arange(3) * TWO_PI / 3 + 0.1, np.arange(64) * TWO_PI / 64
    tri = np.column_stack([60.0 * np.cos(a3), 60.0 * np.sin(a3)])
    gon = np.column_stack([80.0 * np.cos(a64), 80.0 * np.sin(a64)])
    cps = [tri, cp[off[0]:off[1]], gon, cp[off[1]:off[2]], cp[off[2]:off[3]]]
    cdf = np.cumsum([1 << 40, 1, 1 << 40, 1, 1]).astype(np.int64)
    return pack(cps), np.ascontiguousarray(np.concatenate(cps)), np.array([6.0, 7.0, 9.0, 8.0, 6.0]), cdf


def rank_cdf(L, n, kind="mixed"):
    score, seen = score_case(kind, n)
    return host_tables(L, score, seen, 4, 9)[1].copy()


def spawn_sets(n):
    """n_spawn of 0, 1 and all, and (where the pool has room) a scattered quarter."""
    sets = [np.zeros(0, dtype=np.int32), np.array([n // 2], dtype=np.int32), np.arange(n, dtype=np.int32)]
    if n >= 5:
        sets.append(np.sort(np.random.RandomState(n).choice(n, size=n // 4, replace=False)).astype(np.int32))
    return sets


def check_invariants(L, slots, plan, details, old, new):
    """Every invariant of a spawned pool; old / new = (cp_off, cp, width)."""
    (off0, cp0, w0), (off1, cp1, w1) = old, new
    n = len(w1)
    spawned = np.zeros(n, dtype=bool)
    spawned[slots] = True
    for k in np.nonzero(~spawned)[0]:  # kept: byte-equal
        assert cp1[off1[k]:off1[k + 1]].tobytes() == cp0[off0[k]:off0[k + 1]].tobytes(), k
        assert w1[k].tobytes() == w0[k].tobytes(), k
    for j, k in enumerate(slots):
        kind, parent, P, applied = (int(v) for v in plan[j])
        pts = cp1[off1[k]:off1[k + 1]]
        assert len(pts) == P and w1[k] in (6.0, 7.0, 8.0, 9.0), (k, w1[k])
        radius = np.sqrt((pts * pts).sum(1))
        if kind == 0:
            assert parent == -1 and 10 <= P <= 14 and applied == 0
            # r * sqrt(cos^2 + sin^2): three roundings of relative size 2^-53 around the rule's own [36, 107]
            assert radius.min() >= R_MIN * (1 - 4 * 2.0 ** -53) and radius.max() <= R_MAX * (1 + 4 * 2.0 ** -53)
        else:
            assert 0 <= parent < n and P == off0[parent + 1] - off0[parent] and 0 <= applied <= 3
            assert abs(w1[k] - w0[parent]) <= 1.0
            par = cp0[off0[parent]:off0[parent + 1]]
            differ = np.nonzero((pts != par).any(1))[0]
            if details is not None:
                assert details[j][0] == "edit" and set(differ) <= set(details[j][1]) and applied == len(details[j][1])
            assert len(differ) <= applied
            # an edited point keeps its radius (angular, two roundings) or is clipped into [36, 107] (radial)
            for i in differ:
                r_old = math.sqrt(par[i] @ par[i])
                assert min(R_MIN, r_old) * (1 - 2.0 ** -50) <= radius[i] <= max(R_MAX, r_old) * (1 + 2.0 ** -50)
        nxt = np.roll(pts, -1, axis=0)
        assert (pts[:, 0] * nxt[:, 1] - pts[:, 1] * nxt[:, 0] > 0).all(), (k, "cross products")
        d = nxt - pts
        assert (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] >= CHORD2).all(), (k, "chords")
    build_host(L, off1, cp1, w1)


def build_host(L, cp_off, cp, width, factor=30):
    """rx_build_tracks_host accepts the pool and no slot is marked bad."""
    from rx import _lib
    n, wt = len(width), int(cp_off[-1]) * factor
    wp_off = np.zeros(n + 1, dtype=np.int32)
    wp, nrm, seg, meta = np.zeros((wt, 2)), np.zeros((wt, 2)), np.zeros((2 * wt, 4)), np.zeros((n, 8))
    rc = L.rx_build_tracks_host(n, factor, _lib.ptr(np.ascontiguousarray(cp_off, dtype=np.int32)),
                                _lib.ptr(np.ascontiguousarray(cp)), _lib.ptr(np.ascontiguousarray(width)),
                                _lib.ptr(wp_off), _lib.ptr(wp), _lib.ptr(nrm), _lib.ptr(seg), _lib.ptr(meta), None)
    assert rc == 0, L.rx_last_error()
    assert np.isfinite(meta).all() and np.isfinite(wp).all()
    return wp_off, wp, nrm, seg, meta


# ---- 1: the ABI, the layout, the build lists ------------------------------------------------------
def test_abi_is_still_25_and_the_new_symbols_are_exported(L):
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert "#define RX_ABI_VERSION 25" in hdr
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name


def test_rx_track_evolve_io_layout_matches_the_header():
    from rx import _lib
    T = _lib.RxTrackEvolveIO
    assert [f[0] for f in T._fields_] == FIELDS
    assert ctypes.sizeof(T) == 88
    assert [getattr(T, k).offset for k in FIELDS] == [0, 4] + list(range(8, 88, 8))
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    body = re.search(r"typedef struct rx_track_evolve_io \{(.*?)\} rx_track_evolve_io;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert [re.search(r"(\w+)$", d).group(1) for d in decl] == FIELDS
    kinds = ["*" if "*" in d else d.split()[0] for d in decl]
    assert kinds == ["int32_t", "int32_t"] + ["*"] * 9 + ["uint64_t"]
    assert (_lib.RX_TRACK_EVOLVE_W, _lib.RX_TRACK_EVOLVE_FRESH, _lib.RX_TRACK_EVOLVE_EDIT) == (4, 0, 1)
    # the pinned layouts beside it stay (additive)
    assert ctypes.sizeof(_lib.RxTrackLearnIO) == 80 and ctypes.sizeof(_lib.RxTrackIO) == 56


def test_sources_are_in_the_build_lists():
    from rx import _build
    assert "rx_track_evolve.hip" in _build.SOURCES and "rx_track_evolve_host.cpp" in _build.SOURCES
    assert "rx_track_evolve_host.cpp" in _build.HOST_ONLY and "rx_track_evolve.hip" not in _build.HOST_ONLY
    assert "rx_track_evolve.h" in _build.HEADERS
    for f in ("rx_track_evolve.hip", "rx_track_evolve_host.cpp", "rx_track_evolve.h"):
        assert os.path.exists(os.path.join(_build.CSRC, f))
    assert "-ffp-contract=off" in _build.FLAGS


# ---- 2: the host twins against the restatement, and the invariants ----------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_host_twins_equal_the_restatement(L, n):
    off, cp, width = pool_case(n, 40 + n)
    old = (off, cp, width)
    assert check_pool_is_valid(old)
    for cdf in (rank_cdf(L, n), np.zeros(n, dtype=np.int64)):
        for slots in spawn_sets(n):
            for edit_frac in (0.0, 0.5, 1.0):
                want = py_evolve(slots, off, cp, width, cdf, SEED, 3, edit_frac)
                got = host_evolve(L, slots, off, cp, width, cdf, SEED, 3, edit_frac)
                for a, b in zip(want[:4], got):
                    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (len(slots),
                                                                                                      edit_frac)
                plan = got[0]
                if cdf[-1] == 0 or edit_frac == 0.0:
                    assert (plan[:, 0] == 0).all(), "a zero rank table or edit_frac 0: every spawn is fresh"
                elif edit_frac == 1.0:
                    assert (plan[:, 0] == 1).all()
                elif len(slots) >= 16:
                    assert 0 < plan[:, 0].sum() < len(slots)
                if len(slots) == 0:
                    assert got[2].tobytes() == cp.tobytes() and got[3].tobytes() == width.tobytes()
                if n <= 65 or (edit_frac == 0.5 and cdf[-1] > 0):
                    check_invariants(L, slots, plan, want[4], old, got[1:])


def check_pool_is_valid(pool):
    off, cp, width = pool
    for k in range(len(width)):
        pts = cp[off[k]:off[k + 1]]
        nxt = np.roll(pts, -1, axis=0)
        d = nxt - pts
        if not ((pts[:, 0] * nxt[:, 1] - pts[:, 1] * nxt[:, 0] > 0).all() and ((d * d).sum(1) >= CHORD2).all()):
            return False
    return True


def test_hand_made_parents_at_the_point_count_limits(L):
    """P = 3 and P = 64: the smallest and the largest track rx_build_tracks takes."""
    off, cp, width, cdf = hand_made_pool()
    slots = np.arange(5, dtype=np.int32)
    parents = set()
    for g in range(1, 9):
        want = py_evolve(slots, off, cp, width, cdf, SEED, g, 1.0)
        got = host_evolve(L, slots, off, cp, width, cdf, SEED, g, 1.0)
        for a, b in zip(want[:4], got):
            assert a.tobytes() == b.tobytes(), g
        check_invariants(L, slots, got[0], want[4], (off, cp, width), got[1:])
        parents |= set(got[0][:, 1].tolist())
        assert set(got[0][:, 2].tolist()) <= {3, 64}
    assert parents == {0, 2}


def test_two_generations_chained(L):
    n = 65
    off, cp, width = pool_case(n, 9)
    cdf = rank_cdf(L, n)
    pools = {"py": (off, cp, width), "host": (off, cp, width)}
    for g, slots in ((1, spawn_sets(n)[3]), (2, np.arange(0, n, 3, dtype=np.int32))):
        want = py_evolve(slots, *pools["py"], cdf, SEED, g, 0.7)
        got = host_evolve(L, slots, *pools["host"], cdf, SEED, g, 0.7)
        for a, b in zip(want[:4], got):
            assert a.tobytes() == b.tobytes(), g
        check_invariants(L, slots, got[0], want[4], pools["host"], got[1:])
        pools = {"py": want[1:4], "host": got[1:]}
    # another generation or another seed is another stream
    a = host_evolve(L, slots, off, cp, width, cdf, SEED, 1, 0.7)
    b = host_evolve(L, slots, off, cp, width, cdf, SEED, 2, 0.7)
    c = host_evolve(L, slots, off, cp, width, cdf, SEED + 1, 1, 0.7)
    assert a[2].tobytes() != b[2].tobytes() and a[2].tobytes() != c[2].tobytes()


def test_offsets_that_do_not_follow_the_plan_mark_the_slot_and_write_nothing(L):
    from rx import _lib
    n = 5
    off, cp, width = pool_case(n, 2)
    cdf = rank_cdf(L, n)
    slots = np.array([1, 3], dtype=np.int32)
    plan, off_new, _, _ = host_evolve(L, slots, off, cp, width, cdf, SEED, 1, 0.5)
    bad = off_new.copy()
    bad[2:] += 1   # slot 1 (spawned) one point too long
    bad[5:] -= 1   # slot 4 (kept) one point too short
    cp_new, width_new = np.full((int(bad[-1]), 2), GUARD), np.full(n, GUARD)
    ev = evolve_io(_lib, n, 2, SEED, slots=slots, cp_off=off, cp=cp, width=width, plan=plan.copy(), cp_off_new=bad,
                   cp_new=cp_new, width_new=width_new)
    assert L.rx_track_evolve_host(ctypes.byref(ev), 1, None) == 0
    assert np.isnan(width_new[[1, 4]]).all() and np.isfinite(width_new[[0, 2, 3]]).all()
    for k in (1, 4):
        assert (cp_new[bad[k]:bad[k + 1]] == GUARD).all()
    for k in (0, 2):
        assert cp_new[bad[k]:bad[k + 1]].tobytes() == cp[off[k]:off[k + 1]].tobytes()


# ---- 3: the distribution of fresh tracks --------------------------------------------------------------
def test_fresh_tracks_cover_the_generators_ranges(L):
    n = 4096
    off = (np.arange(n + 1) * 3).astype(np.int32)  # any pool: every slot is replaced by a fresh track
    cp, width = np.ones((3 * n, 2)), np.full(n, 6.0)
    slots = np.arange(n, dtype=np.int32)
    want = py_evolve(slots, off, cp, width, np.zeros(n, dtype=np.int64), SEED, 1, 1.0)
    got = host_evolve(L, slots, off, cp, width, np.zeros(n, dtype=np.int64), SEED, 1, 1.0)
    for a, b in zip(want[:4], got):
        assert a.tobytes() == b.tobytes()
    params = np.array([d[1] for d in want[4]])
    assert set(params[:, 0]) == set(range(10, 15)) == set(got[0][:, 2].tolist())
    assert set(params[:, 1]) == set(range(50, 80))
    assert set(got[3].tolist()) == {6.0, 7.0, 8.0, 9.0}
    assert (params[:, 2] >= 10).all() and (params[:, 2] < params[:, 1] // 2 - 10).all()
    assert params[:, 2].max() == 28 and (params[params[:, 1] == 50, 2] <= 14).all()
    check_invariants(L, slots, got[0], want[4], (off, cp, width), got[1:])


# ---- 4: the condition: an edit child is seldom its parent's copy ----------------------------------------
def test_at_most_one_edit_child_in_a_hundred_equals_its_parent(L):
    """Eight chained generations of three gen_tracks pools of 512, every slot replaced by an edit child:
    at most 1 % of the children may equal their parent bit for bit (every edit dropped).  The cap is put
    to the restatement first, then to the host twin (which must give the restatement's bytes)."""
    n, gens = 512, 8
    cdf = ((np.arange(n, dtype=np.int64) + 1) << 32)  # every slot weighs the same
    slots = np.arange(n, dtype=np.int32)
    same_py = same_host = total = 0
    for s in (0, 1, 2):
        pool = pool_case(n, s)
        assert check_pool_is_valid(pool)
        host_pool = pool
        for g in range(1, gens + 1):
            plan, off1, cp1, w1, details = py_evolve(slots, *pool, cdf, SEED + s, g, 1.0)
            assert (plan[:, 0] == 1).all()
            same_py += int((plan[:, 3] == 0).sum())
            for j in range(n):  # no edit applied <=> the parent's points bit for bit
                par = pool[1][pool[0][plan[j, 1]]:pool[0][plan[j, 1] + 1]]
                assert (cp1[off1[j]:off1[j + 1]].tobytes() == par.tobytes()) == (plan[j, 3] == 0)
            got = host_evolve(L, slots, *host_pool, cdf, SEED + s, g, 1.0)
            same_host += int((got[0][:, 3] == 0).sum())
            assert got[2].tobytes() == cp1.tobytes() and got[0].tobytes() == plan.tobytes()
            if g in (1, gens):
                check_invariants(L, slots, got[0], details, host_pool, got[1:])
            pool, host_pool = (off1, cp1, w1), got[1:]
            total += n
    assert total == 12288
    print(f"edit children equal to their parent: restatement {same_py}, host twin {same_host} of {total}")
    assert same_py <= total // 100
    assert same_host <= total // 100


# ---- 5: the argument checks ---------------------------------------------------------------------------
def test_argument_checks_name_the_field(L):
    from rx import _lib
    n, ns = 4, 2
    off, cp, width = pool_case(n, 1)
    buf = dict(slots=np.array([0, 2], dtype=np.int32), cp_off=off, cp=cp, width=width,
               cdf_score=np.cumsum(np.ones(n, dtype=np.int64)), plan=np.zeros((ns, 4), dtype=np.int32),
               cp_off_new=off.copy(), cp_new=np.zeros((int(off[-1]) + 64, 2)), width_new=np.zeros(n))
    nan = float("nan")

    def ev(n_tracks=n, n_spawn=ns, **over):
        return ctypes.byref(evolve_io(_lib, n_tracks, n_spawn, 1, **{**buf, **over}))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        Pl, Ev = getattr(L, "rx_track_evolve_plan" + sfx), getattr(L, "rx_track_evolve" + sfx)
        calls = ((Pl, (1, 0.5, None), ("slots", "cp_off", "cdf_score", "plan")),
                 (Ev, (1, None), ("slots", "cp_off", "cp", "width", "plan", "cp_off_new", "cp_new", "width_new")))
        for fn, rest, reads in calls:
            refused(fn(None, *rest), "null track evolve io")
            for bad in (0, -4):
                refused(fn(ev(n_tracks=bad), *rest), "n_tracks")
            for bad in (-1, n + 1):
                refused(fn(ev(n_spawn=bad), *rest), "n_spawn")
            for k in reads:
                refused(fn(ev(**{k: None}), *rest), f"null {k}")
        for bad in (-0.01, 1.01, nan):
            refused(Pl(ev(), 1, bad, None), "edit_frac")
    # what an entry point does not read may be null; with nothing to spawn, slots and plan too
    only = lambda *keep, **kw: ev(**{k: None for k in buf if k not in keep}, **kw)  # noqa: E731
    assert L.rx_track_evolve_plan_host(only("slots", "cp_off", "cdf_score", "plan"), 1, 0.5, None) == 0
    assert L.rx_track_evolve_plan_host(only("cp_off", "cdf_score", n_spawn=0), 1, 0.5, None) == 0
    assert L.rx_track_evolve_plan(only("cp_off", "cdf_score", n_spawn=0), 1, 0.5, None) == 0, "no launch, no HIP call"
    assert L.rx_track_evolve_host(only("cp_off", "cp", "width", "cp_off_new", "cp_new", "width_new", n_spawn=0), 1,
                                  None) == 0
    assert buf["cp_new"][:int(off[-1])].tobytes() == cp.tobytes()


# ---- 6: the trainer's refusals and the unchanged default -----------------------------------------------
def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import base_config
    from rx.envs import MultiRacingEnv
    from rx.track_evolve import EvolvingCurriculumPPO

    def env_fn(i):
        raise AssertionError("no env may be built")
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        EvolvingCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    with pytest.raises(ValueError, match="two-car"):
        EvolvingCurriculumPPO(lambda i: MultiRacingEnv(num_agents=2, num_sensors=11),
                              base_config(num_envs=64, num_steps=16))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="evolve_edit"):
            EvolvingCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, evolve_edit=bad))
    for key, bad in (("replay_power", 11), ("curriculum_refresh", 1.5)):  # the parents' keys keep their checks
        with pytest.raises(ValueError, match=key):
            EvolvingCurriculumPPO(env_fn, base_config(num_envs=64, num_steps=16, **{key: bad}))


def test_the_default_hook_is_the_host_draw():
    """CurriculumPPO._spawn_tracks draws what resample_tracks always drew: gen_tracks and one width each
    from RandomState(seed + 7919 * g), np.random untouched."""
    from rx.curriculum import CurriculumPPO
    from rx.track import gen_tracks

    class Stub(CurriculumPPO):
        def __init__(self):
            self.config = {"seed": 11}
            self._cps, self._widths = [None] * 6, [None] * 6
            self.built = None

        def _replace_tracks(self, generation, slots, control_points, widths):
            self.built = (generation, list(slots), control_points, widths)
            return "table"

    state = np.random.get_state()
    t = Stub()
    assert t._spawn_tracks(3, np.array([4, 1])) == "table"
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    rng = np.random.RandomState((11 + 7919 * 3) % 2 ** 32)
    cps = gen_tracks(2, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(2)]
    g, slots, got_cps, got_widths = t.built
    assert g == 3 and slots == [4, 1] and got_widths == widths
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cps, got_cps))
