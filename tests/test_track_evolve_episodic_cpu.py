"""Track evolution in place without a GPU: the host twins rx_track_evolve_classes_host,
rx_track_evolve_inplace_host and rx_track_evolve_commit_host against numpy and against a
Python restatement of the in-place rules of csrc/rx_track_evolve.h written here (byte for
byte; the pieces the two forms share -- the stream, the edit, rx_sincos -- come from
tests/test_track_evolve_cpu.py), the pinned layout of rx_track_evolve_inplace_io, every
argument check that runs before a HIP call, and EpisodicEvolvingCurriculumPPO's refusals."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.test_track_evolve_cpu import (GUARD, SEED, TWO_PI, build_host, hand_made_pool, host_evolve, mulhi, pack,
                                         pool_case, py_edit, py_fresh, rank_cdf, search, sincos, spawn_sets, stream,
                                         unit)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rx_track_evolve_classes", "rx_track_evolve_inplace", "rx_track_evolve_commit")
FIELDS = ["n_tracks", "n_spawn", "slots", "cp_off", "cp", "width", "cdf_score", "order", "cdf_class", "class_end",
          "plan", "out_off", "cp_out", "width_out", "seed"]
MAX_P = 64
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the Python restatement of the in-place rules -------------------------------------------------
def py_classes(cp_off, cdf):
    """-> (order int32 [n], cdf_class int64 [n], class_end int32 [65])."""
    P = np.diff(cp_off).astype(np.int64)
    w = np.diff(np.concatenate([[0], np.asarray(cdf, dtype=np.int64)]))
    inside = (P >= 1) & (P <= MAX_P)
    order = np.argsort(np.where(inside, P, MAX_P + 1), kind="stable").astype(np.int32)
    cdf_class = np.cumsum(np.where(inside, w, 0)[order]).astype(np.int64)
    hist = np.bincount(P[inside], minlength=MAX_P + 1)[:MAX_P + 1]
    return order, cdf_class, np.cumsum(hist).astype(np.int32)


def py_fresh_points(hs, P):
    """A fresh track of the slot's own P points; hs: the slot's stream after the kind draw."""
    next(hs)  # draw 1 is consumed and discarded
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
    return [[r[i] * float(c[i]), r[i] * float(s[i])] for i in range(P)], width


def staging_offsets(slots, cp_off):
    return np.concatenate([[0], np.cumsum(np.diff(cp_off)[slots])]).astype(np.int32)


def py_inplace(slots, cp_off, cp, width, classes, seed, g, edit_frac, out_off=None):
    """-> (plan int32 [n_spawn, 4], out_off, cp_out, width_out); what is not written holds GUARD."""
    order, cdf_class, class_end = classes
    out_off = staging_offsets(slots, cp_off) if out_off is None else out_off
    ns, n = len(slots), len(cp_off) - 1
    plan = np.zeros((ns, 4), dtype=np.int32)
    cp_out, width_out = np.full((int(out_off[-1]), 2), GUARD), np.full(ns, GUARD)
    for j, k in enumerate(slots):
        P = int(cp_off[k + 1] - cp_off[k]) if 0 <= k < n else 0
        plan[j] = (0, -1, P, 0)
        if not (0 <= k < n and 1 <= P <= MAX_P and out_off[j + 1] - out_off[j] == P):
            width_out[j] = NAN
            continue
        hs = stream(seed, g, int(k))
        u = unit(next(hs))
        lo, hi = int(class_end[P - 1]), int(class_end[P])
        base = int(cdf_class[lo - 1]) if lo else 0
        F = int(cdf_class[hi - 1]) - base
        if u < edit_frac and F > 0:
            t = base + mulhi(next(hs), F)
            parent = int(order[lo + search(cdf_class[lo:hi], t)])
            pts, w, applied, _ = py_edit(hs, cp[cp_off[parent]:cp_off[parent + 1]], width[parent])
            plan[j] = (1, parent, P, applied)
        else:
            pts, w = py_fresh_points(hs, P)
        cp_out[out_off[j]:out_off[j + 1]] = pts
        width_out[j] = w
    return plan, out_off, cp_out, width_out


def py_commit(slots, cp_off, cp, width, out_off, cp_out, width_out):
    cp, width = cp.copy(), width.copy()
    for j, k in enumerate(slots):
        P = int(cp_off[k + 1] - cp_off[k])
        if 1 <= P <= MAX_P and out_off[j + 1] - out_off[j] == P:
            cp[cp_off[k]:cp_off[k + 1]] = cp_out[out_off[j]:out_off[j + 1]]
        width[k] = width_out[j]
    return cp, width


# ---- the host twins (shared with tests/test_track_evolve_episodic_gpu.py) -----------------------------
def inplace_io(_lib, n_tracks, n_spawn, seed=0, **arrays):
    assert set(arrays) <= set(_lib.TRACK_EVOLVE_INPLACE_FIELDS)
    return _lib.RxTrackEvolveInplaceIO(n_tracks, n_spawn,
                                       *(_lib.ptr(arrays.get(k)) for k in _lib.TRACK_EVOLVE_INPLACE_FIELDS), seed)


def c32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def host_classes(L, cp_off, cdf):
    """rx_track_evolve_classes_host -> (order, cdf_class, class_end); the guards are checked."""
    from rx import _lib
    n = len(cp_off) - 1
    order, cdf_class = np.full(n + 1, -9, dtype=np.int32), np.full(n + 1, -9, dtype=np.int64)
    class_end = np.full(MAX_P + 2, -9, dtype=np.int32)
    ev = inplace_io(_lib, n, 0, cp_off=c32(cp_off), cdf_score=np.ascontiguousarray(cdf, dtype=np.int64), order=order,
                    cdf_class=cdf_class, class_end=class_end)
    assert L.rx_track_evolve_classes_host(ctypes.byref(ev), None) == 0, L.rx_last_error()
    assert order[n] == -9 and cdf_class[n] == -9 and class_end[MAX_P + 1] == -9
    return order[:n].copy(), cdf_class[:n].copy(), class_end[:MAX_P + 1].copy()


def host_inplace(L, slots, cp_off, cp, width, classes, seed, g, edit_frac, out_off=None, sfx="_host"):
    """rx_track_evolve_inplace_host -> (plan, out_off, cp_out, width_out); GUARD where nothing was written."""
    from rx import _lib
    n, ns = len(cp_off) - 1, len(slots)
    out_off = c32(staging_offsets(slots, cp_off) if out_off is None else out_off)
    plan = np.full((ns + 1, 4), -9, dtype=np.int32)
    cp_out, width_out = np.full((int(out_off[-1]) + 1, 2), GUARD), np.full(ns + 1, GUARD)
    cp0, w0 = np.ascontiguousarray(cp, dtype=np.float64), np.ascontiguousarray(width, dtype=np.float64)
    cp_in, w_in = cp0.copy(), w0.copy()
    order, cdf_class, class_end = (np.ascontiguousarray(a) for a in classes)
    ev = inplace_io(_lib, n, ns, seed, slots=c32(slots), cp_off=c32(cp_off), cp=cp_in, width=w_in, order=order,
                    cdf_class=cdf_class, class_end=class_end, plan=plan, out_off=out_off, cp_out=cp_out,
                    width_out=width_out)
    assert getattr(L, "rx_track_evolve_inplace" + sfx)(ctypes.byref(ev), g, edit_frac, None) == 0, L.rx_last_error()
    assert (plan[ns] == -9).all() and (cp_out[-1] == GUARD).all() and width_out[ns] == GUARD
    assert cp_in.tobytes() == cp0.tobytes() and w_in.tobytes() == w0.tobytes(), "the pool was written"
    return plan[:ns].copy(), out_off, cp_out[:-1].copy(), width_out[:ns].copy()


def host_commit(L, slots, cp_off, cp, width, out_off, cp_out, width_out):
    """rx_track_evolve_commit_host on copies of the pool with a guard element -> (cp, width)."""
    from rx import _lib
    n, ns = len(cp_off) - 1, len(slots)
    cp1 = np.concatenate([np.ascontiguousarray(cp, dtype=np.float64), [[GUARD, GUARD]]])
    w1 = np.concatenate([np.ascontiguousarray(width, dtype=np.float64), [GUARD]])
    ev = inplace_io(_lib, n, ns, slots=c32(slots), cp_off=c32(cp_off), cp=cp1, width=w1, out_off=c32(out_off),
                    cp_out=np.ascontiguousarray(cp_out), width_out=np.ascontiguousarray(width_out))
    assert L.rx_track_evolve_commit_host(ctypes.byref(ev), None) == 0, L.rx_last_error()
    assert (cp1[-1] == GUARD).all() and w1[n] == GUARD
    return cp1[:-1].copy(), w1[:n].copy()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def one_class_zero(cp_off, cdf, p0):
    """The rank table with every weight raised by one (rank ** -4 rounds to 0 from rank 257 on) and the
    weights of the slots of p0 points taken out: exactly one class weighs nothing."""
    w = np.diff(np.concatenate([[0], cdf])) + 1
    w[np.diff(cp_off) == p0] = 0
    return np.cumsum(w).astype(np.int64)


def class_weights(classes):
    """F of every point count 0..64 from the class table (0 for an empty class)."""
    _, cdf_class, class_end = classes
    c = np.concatenate([[0], cdf_class])
    return np.concatenate([[0], c[class_end[1:]] - c[class_end[:-1]]])


def class_cases(L, n):
    """(name, cp_off, cdf) of every class-table case at n slots (the GPU test walks the same)."""
    const = (np.arange(n + 1) * 12).astype(np.int32)
    cyc = np.concatenate([[0], np.cumsum(3 + np.arange(n) % 62)]).astype(np.int32)
    gen = pool_case(n, 40 + n)[0]
    cdf = rank_cdf(L, n)
    out = [("one point count", const, cdf), ("cycling 3..64", cyc, cdf), ("generated", gen, cdf),
           ("zero table", cyc, np.zeros(n, dtype=np.int64))]
    p0 = int(np.diff(gen)[n // 2])
    out.append(("one class weighs nothing", gen, one_class_zero(gen, cdf, p0)))
    out.append(("one class weighs nothing, cycling", cyc, one_class_zero(cyc, cdf, 3)))
    return out


# ---- 1: the ABI, the layout, the build lists ------------------------------------------------------
def test_abi_is_still_25_and_the_new_symbols_are_exported(L):
    from rx import _lib
    assert L.rx_abi_version() == 25 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert "#define RX_ABI_VERSION 25" in hdr
    for base in NEW:
        for name in (base, base + "_host"):
            assert hasattr(L, name) and name in _lib.EXPORTS and f"int {name}(" in hdr, name


def test_rx_track_evolve_inplace_io_layout_matches_the_header():
    from rx import _lib
    T = _lib.RxTrackEvolveInplaceIO
    assert [f[0] for f in T._fields_] == FIELDS
    assert ctypes.sizeof(T) == 112
    assert [getattr(T, k).offset for k in FIELDS] == [0, 4] + list(range(8, 112, 8))
    hdr = open(os.path.join(ROOT, "include", "rx.h")).read()
    body = re.search(r"typedef struct rx_track_evolve_inplace_io \{(.*?)\} rx_track_evolve_inplace_io;", hdr,
                     re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [d.strip() for d in body.split(";") if d.strip()]
    assert [re.search(r"(\w+)$", d).group(1) for d in decl] == FIELDS
    kinds = ["*" if "*" in d else d.split()[0] for d in decl]
    assert kinds == ["int32_t", "int32_t"] + ["*"] * 12 + ["uint64_t"]
    assert _lib.RX_TRACK_MAX_P == MAX_P
    src = open(os.path.join(ROOT, "self-play-racing_amd", "csrc", "rx_spline.h")).read()
    assert "#define RX_TRACK_MAX_P 64" in src
    assert ctypes.sizeof(_lib.RxTrackEvolveIO) == 88  # the pinned layout beside it stays (additive)


def test_sources_are_in_the_build_lists():
    from rx import _build
    assert "rx_track_evolve.hip" in _build.SOURCES and "rx_track_evolve_host.cpp" in _build.SOURCES
    assert "rx_track_evolve_host.cpp" in _build.HOST_ONLY and "rx_track_evolve.h" in _build.HEADERS
    hip = open(os.path.join(_build.CSRC, "rx_track_evolve.hip")).read()
    host = open(os.path.join(_build.CSRC, "rx_track_evolve_host.cpp")).read()
    for k in ("classes", "inplace", "commit"):
        assert f"k_track_evolve_{k}" in hip and f"rx_host_track_evolve_{k}" in host, k
    assert "#include <hip" not in host, "the twins make no HIP call"


# ---- 2: the class table ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_class_twin_equals_numpy(L, n):
    for name, off, cdf in class_cases(L, n):
        order, cdf_class, class_end = host_classes(L, off, cdf)
        P = np.diff(off)
        w = np.diff(np.concatenate([[0], cdf]))
        assert np.array_equal(order, np.argsort(P, kind="stable")), name
        assert np.array_equal(cdf_class, np.cumsum(w[order])), name
        assert np.array_equal(class_end, np.cumsum(np.bincount(P, minlength=MAX_P + 1))), name
        assert class_end[0] == 0 and class_end[MAX_P] == n and cdf_class[-1] == cdf[-1]
        for a, b in zip((order, cdf_class, class_end), py_classes(off, cdf)):
            assert same(a, b), name
        if name.startswith("one class weighs nothing"):
            p0 = 3 if "cycling" in name else int(P[n // 2])
            lo, hi = class_end[p0 - 1], class_end[p0]
            assert hi > lo and cdf_class[hi - 1] - (cdf_class[lo - 1] if lo else 0) == 0
            zero = [p for p in range(1, MAX_P + 1) if class_end[p] > class_end[p - 1]
                    and cdf_class[class_end[p] - 1] == (cdf_class[class_end[p - 1] - 1] if class_end[p - 1] else 0)]
            assert zero == [p0], "exactly one class weighs nothing"


def test_class_twin_on_the_hand_made_pool_and_out_of_range_counts(L):
    off, _, _, cdf = hand_made_pool()
    order, cdf_class, class_end = host_classes(L, off, cdf)
    P = np.diff(off)
    assert set(P.tolist()) >= {3, 64} and np.array_equal(order, np.argsort(P, kind="stable"))
    assert order[0] == 0 and order[-1] == 2 and class_end[3] == 1 and class_end[63] == 4 and class_end[64] == 5
    assert np.array_equal(cdf_class, np.cumsum(np.diff(np.concatenate([[0], cdf]))[order]))
    # P = 0 and P = 65 belong to no class: behind the last class in slot order, weight 0, nothing out of bounds
    P = np.array([12, 0, 65, 12, 64, 0, 1, 70], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(P)]).astype(np.int32)
    cdf = np.cumsum(np.arange(1, 9, dtype=np.int64) << 20)
    order, cdf_class, class_end = host_classes(L, off, cdf)
    assert order.tolist() == [6, 0, 3, 4, 1, 2, 5, 7]
    w = np.arange(1, 9, dtype=np.int64) << 20
    assert cdf_class.tolist() == np.cumsum([w[6], w[0], w[3], w[4], 0, 0, 0, 0]).tolist()
    assert class_end[0] == 0 and class_end[1] == 1 and class_end[11] == 1 and class_end[12] == 3 \
        and class_end[63] == 3 and class_end[64] == 4
    for a, b in zip((order, cdf_class, class_end), py_classes(off, cdf)):
        assert same(a, b)


# ---- 3: the in-place twin against the restatement ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_inplace_twin_equals_the_restatement(L, n):
    off, cp, width = pool_case(n, 40 + n)
    P = np.diff(off)
    cdf = rank_cdf(L, n)
    p0 = int(P[n // 2])
    for name, table in (("ranked", cdf), ("zero", np.zeros(n, dtype=np.int64)),
                        ("one class zero", one_class_zero(off, cdf, p0))):
        classes = host_classes(L, off, table)
        for slots in spawn_sets(n):
            for edit_frac in (0.0, 0.5, 1.0):
                want = py_inplace(slots, off, cp, width, classes, SEED, 3, edit_frac)
                got = host_inplace(L, slots, off, cp, width, classes, SEED, 3, edit_frac)
                for a, b in zip(want, got):
                    assert same(a, b), (name, len(slots), edit_frac)
                plan = got[0]
                assert np.array_equal(plan[:, 2], P[slots]) and np.isfinite(got[3]).all()
                edit = plan[:, 0] == 1
                assert np.array_equal(P[plan[edit, 1]], plan[edit, 2]), "a parent of another point count"
                assert (plan[~edit, 1] == -1).all() and (plan[~edit, 3] == 0).all()
                F = class_weights(classes)
                if name == "zero" or edit_frac == 0.0:
                    assert not edit.any()
                elif edit_frac == 1.0:  # a class of zero weight gives FRESH, every other class EDIT
                    assert np.array_equal(edit, F[P[slots]] > 0)
                    if name == "one class zero":
                        assert np.array_equal(F[P[slots]] > 0, P[slots] != p0)
                    elif n <= 65:
                        assert edit.all()
                elif len(slots) >= 16:
                    assert 0 < edit.sum() < len(slots)


def test_a_slot_parents_itself_and_a_retired_slot_parents_another(L):
    """Every slot of a 64-slot pool spawned as an edit: some slot draws itself, and every parent is a slot
    that is being replaced.  The children are edits of the OLD points (the restatement reads the pool as it
    stood; the twin never writes it), also after the commit has put the children in."""
    n = 64
    off, cp, width = pool_case(n, 104)
    classes = host_classes(L, off, rank_cdf(L, n))
    slots = np.arange(n, dtype=np.int32)
    want = py_inplace(slots, off, cp, width, classes, SEED, 5, 1.0)
    plan, out_off, cp_out, width_out = host_inplace(L, slots, off, cp, width, classes, SEED, 5, 1.0)
    for a, b in zip(want, (plan, out_off, cp_out, width_out)):
        assert same(a, b)
    assert (plan[:, 0] == 1).all()
    own = np.nonzero(plan[:, 1] == slots)[0]
    other = np.nonzero(plan[:, 1] != slots)[0]
    assert len(own) >= 1 and len(other) >= 1, "pick another generation: no slot drew itself"
    cp1, w1 = host_commit(L, slots, off, cp, width, out_off, cp_out, width_out)
    for j in list(own[:2]) + list(other[:4]):
        k, parent = int(slots[j]), int(plan[j, 1])
        hs = stream(SEED, 5, k)
        next(hs), next(hs)
        pts, w, applied, _ = py_edit(hs, cp[off[parent]:off[parent + 1]], width[parent])
        assert np.array(pts).tobytes() == cp1[off[k]:off[k + 1]].tobytes() and w == w1[k] and applied == plan[j, 3]


def test_fresh_rows_equal_the_pool_rebuilding_path_where_it_drew_the_same_point_count(L):
    n = 65
    off, cp, width = pool_case(n, 9)
    slots = np.arange(n, dtype=np.int32)
    zero = np.zeros(n, dtype=np.int64)
    plan_old, off_new, cp_new, width_new = host_evolve(L, slots, off, cp, width, zero, SEED, 2, 0.0)
    plan, out_off, cp_out, width_out = host_inplace(L, slots, off, cp, width, host_classes(L, off, zero), SEED, 2, 0.0)
    assert (plan_old[:, 0] == 0).all() and (plan[:, 0] == 0).all()
    hit = np.nonzero(plan_old[:, 2] == plan[:, 2])[0]
    assert len(hit) >= 1 and len(hit) < n, "choose a seed at which some slot draws its own point count"
    for j in hit:
        assert cp_out[out_off[j]:out_off[j + 1]].tobytes() == cp_new[off_new[j]:off_new[j + 1]].tobytes(), j
        assert width_out[j].tobytes() == width_new[j].tobytes(), j
    # and through py_fresh, whose P is the stream's own
    j = int(hit[0])
    hs = stream(SEED, 2, int(slots[j]))
    next(hs)
    pts, w, (P, _, _) = py_fresh(hs)
    assert P == plan[j, 2] and np.array(pts).tobytes() == cp_out[out_off[j]:out_off[j + 1]].tobytes()


# ---- 4: the commit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 65, 1000])
def test_commit_replaces_the_spawned_spans_only(L, n):
    off, cp, width = pool_case(n, 40 + n)
    classes = host_classes(L, off, rank_cdf(L, n))
    for slots in spawn_sets(n):
        plan, out_off, cp_out, width_out = host_inplace(L, slots, off, cp, width, classes, SEED, 1, 0.5)
        cp1, w1 = host_commit(L, slots, off, cp, width, out_off, cp_out, width_out)
        want = py_commit(slots, off, cp, width, out_off, cp_out, width_out)
        assert same(cp1, want[0]) and same(w1, want[1])
        spawned = np.zeros(n, dtype=bool)
        spawned[slots] = True
        for k in range(n):
            a, b = cp1[off[k]:off[k + 1]].tobytes(), cp[off[k]:off[k + 1]].tobytes()
            if spawned[k]:
                j = int(np.searchsorted(slots, k))
                assert a == cp_out[out_off[j]:out_off[j + 1]].tobytes() and w1[k] == width_out[j]
            else:
                assert a == b and w1[k].tobytes() == width[k].tobytes()
        if len(slots) == 0:
            assert cp1.tobytes() == cp.tobytes() and w1.tobytes() == width.tobytes()
        if n <= 65:
            build_host(L, off, cp1, w1)  # asserts a finite meta


def test_two_generations_chained(L):
    n = 65
    off, cp, width = pool_case(n, 9)
    cdf = rank_cdf(L, n)
    classes = host_classes(L, off, cdf)
    pools = {"py": (cp, width), "host": (cp, width)}
    hist = np.bincount(np.diff(off))
    for g, slots in ((1, spawn_sets(n)[3]), (2, np.arange(0, n, 3, dtype=np.int32))):
        want = py_inplace(slots, off, *pools["py"], classes, SEED, g, 0.7)
        got = host_inplace(L, slots, off, *pools["host"], classes, SEED, g, 0.7)
        for a, b in zip(want, got):
            assert same(a, b), g
        pools = {"py": py_commit(slots, off, *pools["py"], *want[1:]),
                 "host": host_commit(L, slots, off, *pools["host"], *got[1:])}
        assert same(pools["py"][0], pools["host"][0]) and same(pools["py"][1], pools["host"][1])
        build_host(L, off, *pools["host"])
    assert pools["host"][0].tobytes() != cp.tobytes() and np.array_equal(np.bincount(np.diff(off)), hist)
    a = host_inplace(L, slots, off, cp, width, classes, SEED, 1, 0.7)
    b = host_inplace(L, slots, off, cp, width, classes, SEED, 2, 0.7)
    c = host_inplace(L, slots, off, cp, width, classes, SEED + 1, 1, 0.7)
    assert a[2].tobytes() != b[2].tobytes() and a[2].tobytes() != c[2].tobytes()


# ---- 5: spans and point counts that do not fit ----------------------------------------------------
def test_a_staging_span_that_is_not_the_point_count_marks_the_slot_and_writes_nothing(L):
    n = 5
    off, cp, width = pool_case(n, 2)
    classes = host_classes(L, off, rank_cdf(L, n))
    slots = np.array([1, 3, 4], dtype=np.int32)
    bad = staging_offsets(slots, off)
    bad[2:] += 1  # slot 3 one point too long (slot 1 and slot 4 keep their spans)
    want = py_inplace(slots, off, cp, width, classes, SEED, 1, 0.5, out_off=bad)
    plan, _, cp_out, width_out = host_inplace(L, slots, off, cp, width, classes, SEED, 1, 0.5, out_off=bad)
    for a, b in zip(want, (plan, bad, cp_out, width_out)):
        assert same(a, b)
    assert np.isnan(width_out[1]) and np.isfinite(width_out[[0, 2]]).all()
    assert (cp_out[bad[1]:bad[2]] == GUARD).all() and plan[1].tolist() == [0, -1, int(off[4] - off[3]), 0]
    cp1, w1 = host_commit(L, slots, off, cp, width, bad, cp_out, width_out)
    assert cp1[off[3]:off[4]].tobytes() == cp[off[3]:off[4]].tobytes() and np.isnan(w1[3])
    for j, k in ((0, 1), (2, 4)):
        assert cp1[off[k]:off[k + 1]].tobytes() == cp_out[bad[j]:bad[j + 1]].tobytes() and w1[k] == width_out[j]
    for k in (0, 2):
        assert cp1[off[k]:off[k + 1]].tobytes() == cp[off[k]:off[k + 1]].tobytes() and w1[k] == width[k]


def test_point_counts_of_0_and_65_corrupt_nothing(L):
    real = pool_case(3, 5)
    rs = np.random.RandomState(3)
    tracks = [real[1][real[0][0]:real[0][1]], np.zeros((0, 2)), 50.0 * rs.rand(65, 2), real[1][real[0][1]:real[0][2]],
              np.zeros((0, 2)), real[1][real[0][2]:real[0][3]]]
    off, cp = pack(tracks), np.ascontiguousarray(np.concatenate(tracks))
    width = np.array([6.0, 7.0, 8.0, 9.0, 6.0, 7.0])
    cdf = np.cumsum(np.full(6, 1 << 30, dtype=np.int64))
    classes = host_classes(L, off, cdf)
    assert same(classes[0], py_classes(off, cdf)[0])
    slots = np.arange(6, dtype=np.int32)
    for edit_frac in (0.0, 1.0):
        want = py_inplace(slots, off, cp, width, classes, SEED, 1, edit_frac)
        got = host_inplace(L, slots, off, cp, width, classes, SEED, 1, edit_frac)  # guards checked inside
        for a, b in zip(want, got):
            assert same(a, b)
        plan, out_off, cp_out, width_out = got
        assert np.isnan(width_out[[1, 2, 4]]).all() and np.isfinite(width_out[[0, 3, 5]]).all()
        assert (cp_out[out_off[2]:out_off[3]] == GUARD).all() and plan[:, 2].tolist() == np.diff(off).tolist()
        assert (plan[plan[:, 0] == 1, 1] != 2).all(), "the 65-point slot was drawn as a parent"
        cp1, w1 = host_commit(L, slots, off, cp, width, out_off, cp_out, width_out)
        assert cp1[off[2]:off[3]].tobytes() == cp[off[2]:off[3]].tobytes() and np.isnan(w1[[1, 2, 4]]).all()


# ---- 6: the argument checks ---------------------------------------------------------------------------
def test_argument_checks_name_the_field_and_write_nothing(L):
    from rx import _lib
    n, ns = 4, 2
    off, cp, width = pool_case(n, 1)
    slots = np.array([0, 2], dtype=np.int32)
    out_off = staging_offsets(slots, off)

    def fresh_buffers():
        return dict(slots=slots, cp_off=off, cp=cp.copy(), width=width.copy(),
                    cdf_score=np.cumsum(np.ones(n, dtype=np.int64)), order=np.full(n, -9, dtype=np.int32),
                    cdf_class=np.full(n, -9, dtype=np.int64), class_end=np.full(MAX_P + 1, -9, dtype=np.int32),
                    plan=np.full((ns, 4), -9, dtype=np.int32), out_off=out_off,
                    cp_out=np.full((int(out_off[-1]), 2), GUARD), width_out=np.full(ns, GUARD))

    buf = fresh_buffers()
    before = {k: v.copy() for k, v in buf.items()}

    def ev(n_tracks=n, n_spawn=ns, **over):
        return ctypes.byref(inplace_io(_lib, n_tracks, n_spawn, 1, **{**buf, **over}))

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, (rc, word)
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    touched = {"classes": ("cp_off", "cdf_score", "order", "cdf_class", "class_end"),
               "inplace": ("slots", "cp_off", "cp", "width", "order", "cdf_class", "class_end", "plan", "out_off",
                           "cp_out", "width_out"),
               "commit": ("slots", "cp_off", "cp", "width", "out_off", "cp_out", "width_out")}
    for sfx in ("", "_host"):
        for which, fields in touched.items():
            fn = getattr(L, f"rx_track_evolve_{which}{sfx}")
            rest = (1, 0.5, None) if which == "inplace" else (None,)
            refused(fn(None, *rest), "null track evolve inplace io")
            for bad in (0, -4):
                refused(fn(ev(n_tracks=bad), *rest), "n_tracks")
            for bad in (-1, n + 1):
                refused(fn(ev(n_spawn=bad), *rest), "n_spawn")
            for k in fields:
                refused(fn(ev(**{k: None}), *rest), f"null {k}")
        for bad in (-0.01, 1.01, NAN):
            refused(getattr(L, "rx_track_evolve_inplace" + sfx)(ev(), 1, bad, None), "edit_frac")
    for k, v in buf.items():
        assert v.tobytes() == before[k].tobytes(), f"a refused call wrote {k}"
    # what an entry point does not touch may be null; with nothing to spawn inplace and commit do nothing at all
    only = lambda which, **kw: ev(**{k: None for k in buf if k not in touched[which]}, **kw)  # noqa: E731
    nothing = lambda **kw: ev(**{k: None for k in buf}, **kw)  # noqa: E731
    for sfx in ("", "_host"):  # (without a device too: no launch, no HIP call)
        assert getattr(L, "rx_track_evolve_inplace" + sfx)(nothing(n_spawn=0), 1, 0.5, None) == 0
        assert getattr(L, "rx_track_evolve_commit" + sfx)(nothing(n_spawn=0), None) == 0
    assert L.rx_track_evolve_classes_host(only("classes", n_spawn=0), None) == 0
    assert L.rx_track_evolve_inplace_host(only("inplace"), 1, 0.5, None) == 0
    assert L.rx_track_evolve_commit_host(only("commit"), None) == 0
    assert buf["order"].tolist() == np.argsort(np.diff(off), kind="stable").tolist()


# ---- 7: the Python layer without a device -----------------------------------------------------------
def test_replacement_from_device_checks_the_spans_from_the_host_offsets(monkeypatch):
    from rx.track_device import DeviceTrackTable

    def no_build(*a, **kw):
        raise AssertionError("nothing may be built")
    monkeypatch.setattr(DeviceTrackTable, "build_from_device", classmethod(no_build))
    wp_off = np.concatenate([[0], np.cumsum([300, 360, 420, 300])]).astype(np.int32)

    class Meta:
        device = "cpu"
    t = DeviceTrackTable(wp_off, None, None, None, Meta(), factor=30)
    with pytest.raises(ValueError, match=r"slot 2\b.*keeps its point count"):
        t.replacement_from_device([1, 2], [0, 12, 25], None, None)
    with pytest.raises(ValueError, match="ascending"):
        t.replacement_from_device([2, 1], [0, 14, 26], None, None)
    with pytest.raises(ValueError, match="ascending"):
        t.replacement_from_device([1, 4], [0, 12, 22], None, None)
    with pytest.raises(ValueError, match="offsets"):
        t.replacement_from_device([1, 2], [0, 12], None, None)
    with pytest.raises(AssertionError, match="nothing may be built"):  # past the checks
        t.replacement_from_device([1, 2], [0, 12, 26], None, None)


def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import base_config
    from rx.envs import MultiRacingEnv
    from rx.track_evolve_episodic import EpisodicEvolvingCurriculumPPO as PPO
    from rx.track_replay_episodic import EpisodicReplayCurriculumPPO

    def env_fn(i):
        raise AssertionError("no env may be built")
    assert issubclass(PPO, EpisodicReplayCurriculumPPO)
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        PPO(env_fn, base_config(num_envs=64, num_steps=16))
    monkeypatch.setattr(rdist, "world", lambda: 1)
    with pytest.raises(ValueError, match="two-car"):
        PPO(lambda i: MultiRacingEnv(num_agents=2, num_sensors=11), base_config(num_envs=64, num_steps=16))
    for bad in (-0.1, 1.5, NAN):
        with pytest.raises(ValueError, match="evolve_edit"):
            PPO(env_fn, base_config(num_envs=64, num_steps=16, evolve_edit=bad))
    with pytest.raises(ValueError, match="episodic_partial"):
        PPO(env_fn, base_config(num_envs=64, num_steps=16, episodic_partial=False))
    for key, bad in (("episodic_scores_every", 0), ("replay_power", 11), ("replay_kind", "advantage"),
                     ("curriculum_refresh", 1.5)):  # the parents' keys keep their checks
        with pytest.raises(ValueError, match=key):
            PPO(env_fn, base_config(num_envs=64, num_steps=16, episodic_partial=True, **{key: bad}))


def test_the_default_hooks_are_the_host_spawn():
    """EpisodicCurriculumPPO._replace_retired is what _resample_partial always did: spawn_same_points of the
    retired slots' own point counts at the generation, replace_tracks, the host copy of the pool."""
    from rx.track_episodic import EpisodicCurriculumPPO, spawn_same_points

    class Envs:
        def replace_tracks(self, slots, cps, widths):
            self.got = (list(slots), cps, widths)
            return "obs", "mask"

    class Stub(EpisodicCurriculumPPO):
        def __init__(self):
            self.config, self.envs = {"seed": 11}, Envs()
            self._cps, self._widths = [np.zeros((10 + k % 5, 2)) for k in range(6)], [6] * 6

    t = Stub()
    assert t._before_retire(3, np.array([1, 4])) is None
    assert t._replace_retired(3, np.array([1, 4])) == ("obs", "mask")
    cps, widths = spawn_same_points(11, 3, [11, 14])
    slots, got_cps, got_widths = t.envs.got
    assert slots == [1, 4] and got_widths == widths and [len(c) for c in got_cps] == [11, 14]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cps, got_cps))
    assert t._cps[1].tobytes() == cps[0].tobytes() and t._cps[4].tobytes() == cps[1].tobytes()
    assert t._widths == [6, widths[0], 6, 6, widths[1], 6]


def test_curriculum_train_takes_evolve_on_the_partial_path_only():
    tool = os.path.join(ROOT, "tools", "curriculum_train.py")
    p = subprocess.run([sys.executable, tool, "--episodic", "--evolve"], capture_output=True, text=True)
    assert p.returncode != 0 and "--partial" in p.stderr and "point count" in p.stderr, p.stderr
    p = subprocess.run([sys.executable, tool, "--partial", "--evolve"], capture_output=True, text=True)
    assert p.returncode != 0 and "--episodic" in p.stderr, p.stderr
    src = open(tool).read()
    assert "EpisodicEvolvingCurriculumPPO" in src
