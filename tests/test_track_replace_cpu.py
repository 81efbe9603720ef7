"""Slots replaced in place, on the host (rx_patch_tracks_host, include/rx.h): a
patched table and its patched culling tables equal, byte for byte and guards
included, the from-scratch host build (rx_build_cull_tables_host) of the updated
pool; the offset arrays stay; a refused patch leaves every destination byte as it
was.  Also the argument refusals of the device form (before any HIP call: they run
on a machine with no GPU), the three new names in the ABI, and the fresh draw of the
partial episodic trainers (rx.track_episodic.spawn_same_points), which needs no
device.  tests/test_track_replace_gpu.py holds the kernel to this twin.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_cull_tables_cpu import DTYPES, GUARD, PARAMS, buffer_sizes, make_table, tables_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("wp", "nrm", "seg", "meta")
WS9 = [(3, 4, 6, 10)[k % 4] for k in range(9)]
WS_WIDE = [5, 2048, 7, 3, 9]  # the largest slot the tables allow beside the smallest of the pools here
LISTS9 = ([0], [8], [0, 4, 8], list(range(9)))  # 8 owns the offset arrays' last entries


def table_with_nrm(ws, seed):
    """make_table plus the nrm rows it leaves out (a patch copies them), every table array guarded."""
    t = make_table(ws, seed)
    t["nrm"] = np.random.RandomState(seed + 1000).uniform(-1.0, 1.0, t["wp"].shape)
    return t


def guarded(t):
    """The four table arrays flattened, each with a guard element past its end."""
    return {k: np.concatenate([t[k].reshape(-1), [GUARD]]) for k in KEYS}


def updated(t, slots, src):
    """The pool after the patch, written in NumPy: source track j over slot slots[j]."""
    u = {k: t[k].copy() for k in t}
    for j, k in enumerate(slots):
        a, b = int(t["wp_off"][k]), int(t["wp_off"][k + 1])
        sa, sb = int(src["wp_off"][j]), int(src["wp_off"][j + 1])
        u["wp"][a:b], u["nrm"][a:b] = src["wp"][sa:sb], src["nrm"][sa:sb]
        u["seg"][2 * a:2 * b] = src["seg"][2 * sa:2 * sb]
        u["meta"][k] = src["meta"][j]
    return u


def cull_build(fn, t, G, SG, arrays=None, stream=None, full=np.full):
    """A from-scratch culling-table build into guarded buffers (host arrays, or whatever ``full`` makes)."""
    from rx import _lib
    L = _lib.load()
    bufs = {k: full(m + 1, GUARD, DTYPES[k]) for k, m in buffer_sizes(t, G, SG).items()}
    st = tables_struct(bufs)
    a = arrays if arrays is not None else t
    _lib.check(getattr(L, fn)(len(t["wp_off"]) - 1, _lib.ptr(t["wp_off"]), _lib.ptr(a["wp"]), _lib.ptr(a["seg"]),
                              _lib.ptr(a["meta"]), G, SG, ctypes.byref(st), stream), fn)
    return bufs


def patch_struct(slots, src, n_upd=None, drop=()):
    """(rx_track_patch, the arrays it points to)."""
    from rx import _lib
    keep = dict(slots=np.ascontiguousarray(slots, dtype=np.int32), src_off=src["wp_off"], wp=src["wp"], nrm=src["nrm"],
                seg=src["seg"], meta=src["meta"])
    p = _lib.RxTrackPatch(len(slots) if n_upd is None else n_upd,
                          *[None if k in drop else _lib.ptr(keep[k]) for k in _lib.PATCH_FIELDS])
    return p, keep


def call_patch(fn, t, dst, G, SG, bufs, p, stream=None, drop=()):
    """One patch call on the destination arrays ``dst`` and tables ``bufs`` (None: t = NULL) -> (rc, message)."""
    from rx import _lib
    L = _lib.load()
    st = tables_struct(bufs) if bufs is not None else None
    arg = lambda k: None if k in drop else _lib.ptr(dst[k])  # noqa: E731
    rc = getattr(L, fn)(len(t["wp_off"]) - 1, None if "wp_off" in drop else _lib.ptr(t["wp_off"]), arg("wp"),
                        arg("nrm"), arg("seg"), arg("meta"), G, SG, ctypes.byref(st) if st is not None else None,
                        ctypes.byref(p) if p is not None else None, stream)
    return rc, L.rx_last_error().decode()


def assert_same_bytes(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def _patched_equals_rebuild(ws, lists, G, SG, seed):
    from rx import _lib
    t = table_with_nrm(ws, seed)
    before = cull_build("rx_build_cull_tables_host", t, G, SG)
    for slots in lists:
        src = table_with_nrm([ws[k] for k in slots], seed + 50 + len(slots))
        dst, bufs = guarded(t), {k: v.copy() for k, v in before.items()}
        p, keep = patch_struct(slots, src)
        rc, msg = call_patch("rx_patch_tracks_host", t, dst, G, SG, bufs, p)
        assert rc == _lib.RX_OK, msg
        u = updated(t, slots, src)
        what = f"ws={ws[:4]}.. slots={slots} G={G} SG={SG}"
        assert_same_bytes(dst, guarded(u), what)
        assert_same_bytes(bufs, cull_build("rx_build_cull_tables_host", u, G, SG), what)
        for k in bufs:
            if k.endswith("_off"):
                assert bufs[k].tobytes() == before[k].tobytes(), (what, k)
        if len(slots) < len(ws):  # the patch did something, and only there
            assert dst["wp"].tobytes() != guarded(t)["wp"].tobytes()
            assert bufs["seg_f"].tobytes() != before["seg_f"].tobytes()


@pytest.mark.parametrize("G,SG", PARAMS)
def test_patched_tables_are_the_rebuilt_tables_bytes(G, SG):
    _patched_equals_rebuild(WS9, LISTS9, G, SG, 11)


@pytest.mark.parametrize("G,SG", PARAMS)
def test_the_widest_and_the_narrowest_slot(G, SG):
    _patched_equals_rebuild(WS_WIDE, ([1], [3], [1, 3]), G, SG, 12)


def test_without_tables_only_the_four_arrays_change():
    from rx import _lib
    t = table_with_nrm(WS9, 13)
    slots = [0, 4, 8]
    src = table_with_nrm([WS9[k] for k in slots], 14)
    dst = guarded(t)
    p, keep = patch_struct(slots, src)
    rc, msg = call_patch("rx_patch_tracks_host", t, dst, 8, 8, None, p)  # G and SG are not looked at
    assert rc == _lib.RX_OK, msg
    assert_same_bytes(dst, guarded(updated(t, slots, src)), "t = NULL")
    rc, msg = call_patch("rx_patch_tracks_host", t, dst, 8, 65, None, p)
    assert rc == _lib.RX_OK, msg


def _bad_patches():
    """name -> (slots, source waypoint counts, what to break, what the message must say)."""
    return {
        "w_mismatch": ([0, 4], [3, 4], None, (r"slot 4\b", "waypoint count")),
        "slot_out_of_range": ([0, 9], [3, 4], None, (r"slot 9\b", "slots")),
        "slot_negative": ([-1, 4], [3, 3], None, (r"slot -1\b", "slots")),
        "descending": ([4, 0], [3, 3], None, (r"slot 0\b", "ascending")),
        "repeated": ([4, 4], [3, 3], None, (r"slot 4\b", "distinct")),
        "n_upd_0": ([0], [3], dict(n_upd=0), ("n_upd",)),
        "n_upd_above": ([0], [3], dict(n_upd=10), ("n_upd",)),
        "src_off0": ([0], [3], dict(src_off0=1), (r"src_off\[0\]",)),
    }


@pytest.mark.parametrize("fn", ["rx_patch_tracks_host", "rx_patch_tracks"])
@pytest.mark.parametrize("case", list(_bad_patches()))
def test_bad_patches_are_refused_before_any_write_or_hip_call(fn, case):
    """Both forms check the same things first, so the device form refuses on a machine
    with no GPU exactly as the host one does (its pointers are never followed)."""
    from rx import _lib
    slots, src_ws, how, says = _bad_patches()[case]
    t = table_with_nrm(WS9, 15)
    src = table_with_nrm(src_ws, 16)
    how = how or {}
    if "src_off0" in how:
        src["wp_off"] = src["wp_off"] + np.int32(how["src_off0"])
    dst, bufs = guarded(t), cull_build("rx_build_cull_tables_host", t, 8, 8)
    dst0, bufs0 = {k: v.copy() for k, v in dst.items()}, {k: v.copy() for k, v in bufs.items()}
    p, keep = patch_struct(slots, src, n_upd=how.get("n_upd"))
    rc, msg = call_patch(fn, t, dst, 8, 8, bufs, p)
    assert rc == _lib.RX_EINVAL, (case, rc, msg)
    for pat in says:
        assert re.search(pat, msg), (case, msg)
    assert_same_bytes(dst, dst0, case)
    assert_same_bytes(bufs, bufs0, case)


@pytest.mark.parametrize("col,value,says", [(4, np.nan, "max_track_distance"), (4, 0.0, "max_track_distance"),
                                            (3, -1.0, "width"), (3, np.nan, "width")])
def test_the_host_twin_refuses_a_bad_source_track(col, value, says):
    from rx import _lib
    t = table_with_nrm(WS9, 17)
    slots = [2, 5]
    src = table_with_nrm([WS9[k] for k in slots], 18)
    src["meta"][1, col] = value
    dst, bufs = guarded(t), cull_build("rx_build_cull_tables_host", t, 5, 3)
    dst0, bufs0 = {k: v.copy() for k, v in dst.items()}, {k: v.copy() for k, v in bufs.items()}
    p, keep = patch_struct(slots, src)
    rc, msg = call_patch("rx_patch_tracks_host", t, dst, 5, 3, bufs, p)
    assert rc == _lib.RX_EINVAL and re.search(r"slot 5\b", msg) and says in msg, msg
    assert_same_bytes(dst, dst0, says)
    assert_same_bytes(bufs, bufs0, says)


@pytest.mark.parametrize("fn", ["rx_patch_tracks_host", "rx_patch_tracks"])
def test_null_pointers_and_table_limits_are_refused(fn):
    from rx import _lib
    t = table_with_nrm(WS9, 19)
    src = table_with_nrm([3], 20)
    dst, bufs = guarded(t), cull_build("rx_build_cull_tables_host", t, 8, 8)
    p, keep = patch_struct([0], src)
    for k in ("wp_off",) + KEYS:
        rc, msg = call_patch(fn, t, dst, 8, 8, bufs, p, drop=(k,))
        assert rc == _lib.RX_EINVAL and k in msg and "null" in msg, (k, msg)
    rc, msg = call_patch(fn, t, dst, 8, 8, bufs, None)
    assert rc == _lib.RX_EINVAL and "patch" in msg and "null" in msg, msg
    for k in _lib.PATCH_FIELDS:
        q, keep_q = patch_struct([0], src, drop=(k,))
        rc, msg = call_patch(fn, t, dst, 8, 8, bufs, q)
        assert rc == _lib.RX_EINVAL and f"patch->{k}" in msg and "null" in msg, (k, msg)
    rc, msg = call_patch(fn, t, dst, 8, 8, {k: v for k, v in bufs.items() if k != "seg_f"}, p)
    assert rc == _lib.RX_EINVAL and "seg_f" in msg, msg
    rc, msg = call_patch(fn, t, dst, 8, 65, bufs, p)
    assert rc == _lib.RX_EINVAL and "cull_super" in msg, msg
    bad = dict(t, wp_off=t["wp_off"] + np.int32(1))
    rc, msg = call_patch(fn, bad, dst, 8, 8, bufs, p)
    assert rc == _lib.RX_EINVAL and "wp_off[0]" in msg, msg


def test_replace_tracks_device_refuses_a_null_handle():
    from rx import _lib
    L = _lib.load()
    p, keep = patch_struct([0], table_with_nrm([3], 21))
    assert L.rx_replace_tracks_device(None, ctypes.byref(p), None) == _lib.RX_EINVAL
    assert b"null handle" in L.rx_last_error()


def test_abi_stays_25_and_the_new_names_are_declared_and_exported():
    from rx import _build, _lib
    assert _lib.ABI_VERSION == 25 and _lib.load().rx_abi_version() == 25
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    lib = ctypes.CDLL(_build.LIB)
    for name in ("rx_patch_tracks", "rx_patch_tracks_host", "rx_replace_tracks_device"):
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert "typedef struct rx_track_patch" in src
    assert ctypes.sizeof(_lib.RxTrackPatch) == 7 * ctypes.sizeof(ctypes.c_void_p)  # int32 + padding, six pointers


# ---------------------------------------------------------------- the partial trainers' fresh draw
def test_spawn_same_points_keeps_every_slots_point_count():
    """A 12-slot pool with point counts 10..14: every retired slot gets a track of its
    own point count, a function of (seed, generation) only, from the RandomState
    CurriculumPPO._spawn_tracks uses, and np.random does not move."""
    from rx.track import _draw_params, gen_random_track
    from rx.track_episodic import spawn_same_points
    counts = [10 + k % 5 for k in range(12)]
    retired = [1, 4, 7, 8, 11]
    np.random.seed(5)
    before = np.random.get_state()
    cps, widths = spawn_same_points(3, 2, [counts[k] for k in retired])
    now = np.random.get_state()
    assert now[0] == before[0] and np.array_equal(now[1], before[1]) and now[2:] == before[2:]
    assert [len(c) for c in cps] == [counts[k] for k in retired] and len(widths) == len(retired)
    assert all(c.shape == (counts[k], 2) and np.isfinite(c).all() for c, k in zip(cps, retired))
    assert all(isinstance(w, int) and 6 <= w < 10 for w in widths)
    again = spawn_same_points(3, 2, [counts[k] for k in retired])
    assert all(np.array_equal(a, b) for a, b in zip(cps, again[0])) and widths == again[1]
    for other in (spawn_same_points(4, 2, [counts[k] for k in retired]),
                  spawn_same_points(3, 3, [counts[k] for k in retired])):
        assert not any(np.array_equal(a, b) for a, b in zip(cps, other[0]))
    # the draws, restated: the parameters of gen_tracks with the drawn point count discarded
    rng = np.random.RandomState((3 + 7919 * 2) % 2 ** 32)
    for c, w, k in zip(cps, widths, retired):
        _, base, var, jit, smooth = _draw_params(rng)
        assert np.array_equal(c, gen_random_track(counts[k], base, var, jit, smooth, None, rng))
        assert w == int(rng.randint(6, 10))
