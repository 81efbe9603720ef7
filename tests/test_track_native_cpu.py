"""Track tables from librx's host builder (rx_build_tracks_host, ABI v24;
TrackSet backend="native") against the scipy geometry and the golden vectors.

Parity: scipy solves the periodic spline system through LAPACK,
so the native waypoints agree with TrackGeometry's to rounding, not bit for
bit.  Measured over np.random.seed(7); gen_tracks(3000, seed=None), the default
track and the golden tracks: max |native - scipy| = 6.4e-14 in waypoints
(coordinates up to ~150: 2-3 ulp).  WP_BOUND is 16x that.  Everything after the
waypoints -- normals, segments, all of meta -- is an exact function of them and
is compared byte for byte with TrackGeometry.from_waypoints.
"""
import ctypes

import numpy as np
import pytest

from rx.track import DEFAULT_CONTROL_POINTS, DEFAULT_WIDTH, TrackGeometry, TrackSet, build_table, gen_tracks

WP_BOUND = 16 * 6.4e-14


def _golden_inputs(golden):
    cps = [DEFAULT_CONTROL_POINTS if t["label"] == "default" else t["cp"] for t in golden.tracks]
    ws = [None if t["label"] == "default" else t["width"] for t in golden.tracks]
    return cps + [None], ws + [None]  # plus the default track as the envs pass it (integer points, width None)


def _pool192():
    np.random.seed(11)
    pool = gen_tracks(192, seed=None)
    return pool, [float(4 + k % 6) for k in range(192)]


def _slot_rows(g):
    """One slot as TrackSet._pack lays it out."""
    a = TrackSet._pack([g])
    return a["wp"], a["nrm"], a["seg"], a["meta"]


def _assert_exact_function_of_waypoints(ts, k):
    g = ts.geoms[k]
    ref = TrackGeometry.from_waypoints(g.control_points, g.track_width, g.waypoints)
    a = ts.arrays()
    s, e = a["wp_off"][k], a["wp_off"][k + 1]
    wp, nrm, seg, meta = _slot_rows(ref)
    assert a["wp"][s:e].tobytes() == wp.tobytes(), k
    assert a["nrm"][s:e].tobytes() == nrm.tobytes(), k
    assert a["seg"][2 * s:2 * e].tobytes() == seg.tobytes(), k
    assert a["meta"][k].tobytes() == meta[0].tobytes(), (k, a["meta"][k], meta[0])
    assert g.max_track_distance == ref.max_track_distance and g.track_bounds == ref.track_bounds
    assert np.array_equal(g.segment_cache["ends"], ref.segment_cache["ends"])


def test_from_waypoints_is_what_init_derives(golden):
    for t in golden.tracks[:4]:
        cp = DEFAULT_CONTROL_POINTS if t["label"] == "default" else t["cp"]
        g = TrackGeometry.from_waypoints(cp, t["width"], t["wp"])
        assert np.array_equal(g.normals, t["nrm"]) and np.array_equal(g.segment_cache["v2"], t["v2"])
        assert np.array_equal(g.segment_cache["starts"], t["starts"]) and g.max_track_distance == t["maxd"]


def test_native_golden_tracks(golden):
    cps, ws = _golden_inputs(golden)
    ts = TrackSet(backend="native")
    slots = [ts.slot(c, w) for c, w in zip(cps, ws)]
    dev = 0.0
    for i, t in enumerate(golden.tracks):
        d = np.abs(ts.geoms[slots[i]].waypoints - t["wp"]).max()
        dev = max(dev, d)
    print(f"max |native - golden| waypoints = {dev:.3e} (bound {WP_BOUND:.3e})")
    assert dev <= WP_BOUND
    k = slots[-1]  # the default track: integer control points, width None
    assert ts.geoms[k].track_width == DEFAULT_WIDTH
    assert np.abs(ts.geoms[k].waypoints - TrackGeometry().waypoints).max() <= WP_BOUND
    for k in range(len(ts)):
        _assert_exact_function_of_waypoints(ts, k)


def test_native_pool_of_192_against_scipy():
    pool, ws = _pool192()
    ts = TrackSet.build(pool, ws, backend="native")
    assert len(ts) == 192
    dev = 0.0
    for k, (c, w) in enumerate(zip(pool, ws)):
        ref = TrackGeometry(c, w)
        assert ref.waypoints.shape == ts.geoms[k].waypoints.shape
        dev = max(dev, np.abs(ts.geoms[k].waypoints - ref.waypoints).max())
        _assert_exact_function_of_waypoints(ts, k)
    print(f"max |native - scipy| waypoints = {dev:.3e} (bound {WP_BOUND:.3e})")
    assert dev <= WP_BOUND


def test_build_native_slots_dedup_and_packing():
    import random
    random.seed(1)
    np.random.seed(1)
    pool = gen_tracks(num_tracks=256, seed=1)
    widths = [np.random.randint(6, 10) for _ in range(256)]
    pool, widths = pool + [None], widths + [None]
    a = TrackSet.build(pool, widths)
    b = TrackSet.build(pool, widths, backend="native")
    assert len(a) == len(b) == 8  # the seed-1 pool's 7 slots and the default track
    assert a._index == b._index  # same keys -> same slot numbers, in first-sight order
    assert np.array_equal(a.arrays()["wp_off"], b.arrays()["wp_off"])
    for k in range(len(b)):
        assert np.array_equal(np.asarray(a.geoms[k].control_points), np.asarray(b.geoms[k].control_points))
        assert a.geoms[k].track_width == b.geoms[k].track_width
    # arrays() == packing the per-track native results
    per = TrackSet(backend="native")
    for k, g in enumerate(b.geoms):
        assert per.slot(g.control_points, g.track_width) == k
    assert per._packed is None
    pa, pb = per.arrays(), b.arrays()
    for key in ("wp_off", "wp", "nrm", "seg", "meta"):
        assert pa[key].dtype == pb[key].dtype and pa[key].tobytes() == pb[key].tobytes(), key
    assert TrackSet._pack(b.geoms)["meta"].tobytes() == pb["meta"].tobytes()
    # a pair the set already holds is looked up, not rebuilt
    assert b.slot(pool[3], widths[3]) == a.slot(pool[3], widths[3]) and len(b) == 8


def _circle(P, r=40.0):
    a = np.linspace(0, 2 * np.pi, P, endpoint=False)
    return np.column_stack([r * np.cos(a) + 3.0, r * np.sin(a) - 1.0])


@pytest.mark.parametrize("P,factor", [(3, 1), (64, 2), (12, 30)])
def test_edge_shapes_against_scipy(P, factor):
    cp = _circle(P)
    ts = TrackSet.build([cp], [5.0], factor=factor, backend="native")  # n_tracks = 1
    assert len(ts) == 1 and ts.geoms[0].waypoints.shape == (P * factor, 2)
    ref = TrackGeometry(cp, 5.0, factor)
    assert np.abs(ts.geoms[0].waypoints - ref.waypoints).max() <= WP_BOUND
    _assert_exact_function_of_waypoints(ts, 0)


@pytest.mark.parametrize("factor", [1, 2])
def test_sample_on_a_knot_belongs_to_the_interval_it_starts(factor):
    """A square of side 8: chords and knot parameters are exact, so every
    factor-th sample sits exactly on a knot and must be that control point
    (z = 0 in the interval the knot starts, not z = h at the end of the one before)."""
    cp = np.array([[0.0, 0.0], [8.0, 0.0], [8.0, 8.0], [0.0, 8.0]])
    a = build_table([cp], [1.0], factor=factor)
    assert np.array_equal(a["wp"][::factor], cp)
    assert np.abs(a["wp"] - TrackGeometry(cp, 1.0, factor).waypoints).max() <= WP_BOUND


def _call_host(cps, widths, factor):
    from rx import _lib
    L = _lib.load()
    n = len(cps)
    cp_off = np.concatenate([[0], np.cumsum([len(c) for c in cps])]).astype(np.int32)
    cp = np.ascontiguousarray(np.concatenate(cps), dtype=np.float64)
    w = np.asarray(widths, dtype=np.float64)
    wt = max(int(cp_off[-1]) * max(factor, 1), 1)
    out = [np.full(n + 1, -7, np.int32), np.full((wt, 2), 7.0), np.full((wt, 2), 7.0), np.full((2 * wt, 4), 7.0),
           np.full((n, 8), 7.0)]
    rc = L.rx_build_tracks_host(n, factor, _lib.ptr(cp_off), _lib.ptr(cp), _lib.ptr(w), *[_lib.ptr(o) for o in out],
                                None)
    return rc, L.rx_last_error().decode(), out


def test_validation_names_the_track_and_the_field():
    from rx import _lib
    good = _circle(10)
    rep = good.copy()
    rep[4] = rep[3]  # a repeated control point: a zero-length chord
    inf = good.copy()
    inf[7, 1] = np.inf
    nan = good.copy()
    nan[0, 0] = np.nan
    cases = [
        ([good, _circle(3)[:2]], [6, 6], 30, ("track 1", "P = 2")),
        ([_circle(65)], [6], 2, ("track 0", "P = 65")),
        ([good], [6], 0, ("factor",)),
        ([good, _circle(64)], [6, 6], 33, ("track 1", "W = ", "2112")),  # 64 * 33 > 2048
        ([good, good, rep], [6, 6, 6], 30, ("track 2", "chord 3")),
        ([good, inf], [6, 6], 30, ("track 1", "cp[7]", "non-finite")),
        ([nan], [6], 30, ("track 0", "cp[0]", "non-finite")),
        ([good, good], [6, -0.5], 30, ("track 1", "width")),
        ([good], [np.nan], 30, ("track 0", "width")),
    ]
    for cps, ws, factor, words in cases:
        rc, msg, out = _call_host(cps, ws, factor)
        assert rc == _lib.RX_EINVAL, (words, rc)
        for word in words:
            assert word in msg, (words, msg)
        for o in out[1:]:  # rejected before anything is written: no NaN-filled table
            assert np.all(o == 7.0), words
    rc, msg, out = _call_host([good], [0.0], 30)  # a zero width is a (degenerate) track, not an error
    assert rc == _lib.RX_OK and np.array_equal(out[0], [0, 300])
    with pytest.raises(_lib.RxError, match="chord 3"):
        TrackSet.build([good, rep], [6, 6], backend="native")
    with pytest.raises(_lib.RxError, match="chord 3"):
        TrackSet(backend="native").slot(rep, 6)
    with pytest.raises(ValueError, match="backend"):
        TrackSet(backend="numpy")
    L = _lib.load()
    assert L.rx_build_tracks_host(1, 30, None, None, None, None, None, None, None, None, None) == _lib.RX_EINVAL
    assert L.rx_build_tracks(0, 30, None, None, None, None, None, None, None, None, None) == _lib.RX_EINVAL
    # the device entry point checks what the offsets show before any HIP call
    off = np.array([0, 2], np.int32)
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    assert L.rx_build_tracks(1, 30, _lib.ptr(off), one, one, _lib.ptr(np.zeros(2, np.int32)), one, one, one, one,
                             None) == _lib.RX_EINVAL
    assert b"P = 2" in L.rx_last_error()


def test_native_table_file_roundtrip_and_tampering(golden, tmp_path):
    cps, ws = _golden_inputs(golden)
    ts = TrackSet.build(cps, ws, backend="native")
    toe = np.arange(len(cps), dtype=np.int32) % len(ts)
    p = tmp_path / "native.npz"
    ts.save(p, toe)
    with np.load(p) as z:
        assert str(z["backend"]) == "native"
    ld, toe2 = TrackSet.load(p, verify=True)
    assert ld.backend == "native" and np.array_equal(toe, toe2) and len(ld) == len(ts)
    for k in ts.arrays():
        assert ts.arrays()[k].tobytes() == ld.arrays()[k].tobytes(), k
    assert ld.slot(cps[2], ws[2]) == ts.slot(cps[2], ws[2]) and len(ld) == len(ts)
    # a slot added to a loaded native set comes from the native builder
    extra = _circle(9)
    k = ld.slot(extra, 5.0)
    assert ld.geoms[k].waypoints.tobytes() == build_table([extra], [5.0])["wp"].tobytes()
    d = dict(np.load(p))
    d["wp"] = d["wp"].copy()
    d["wp"][3, 0] += 1e-9
    np.savez(tmp_path / "bad.npz", **d)
    with pytest.raises(ValueError, match="slot 0"):
        TrackSet.load(tmp_path / "bad.npz", verify=True)
    TrackSet.load(tmp_path / "bad.npz")  # unverified loads take the table as it is
    # a "device" table verifies through the host twin (no GPU here)
    d = dict(np.load(p))
    d["backend"] = np.array("device")
    np.savez(tmp_path / "dev.npz", **d)
    assert TrackSet.load(tmp_path / "dev.npz", verify=True)[0].backend == "device"
    # a file without the key is a scipy table, as before: the native one does not verify as scipy
    d.pop("backend")
    np.savez(tmp_path / "old.npz", **d)
    assert TrackSet.load(tmp_path / "old.npz")[0].backend == "scipy"
    with pytest.raises(ValueError):
        TrackSet.load(tmp_path / "old.npz", verify=True)
    sc = TrackSet()
    sc.slot(cps[0], ws[0])
    sc.save(tmp_path / "sc.npz")
    d = dict(np.load(tmp_path / "sc.npz"))
    assert str(d.pop("backend")) == "scipy"
    np.savez(tmp_path / "sc_old.npz", **d)
    old, _ = TrackSet.load(tmp_path / "sc_old.npz", verify=True)
    assert old.backend == "scipy" and old.arrays()["wp"].tobytes() == sc.arrays()["wp"].tobytes()


def test_default_backend_is_still_the_reference_geometry(golden):
    """TrackSet() / TrackSet.build() without the keyword: the golden bytes."""
    cps, ws = _golden_inputs(golden)
    a = TrackSet()
    for c, w in zip(cps, ws):
        a.slot(c, w)
    b = TrackSet.build(cps, ws)
    assert a.backend == b.backend == "scipy"
    for ts in (a, b):
        arr = ts.arrays()
        for k, t in enumerate(golden.tracks):
            k = ts._index[TrackSet._key(cps[k], DEFAULT_WIDTH if ws[k] is None else ws[k])]
            s, e = arr["wp_off"][k], arr["wp_off"][k + 1]
            assert arr["wp"][s:e].tobytes() == t["wp"].tobytes()
            assert arr["nrm"][s:e].tobytes() == t["nrm"].tobytes()
            assert arr["seg"][2 * s:2 * e].tobytes() == np.concatenate([t["starts"], t["v2"]], 1).tobytes()
            assert arr["meta"][k, 4] == t["maxd"] and np.array_equal(arr["meta"][k, :3], t["start"])
    for key in a.arrays():
        assert a.arrays()[key].tobytes() == b.arrays()[key].tobytes()


def test_from_table_checks_the_requested_backend(tmp_path):
    """RacingVectorEnv.from_table(track_backend=...) refuses a table another
    builder made, before it touches the device."""
    from rx.vector_env import RacingVectorEnv
    ts = TrackSet.build([_circle(9)], [5.0], backend="native")
    ts.save(tmp_path / "t.npz", np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="native"):
        RacingVectorEnv.from_table(tmp_path / "t.npz", track_backend="scipy")
