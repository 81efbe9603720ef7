"""The culling tables of a track table (rx_build_cull_tables_host, csrc/rx_cull.h:
the rules rx_upload_tracks derives its tables by) against a NumPy restatement
written from include/rx.h's description of the tables, not from the library.
Everything is equal by value (a min of +0.0 and -0.0 may keep either zero), the
header rows decoded as int32[8] + f64[12].  One column is not an exact function
of the inputs: the circle radius (slot_geo[:, 2] and its copy in the row) goes
through hypot, so it is held to an upper bound of the largest np.hypot distance
and to 1e-13 relative of max_hypot * (1 + 1e-12) + 1e-9 -- a tenth of the
round-up slack the rule itself applies, orders of magnitude above a hypot's error.

Also: the argument refusals (before any HIP call: they run on a machine with no
GPU), and gen_tracks' ``rng`` argument.  tests/test_cull_tables_gpu.py holds the
kernel to this host twin on the same inputs.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 12345.0
WS_MIXED = (2, 7, 8, 9, 33, 450, 2048)  # every offset non-trivial; 2048 = the limit (64 x 8 x 4)
PARAMS = ((8, 8), (8, 0), (5, 3), (1, 1), (0, 8))  # (cull_chunk, cull_super)
WP_CHUNK, WP_SUPER = 8, 4
DTYPES = dict(chunk_off=np.int32, super_off=np.int32, wchunk_off=np.int32, wsuper_off=np.int32,
              chunk_box=np.float64, super_box=np.float64, wchunk_box=np.float64, wsuper_box=np.float64,
              slot_geo=np.float64, chunk_box_f=np.float32, super_box_f=np.float32, seg_f=np.float32,
              slot_hdr=np.float64)  # slot_hdr: 16 doubles = 128 bytes per row


def make_table(ws, seed):
    """A table of random finite doubles with slots of the given waypoint counts.
    Some coordinates are exact float32 values (integers: the outward rounding must
    not step them), some are tiny or large (many binades), a few are zeros of both
    signs."""
    rng = np.random.RandomState(seed)
    wp_off = np.concatenate([[0], np.cumsum(ws)]).astype(np.int32)
    wt, n = int(wp_off[-1]), len(ws)
    wp = rng.uniform(-120.0, 120.0, (wt, 2))
    seg = np.concatenate([rng.uniform(-120.0, 120.0, (2 * wt, 2)), rng.uniform(-6.0, 6.0, (2 * wt, 2))], axis=1)
    for a in (wp, seg):
        flat = a.reshape(-1)
        pick = rng.permutation(flat.size)
        q = flat.size // 8
        flat[pick[:q]] = np.round(flat[pick[:q]])                     # exact in float32
        flat[pick[q:2 * q]] *= 10.0 ** rng.randint(-6, 4, size=q)     # other binades
        flat[pick[2 * q:2 * q + 4]] = (0.0, -0.0, 0.0, -0.0)
    meta = rng.uniform(-50.0, 50.0, (n, 8))
    meta[:, 3] = rng.uniform(4.0, 10.0, n)     # width
    meta[:, 4] = rng.uniform(50.0, 300.0, n)   # max_track_distance
    meta[:, 7] = 0.0
    return dict(wp_off=wp_off, wp=np.ascontiguousarray(wp), seg=np.ascontiguousarray(seg), meta=meta)


TABLES = {"mixed": lambda: make_table(WS_MIXED, 1)}


def np_counts(wp_off, G, SG):
    """Per slot (leaf, super, wchunk, wsuper) box counts, from rx.h's description."""
    W = np.diff(wp_off).astype(np.int64)
    if G <= 0:
        return np.zeros((len(W), 4), np.int64)
    nch = -(-W // G)
    nwc = -(-W // WP_CHUNK)
    return np.stack([2 * nch, 2 * (-(-nch // SG)) if SG > 0 else 0 * W, nwc, -(-nwc // WP_SUPER)], axis=1)


def _box(pts):
    return np.array([pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()])


def _union(boxes):
    b = np.asarray(boxes)
    return np.array([b[:, 0].min(), b[:, 1].min(), b[:, 2].max(), b[:, 3].max()])


def _outward_f32(b):
    """[m][4] f64 boxes -> float32, min corner towards -inf, max corner towards +inf."""
    f = b.astype(np.float32)
    lo, hi = np.float32(-np.inf), np.float32(np.inf)
    back = f.astype(np.float64)
    for c in (0, 1):
        f[:, c] = np.where(back[:, c] > b[:, c], np.nextafter(f[:, c], lo), f[:, c])
    for c in (2, 3):
        f[:, c] = np.where(back[:, c] < b[:, c], np.nextafter(f[:, c], hi), f[:, c])
    assert np.all(f[:, :2].astype(np.float64) <= b[:, :2]) and np.all(f[:, 2:].astype(np.float64) >= b[:, 2:])
    return f


def _quadrant_blocks(f):
    """[m][4] float boxes -> [5][m][4]: the boxes, then per quadrant q (near.x, near.y, far.x, far.y)."""
    out = [f]
    for q in range(4):
        nx, fx = (2, 0) if q & 1 else (0, 2)
        ny, fy = (3, 1) if q & 2 else (1, 3)
        out.append(f[:, [nx, ny, fx, fy]])
    return np.stack(out)


def np_tables(t, G, SG):
    """The NumPy restatement of include/rx.h's rx_cull_tables.  Also returns
    max_hypot [n]: the largest np.hypot distance from the circle centre to a
    segment end point (the radius rule's input)."""
    wp_off, wp, seg, meta = t["wp_off"], t["wp"], t["seg"], t["meta"]
    n = len(wp_off) - 1
    cnt = np_counts(wp_off, G, SG)
    offs = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(cnt, axis=0)]).astype(np.int32)
    out = dict(seg_f=seg.astype(np.float32))
    hdr_i = np.zeros((n, 8), np.int32)
    hdr_f = np.zeros((n, 12))
    hdr_i[:, 0], hdr_i[:, 1] = wp_off[:-1], np.diff(wp_off)
    hdr_f[:, 4:] = meta
    out["hdr_i"], out["hdr_f"] = hdr_i, hdr_f
    if G <= 0:
        return out, None
    hdr_i[:, 2:6] = offs[:-1]
    leaf, sup, wch, wsu, geo, reach = [], [], [], [], np.zeros((n, 4)), np.zeros(n)
    for k in range(n):
        a, W = int(wp_off[k]), int(wp_off[k + 1] - wp_off[k])
        s = seg[2 * a:2 * (a + W)]
        starts, ends = s[:, :2], s[:, :2] + s[:, 2:]
        nch = -(-W // G)
        mine = []
        for side in range(2):
            for c in range(nch):
                rows = slice(side * W + c * G, side * W + min(W, (c + 1) * G))
                mine.append(_box(np.concatenate([starts[rows], ends[rows]])))
        leaf += mine
        if SG > 0:
            for side in range(2):
                for u in range(-(-nch // SG)):
                    sup.append(_union(mine[side * nch + u * SG:side * nch + min(nch, (u + 1) * SG)]))
        w = wp[a:a + W]
        wmine = [_box(w[c * WP_CHUNK:min(W, (c + 1) * WP_CHUNK)]) for c in range(-(-W // WP_CHUNK))]
        wch += wmine
        wsu += [_union(wmine[u * WP_SUPER:(u + 1) * WP_SUPER]) for u in range(-(-len(wmine) // WP_SUPER))]
        allb = _box(np.concatenate([starts, ends]))
        cx, cy = 0.5 * (allb[0] + allb[2]), 0.5 * (allb[1] + allb[3])
        reach[k] = max(np.hypot(starts[:, 0] - cx, starts[:, 1] - cy).max(),
                       np.hypot(ends[:, 0] - cx, ends[:, 1] - cy).max())
        longest = np.sqrt(s[:, 2] * s[:, 2] + s[:, 3] * s[:, 3]).max()
        geo[k] = (cx, cy, reach[k] * (1.0 + 1e-12) + 1e-9, longest * (1.0 + 1e-12) + 1e-12)
    if SG == 0:
        hdr_i[:, 3] = 0
    hdr_f[:, :4] = geo
    out.update(chunk_off=offs[:, 0], wchunk_off=offs[:, 2], wsuper_off=offs[:, 3], chunk_box=np.array(leaf),
               wchunk_box=np.array(wch), wsuper_box=np.array(wsu), slot_geo=geo,
               chunk_box_f=_quadrant_blocks(_outward_f32(np.array(leaf))))
    if SG > 0:
        out.update(super_off=offs[:, 1], super_box=np.array(sup),
                   super_box_f=_quadrant_blocks(_outward_f32(np.array(sup))))
    return out, reach


def sizes(t, G, SG):
    """rx_cull_table_sizes -> (leaf, super, wchunk, wsuper)."""
    from rx import _lib
    L = _lib.load()
    out = np.zeros(4, np.int64)
    _lib.check(L.rx_cull_table_sizes(len(t["wp_off"]) - 1, _lib.ptr(t["wp_off"]), G, SG, _lib.ptr(out)),
               "rx_cull_table_sizes")
    return tuple(int(x) for x in out)


def buffer_sizes(t, G, SG):
    """Elements of every output buffer the builders write for (G, SG); the others stay null."""
    n, wt = len(t["wp_off"]) - 1, int(t["wp_off"][-1])
    leaf, sup, wch, wsu = sizes(t, G, SG)
    s = dict(seg_f=8 * wt, slot_hdr=16 * n)
    if G > 0:
        s.update(chunk_off=n + 1, wchunk_off=n + 1, wsuper_off=n + 1, chunk_box=4 * leaf, wchunk_box=4 * wch,
                 wsuper_box=4 * wsu, slot_geo=4 * n, chunk_box_f=20 * leaf)
        if SG > 0:
            s.update(super_off=n + 1, super_box=4 * sup, super_box_f=20 * sup)
    return s


def tables_struct(bufs):
    from rx import _lib
    return _lib.RxCullTables(*[_lib.ptr(bufs.get(k)) for k in _lib.CULL_FIELDS])


def host_build(t, G, SG):
    """rx_build_cull_tables_host into guarded buffers -> {field: array with its guard element}."""
    from rx import _lib
    L = _lib.load()
    bufs = {k: np.full(m + 1, GUARD, DTYPES[k]) for k, m in buffer_sizes(t, G, SG).items()}
    st = tables_struct(bufs)
    _lib.check(L.rx_build_cull_tables_host(len(t["wp_off"]) - 1, _lib.ptr(t["wp_off"]), _lib.ptr(t["wp"]),
                                           _lib.ptr(t["seg"]), _lib.ptr(t["meta"]), G, SG, ctypes.byref(st), None),
               "rx_build_cull_tables_host")
    return bufs


def decode(bufs):
    """Guards checked and stripped; the header rows split into int32[8] + f64[12]."""
    out = {}
    for k, a in bufs.items():
        assert a[-1] == DTYPES[k](GUARD), f"{k}: the element past the table was written"
        out[k] = a[:-1]
    rows = out.pop("slot_hdr").reshape(-1, 16)
    out["hdr_i"] = np.ascontiguousarray(rows[:, :4]).view(np.int32).reshape(-1, 8)
    out["hdr_f"] = rows[:, 4:]
    return out


def check_radius(got, reach, what):
    """The radius rule: an upper bound of the largest np.hypot distance, within
    1e-13 relative of max_hypot * (1 + 1e-12) + 1e-9."""
    want = reach * (1.0 + 1e-12) + 1e-9
    rel = np.abs(got - want) / want
    print(f"{what}: radius max rel. deviation {rel.max():.3e}")
    assert np.all(got >= reach), what
    assert np.all(rel <= 1e-13), (what, rel.max())


def check_against(got, want, reach, what):
    """`got` (decoded tables) equals `want` by value; radius columns by the rule."""
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want)))
    for k in want:
        g, w = got[k].reshape(np.shape(want[k])), np.asarray(want[k])
        if reach is not None and k in ("slot_geo", "hdr_f"):
            g, w = g.reshape(len(reach), -1), w.reshape(len(reach), -1)
            check_radius(g[:, 2], reach, f"{what} {k}")
            g, w = np.delete(g, 2, axis=1), np.delete(w, 2, axis=1)
        assert g.dtype == w.dtype or k.endswith("_off"), (what, k, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, k)
        assert not np.any(np.isnan(g)), (what, k)


@pytest.mark.parametrize("G,SG", PARAMS)
def test_host_twin_equals_the_numpy_restatement(G, SG):
    t = TABLES["mixed"]()
    want, reach = np_tables(t, G, SG)
    got = decode(host_build(t, G, SG))
    check_against(got, want, reach, f"mixed G={G} SG={SG}")
    if G > 0:
        assert np.all(got["hdr_i"][:, 6:] == 0)
        assert got["chunk_off"][-1] * 20 == got["chunk_box_f"].size


@pytest.mark.parametrize("G,SG", PARAMS)
def test_table_sizes_agree_with_the_restatement(G, SG):
    t = TABLES["mixed"]()
    assert sizes(t, G, SG) == tuple(int(x) for x in np_counts(t["wp_off"], G, SG).sum(0))


def _call(fn, t, G=8, SG=8, bufs=None, drop=(), out_null=False):
    """One builder call with some arguments nulled -> (rc, message)."""
    from rx import _lib
    L = _lib.load()
    if bufs is None:
        bufs = {k: np.zeros(64, DTYPES[k]) for k in DTYPES}  # never reached: every call here is refused
    st = tables_struct({k: v for k, v in bufs.items() if k not in drop})
    arg = lambda k: None if k in drop else _lib.ptr(t[k])  # noqa: E731
    rc = getattr(L, fn)(len(t["wp_off"]) - 1, arg("wp_off"), arg("wp"), arg("seg"), arg("meta"), G, SG,
                        None if out_null else ctypes.byref(st), None)
    return rc, L.rx_last_error().decode()


@pytest.mark.parametrize("fn", ["rx_build_cull_tables_host", "rx_build_cull_tables"])
def test_bad_arguments_are_refused_before_any_hip_call(fn):
    """Both builders check everything first, so the device one refuses on a
    machine with no GPU exactly as the host one does."""
    from rx import _lib
    ok = make_table((4, 5), 2)
    for k in ("wp_off", "wp", "seg", "meta"):
        rc, msg = _call(fn, ok, drop=(k,))
        assert rc == _lib.RX_EINVAL and k in msg and "null" in msg, (k, msg)
    rc, msg = _call(fn, ok, out_null=True)
    assert rc == _lib.RX_EINVAL and "out" in msg
    for k in DTYPES:
        rc, msg = _call(fn, ok, drop=(k,))
        assert rc == _lib.RX_EINVAL and k in msg, (k, msg)
    # what (G, SG) does not write may be null: the first complaint is about something else
    rc, msg = _call(fn, ok, G=8, SG=0, drop=("super_off", "super_box", "super_box_f", "wp"))
    assert rc == _lib.RX_EINVAL and "wp is null" in msg
    bad = dict(ok, wp_off=np.array([1, 4, 9], np.int32))
    rc, msg = _call(fn, bad)
    assert rc == _lib.RX_EINVAL and "wp_off[0]" in msg
    bad = dict(ok, wp_off=np.array([0, 8, 9], np.int32))
    rc, msg = _call(fn, bad)
    assert rc == _lib.RX_EINVAL and "track 1" in msg and "W = 1" in msg
    bad = dict(ok, wp_off=np.array([0, 2049, 2054], np.int32))
    rc, msg = _call(fn, bad)
    assert rc == _lib.RX_EINVAL and "track 0" in msg and "W = 2049" in msg
    for sg in (-1, 65):
        rc, msg = _call(fn, ok, SG=sg)
        assert rc == _lib.RX_EINVAL and "cull_super" in msg
    L = _lib.load()
    assert L.rx_cull_table_sizes(2, _lib.ptr(ok["wp_off"]), 8, 65, _lib.ptr(np.zeros(4, np.int64))) == _lib.RX_EINVAL
    assert L.rx_cull_table_sizes(0, _lib.ptr(ok["wp_off"]), 8, 8, _lib.ptr(np.zeros(4, np.int64))) == _lib.RX_EINVAL


def test_upload_tracks_device_refuses_a_null_handle():
    from rx import _lib
    L = _lib.load()
    t = make_table((4, 5), 2)
    rc = L.rx_upload_tracks_device(None, 2, _lib.ptr(t["wp_off"]), _lib.ptr(t["wp"]), _lib.ptr(t["wp"]),
                                   _lib.ptr(t["seg"]), _lib.ptr(t["meta"]), None)
    assert rc == _lib.RX_EINVAL and b"null handle" in L.rx_last_error()


@pytest.mark.parametrize("seed", [None, 3])
def test_gen_tracks_draws_from_a_random_state(seed):
    """gen_tracks(n, rng=RandomState(s)) == np.random.seed(s); gen_tracks(n), array
    for array, with the global stream left where it was."""
    from rx.track import gen_random_track, gen_tracks
    np.random.seed(4)
    want = gen_tracks(12, seed=seed)
    after = np.random.get_state()
    np.random.seed(99)
    before = np.random.get_state()
    rng = np.random.RandomState(4)
    got = gen_tracks(12, seed=seed, rng=rng)
    now = np.random.get_state()
    assert len(got) == len(want) == 12 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert now[0] == before[0] and np.array_equal(now[1], before[1]) and now[2:] == before[2:]
    assert np.array_equal(rng.get_state()[1], after[1]) and rng.get_state()[2] == after[2]
    np.random.seed(8)
    one = gen_random_track(11, 60, 12, 0.3, 0.4)
    assert np.array_equal(gen_random_track(11, 60, 12, 0.3, 0.4, rng=np.random.RandomState(8)), one)


def test_abi_stays_25_and_the_new_names_are_declared_and_exported():
    from rx import _build, _lib
    assert _lib.ABI_VERSION == 25 and _lib.load().rx_abi_version() == 25
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert re.search(r"#define RX_ABI_VERSION 25\b", src)
    lib = ctypes.CDLL(_build.LIB)
    for name in ("rx_cull_table_sizes", "rx_build_cull_tables", "rx_build_cull_tables_host",
                 "rx_upload_tracks_device"):
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert "rx_cull.hip" in _build.SOURCES and "rx_cull.h" in _build.HEADERS
    assert ctypes.sizeof(_lib.RxCullTables) == 13 * ctypes.sizeof(ctypes.c_void_p)
