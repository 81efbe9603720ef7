"""rx.render on the host backend against tests/raster_ref.py, an independent
NumPy restatement of the raster rules.  No GPU: the host twins
of the three raster kernels make no HIP call.

Sizes 128 and 99: 99 is no multiple of 4 (the row tail of the frame kernel and
its twin's plain loop) nor of the 16-pixel tile; at 64 and below the width-4
borders cover the whole track, so a wrong fill would be invisible."""
import ctypes
import functools

import numpy as np
import pytest

from rx import _lib, render
from rx.envs import MultiRacingEnv, RacingEnv
from tests import raster_ref as R

SIZES = (128, 99)


geoms = R.sample_geoms


@functools.lru_cache(maxsize=None)
def ref_layer(k, size):
    layer = R.static_layer(R.view(geoms()[k], size), size)
    layer.setflags(write=False)
    return layer


@functools.lru_cache(maxsize=None)
def host_canvas(size, n_agents):
    return render.Canvas(list(geoms()), size, n_agents, backend="host")


def scripted(geom):
    """Two cars along the track, 1.5 either side of the centre line, heading along
    the tangent: x, y, angle [T, 2].  Step 10 repeats step 9 (a zero-length
    segment), car 1 is far off-screen at step 20 (the clamp), car 0 has a NaN
    position at step 30."""
    wp, nrm = geom.waypoints[:200:2], geom.normals[:200:2]
    x = np.stack([wp[:, 0] + 1.5 * nrm[:, 0], wp[:, 0] - 1.5 * nrm[:, 0]], axis=1)
    y = np.stack([wp[:, 1] + 1.5 * nrm[:, 1], wp[:, 1] - 1.5 * nrm[:, 1]], axis=1)
    ang = np.arctan2(nrm[:, 0] * -1.0, nrm[:, 1])  # tangent = (n.y, -n.x)
    ang = np.stack([ang, ang], axis=1)
    x[10], y[10] = x[9], y[9]
    x[20, 1] += 1e5
    x[30, 0] = np.nan
    return x, y, ang


# ---------------------------------------------------------------- 1. the view
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("k", range(3))
def test_track_view_equals_restatement(k, size):
    v, r = render.track_view(geoms()[k], size), R.view(geoms()[k], size)
    for a, b in (("scale", "scale"), ("offset_x", "offset_x"), ("offset_y", "offset_y")):
        assert np.float64(v[a]).tobytes() == np.float64(r[b]).tobytes()
    assert v["screen_size"] == size
    assert np.array_equal(np.array(v["left_points"]), r["left"])
    assert np.array_equal(np.array(v["right_points"]), r["right"])
    assert np.array_equal(np.array(v["track_polygon"]), r["polygon"])
    assert tuple(v["start_left"]) == tuple(r["start_left"]) and tuple(v["start_right"]) == tuple(r["start_right"])
    assert all(isinstance(c, int) for p in v["left_points"][:3] + [v["start_left"]] for c in p)
    assert len(v["track_polygon"]) == 2 * len(geoms()[k].waypoints) + 1


# ---------------------------------------------------------------- 2. the static layer
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("k", range(3))
def test_static_layer_equals_restatement(k, size):
    ref = ref_layer(k, size)
    counts = np.bincount(ref.ravel(), minlength=4)
    print("class counts", k, size, counts)
    assert len(counts) == 4 and (counts >= 40).all(), counts  # no class is empty, so none can be wrong unseen
    assert np.array_equal(host_canvas(size, 2).layer[k], ref)


# ---------------------------------------------------------------- 3. trails and frames
@pytest.mark.parametrize("size", SIZES)
def test_scripted_paths_equal_restatement(size):
    g = geoms()
    env_ids = [2, 0, 1]  # image k shows env env_ids[k], whose track is geoms()[env_ids[k]]
    c = render.Canvas([g[e] for e in env_ids], size, 2, backend="host", env_ids=env_ids)
    refs = [R.RefCanvas(g[e], size, 2) for e in env_ids]
    paths = [scripted(g[e]) for e in range(3)]  # by env
    T = paths[0][0].shape[0]
    for t in range(T):
        x, y, a = (np.ascontiguousarray(np.stack([p[i][t] for p in paths]).reshape(-1)) for i in range(3))
        c.add_points(x, y)
        frames = c.compose(x, y, a)
        for k, e in enumerate(env_ids):
            refs[k].add_points(paths[e][0][t], paths[e][1][t])
            assert np.array_equal(c.trail[k], refs[k].trail), (t, k)
            assert np.array_equal(frames[k], refs[k].frame(paths[e][0][t], paths[e][1][t], paths[e][2][t])), (t, k)
    for k in range(3):
        tr = refs[k].trail
        both, only0 = int((tr == 0x30).sum()), int((tr == 0x10).sum())
        print("trail pixels", size, k, "both", both, "only trail 0", only0)
        assert both >= 30 and only0 >= 100  # so trail 1 over trail 0 is really exercised


# ---------------------------------------------------------------- 4. pixels one can check by hand
def test_hand_checkable_pixels():
    S = 128
    g = geoms()[0]
    c = render.Canvas([g], S, 2, backend="host")
    v = render.track_view(g, S)
    nan = np.full(2, np.nan)
    f = c.compose(nan, nan, nan)[0]  # no car is drawn
    assert tuple(f[0, 0]) == (50, 50, 50) and tuple(f[S - 1, S - 1]) == (50, 50, 50)
    (lx, ly), (rx_, ry) = v["start_left"], v["start_right"]
    assert tuple(f[(ly + ry) // 2, (lx + rx_) // 2]) == (0, 255, 0)
    trail_colours = {(255, 100, 100), (100, 100, 255)}
    assert not trail_colours & {tuple(p) for p in f.reshape(-1, 3)}
    # Axis-aligned cars: car 0 heading +x at (30, 30.4), car 1 heading +y at (40.8, 30).  The scale is 1.11
    # pixels per unit, so a car is 4.4 x 2.2 pixels and its truncated quad 2 or 3 pixels wide.  The outline
    # reaches 1 pixel from every edge, so only a quad 3 wide has a fill pixel, at its centre: these two
    # positions give quads of x 49..54, y 64..67 and x 62..65, y 64..68.
    x, y, a = np.array([30.0, 40.8]), np.array([30.4, 30.0]), np.array([0.0, np.pi / 2])
    f = c.compose(x, y, a)[0]
    quads = [R.car_quad(R.view(g, S), S, x[q], y[q], a[q]) for q in range(2)]
    for q, fill in enumerate(((255, 0, 0), (0, 0, 255))):
        lo, hi = quads[q].min(axis=0), quads[q].max(axis=0)
        assert (hi - lo).min() >= 3, quads[q]
        ci, cj = (lo + hi) // 2
        assert tuple(f[cj, ci]) == fill, (q, quads[q], f[cj, ci])
    # paths appear after two points, and begin() removes them
    c.add_points(x, y)
    c.add_points(x + 5.0, y)
    f = c.compose(nan, nan, nan)[0]
    assert trail_colours <= {tuple(p) for p in f.reshape(-1, 3)}
    c.begin()
    assert not c.trail.any() and not c.last.any()
    assert not trail_colours & {tuple(p) for p in c.compose(nan, nan, nan)[0].reshape(-1, 3)}


# ---------------------------------------------------------------- 5. the mosaic
@pytest.mark.parametrize("padding", (10, 3))
def test_mosaic_equals_pasted_frames(padding):
    S = 99
    g = geoms()
    c = render.Canvas([g[0], g[1], g[2], g[0]], S, 2, backend="host")
    x, y, a = (np.ascontiguousarray(np.stack([scripted(g[k % 3])[i][40 + k] for k in range(4)]).reshape(-1))
               for i in range(3))
    c.add_points(x, y)
    c.add_points(x + 3.0, y + 2.0)
    frames = c.compose(x, y, a)
    H = W = 2 * S + 3 * padding
    want = np.full((H, W, 3), 255, dtype=np.uint8)
    for k in range(4):
        top, left = padding + (k // 2) * (S + padding), padding + (k % 2) * (S + padding)
        want[top:top + S, left:left + S] = frames[k]
    got = c.mosaic(x, y, a, 2, 2, padding)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        c.mosaic(x, y, a, 1, 2, padding)


# ---------------------------------------------------------------- 6. the C ABI
RASTER_EXPORTS = ("rx_raster_static", "rx_raster_static_host", "rx_raster_trail", "rx_raster_trail_host",
                  "rx_raster_frame", "rx_raster_frame_host")


def test_abi_exports_and_version():
    L = _lib.load()
    for name in RASTER_EXPORTS:
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert L.rx_abi_version() == 25 and _lib.ABI_VERSION == 25
    assert (_lib.RX_PX_BACKGROUND, _lib.RX_PX_TRACK, _lib.RX_PX_BORDER, _lib.RX_PX_START) == (0, 1, 2, 3)
    assert (_lib.RX_PX_TRAIL0, _lib.RX_PX_TRAIL1) == (0x10, 0x20)


def _good_io(S=16, K=1, A=1):
    """A valid host rx_raster_io and the arrays behind it."""
    keep = dict(env_ids=np.zeros(K, np.int32), x=np.zeros(K * A), y=np.zeros(K * A), angle=np.zeros(K * A),
                view=np.ones((K, 3)), layer_of=np.zeros(K, np.int32), layer=np.zeros((1, S, S), np.uint8),
                trail=np.zeros((K, S, S), np.uint8), last=np.zeros((K, A, 3), np.int32),
                out=np.zeros((K, S, S, 3), np.uint8), out_off=np.arange(K, dtype=np.int64) * 3 * S * S)
    io = _lib.RxRasterIO(K=K, A=A, size=S, n_envs=K, n_layers=1, out_pitch=3 * S, out_size=keep["out"].size)
    for k, v in keep.items():
        setattr(io, k, _lib.ptr(v))
    return io, keep


@pytest.mark.parametrize("sfx", ("", "_host"))  # the device entry points check before any HIP call
def test_abi_refuses_bad_arguments_by_name(sfx):
    L = _lib.load()

    def refused(fn, io, word):
        assert getattr(L, fn + sfx)(ctypes.byref(io), None) == _lib.RX_EINVAL, (fn, word)
        msg = L.rx_last_error().decode()
        assert fn + sfx in msg and word in msg, msg

    for fn in ("rx_raster_trail", "rx_raster_frame"):
        for field, bad, word in (("size", 15, "size"), ("size", 2049, "size"), ("A", 0, "A="), ("A", 3, "A="),
                                 ("K", 0, "K="), ("K", -1, "K=")):
            io, keep = _good_io()
            setattr(io, field, bad)
            refused(fn, io, word)
    for field, bad in (("out_pitch", -4), ("out_pitch", 3 * 16 - 1)):
        io, keep = _good_io()
        setattr(io, field, bad)
        refused("rx_raster_frame", io, "out_pitch")
    for fn, fields in (("rx_raster_trail", ("env_ids", "x", "y", "view", "trail", "last")),
                       ("rx_raster_frame", ("env_ids", "x", "y", "angle", "view", "layer_of", "layer", "trail", "out",
                                            "out_off"))):
        for field in fields:
            io, keep = _good_io()
            setattr(io, field, None)
            refused(fn, io, "null pointer: " + field)
    static = getattr(L, "rx_raster_static" + sfx)
    off, edges, layer = np.zeros(2, np.int32), np.zeros((1, 6), np.int32), np.zeros((1, 16, 16), np.uint8)
    p = _lib.ptr
    for args, word in (((1, 15, 0, p(off), p(edges), p(layer)), "size"), ((1, 2049, 0, p(off), p(edges), p(layer)), "size"),
                       ((0, 16, 0, p(off), p(edges), p(layer)), "n="), ((1, 16, 0, None, p(edges), p(layer)), "edge_off"),
                       ((1, 16, 0, p(off), None, p(layer)), "edges"), ((1, 16, 0, p(off), p(edges), None), "layer")):
        assert static(*args, None) == _lib.RX_EINVAL
        assert word in L.rx_last_error().decode()


def test_abi_host_frame_skips_what_does_not_fit():
    L = _lib.load()
    io, keep = _good_io(S=16, K=2)
    io.out_size = 3 * 16 * 16  # room for one image: the second is left alone
    keep["out"][...] = 7
    assert L.rx_raster_frame_host(ctypes.byref(io), None) == _lib.RX_OK
    assert (keep["out"][0] != 7).any() and (keep["out"][1] == 7).all()


# ---------------------------------------------------------------- 7. the env classes
def test_env_render_modes():
    assert RacingEnv.metadata["render_modes"] == ["rgb_array"]
    assert MultiRacingEnv.metadata["render_modes"] == ["rgb_array"]
    with pytest.raises(ValueError):
        RacingEnv(render_mode="human")
    with pytest.raises(ValueError):
        MultiRacingEnv(render_mode="human")
    assert RacingEnv().render_mode is None and RacingEnv().render() is None
    assert RacingEnv(7, None, None, None, 8.0).render_mode is None  # the positional signature is unchanged
    assert MultiRacingEnv(render_mode="rgb_array").render_mode == "rgb_array"


def test_canvas_refuses_bad_shapes():
    g = geoms()[0]
    with pytest.raises(ValueError):
        render.Canvas([g], 15, 1, backend="host")
    with pytest.raises(ValueError):
        render.Canvas([g], 128, 3, backend="host")
    with pytest.raises(ValueError):
        render.Canvas([g], 128, 1, backend="cpu")
    c = render.Canvas([g], 16, 1, backend="host")
    with pytest.raises(ValueError):
        c.compose(np.zeros(1), np.zeros(2), np.zeros(1))
    with pytest.raises(TypeError):
        c.compose(np.zeros(1, np.float32), np.zeros(1), np.zeros(1))


# ---------------------------------------------------------------- rx.visualize without a device
def test_visualization_grid_over_npy_stacks(tmp_path):
    from rx.visualize import visualization_grid
    rng = np.random.default_rng(0)
    stacks = [rng.integers(0, 255, (n, 16, 16, 3), dtype=np.uint8) for n in (3, 1, 2, 3)]
    paths = []
    for k, st in enumerate(stacks):
        paths.append(str(tmp_path / f"s{k}.npy"))
        np.save(paths[-1], st)
    out = str(tmp_path / "grid.npy")
    visualization_grid(paths, ["a", "b", "c", "d"], output_path=out, padding=3)
    g = np.load(out)
    assert g.shape == (3, 2 * 16 + 9, 2 * 16 + 9, 3)
    for t in range(3):
        want = np.full(g.shape[1:], 255, dtype=np.uint8)
        for k, st in enumerate(stacks):
            top, left = 3 + (k // 2) * 19, 3 + (k % 2) * 19
            want[top:top + 16, left:left + 16] = st[min(t, len(st) - 1)]  # a finished stack keeps its last frame
        assert np.array_equal(g[t], want)
    with pytest.raises(ValueError):
        visualization_grid(paths[:3], ["a", "b", "c"], output_path=out)


def test_video_suffix_without_cv2_is_a_clear_import_error(tmp_path):
    try:
        import cv2  # noqa: F401
        return  # with OpenCV installed the writer opens instead
    except ImportError:
        pass
    from rx.visualize import visualize_single_agent
    with pytest.raises(ImportError, match="cv2"):
        visualize_single_agent(None, None, "cpu", str(tmp_path / "run.mp4"))
