"""rgb_array rendering: the drawing of utils/visualization.py on the device.

``track_view`` is ``setup_track_visualization`` (visualization.py:12-59)
operation for operation in NumPy.  ``Canvas`` owns the layers of K images and
drives librx's three raster calls (include/rx.h, csrc/rx_raster.h):

* the static layer of every distinct track (background / track / border /
  start line, one byte per pixel), rasterised once;
* one trail layer per image, extended by one capsule per car and step;
* ``compose`` / ``mosaic``: the RGB frames, written where they are wanted.

``backend="device"`` runs the gfx950 kernels on torch's current stream with no
host wait; ``backend="host"`` runs the bit-identical host twins on NumPy
arrays and needs no GPU.  ``Renderer`` feeds a ``Canvas`` from a vector env's
device state.  The pixels follow this project's own exact rules,
not pygame's, and there is no HUD text: the numbers are in ``info``.
"""
import numpy as np

from . import _lib

MAX_IMAGES = 1024  # Renderer: images composed at once (1,024 frames of 800 x 800 are 2 GB)
PADDING = 10       # setup_track_visualization's margin in track units


def convert_coords(x, y, ox, oy, scale, screen_size):
    """visualization.py:6-9"""
    return int((x + ox) * scale), int(screen_size - (y + oy) * scale)


def track_view(geom, size=800):
    """``setup_track_visualization(track, size)``: the same dict from a
    ``TrackGeometry`` (visualization.py:12-59)."""
    all_points = np.vstack([geom.left_boundary, geom.right_boundary])
    min_x, min_y = all_points.min(axis=0)
    max_x, max_y = all_points.max(axis=0)
    padding = PADDING
    track_width = max_x - min_x
    track_height = max_y - min_y
    scale = min(size / (track_width + 2 * padding), size / (track_height + 2 * padding))
    offset_x = -min_x + padding
    offset_y = -min_y + padding
    left_points = [convert_coords(p[0], p[1], offset_x, offset_y, scale, size) for p in geom.left_boundary]
    right_points = [convert_coords(p[0], p[1], offset_x, offset_y, scale, size) for p in geom.right_boundary]
    track_polygon = left_points + right_points[::-1] + [left_points[0]]
    wp, nrm, w = geom.waypoints, geom.normals, geom.track_width
    start_left = convert_coords(wp[0][0] + nrm[0][0] * w, wp[0][1] + nrm[0][1] * w, offset_x, offset_y, scale, size)
    start_right = convert_coords(wp[0][0] - nrm[0][0] * w, wp[0][1] - nrm[0][1] * w, offset_x, offset_y, scale, size)
    return {"scale": scale, "offset_x": offset_x, "offset_y": offset_y, "screen_size": size,
            "left_points": left_points, "right_points": right_points, "track_polygon": track_polygon,
            "start_left": start_left, "start_right": start_right}


def view_edges(view):
    """The edge records of a view's static layer, int32 [E][6] = ax, ay, bx, by,
    class, width (include/rx.h): the polygon (closed; visualization.py:104), both
    boundary loops at width 4 (:105-106) and the start line at width 5 (:107)."""
    def seg(pts, closed, cls, width):
        a = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
        b = np.roll(a, -1, axis=0)
        if not closed:
            a, b = a[:-1], b[:-1]
        return np.column_stack([a, b, np.full(len(a), cls), np.full(len(a), width)])
    e = np.concatenate([seg(view["track_polygon"], True, _lib.RX_PX_TRACK, 0),
                        seg(view["left_points"], True, _lib.RX_PX_BORDER, 4),
                        seg(view["right_points"], True, _lib.RX_PX_BORDER, 4),
                        seg([view["start_left"], view["start_right"]], False, _lib.RX_PX_START, 5)])
    return np.ascontiguousarray(e, dtype=np.int32)


def mosaic_shape(size, rows, cols, padding=10):
    """Height and width of visualization_grid's frame (visualization.py:421-422, for any rows x cols)."""
    return size * rows + padding * (rows + 1), size * cols + padding * (cols + 1)


class Canvas:
    """The layers of K images of ``size`` x ``size`` pixels.

    ``geoms[k]`` is the ``TrackGeometry`` image k shows (equal objects share one
    static layer).  Poses are flat float64 arrays with element ``e * n_agents +
    q`` for car q of env e -- the layout of ``RacingVectorEnv.state`` -- and image
    k shows env ``env_ids[k]`` (default: env k).  Arrays are torch tensors on
    ``device`` for the device backend and NumPy arrays for the host backend."""

    def __init__(self, geoms, size, n_agents, backend="device", device=None, env_ids=None):
        if backend not in ("device", "host"):
            raise ValueError(f"backend must be 'device' or 'host', got {backend!r}")
        self.K = K = len(geoms)
        self.size = S = int(size)
        self.A = int(n_agents)
        if K <= 0:
            raise ValueError("need at least one image")
        if not _lib.RX_RASTER_SIZE_MIN <= S <= _lib.RX_RASTER_SIZE_MAX:
            raise ValueError(f"size must be in {_lib.RX_RASTER_SIZE_MIN}..{_lib.RX_RASTER_SIZE_MAX}, got {S}")
        if self.A not in (1, 2):
            raise ValueError(f"n_agents must be 1 or 2, got {n_agents}")
        self.backend = backend
        self.L = _lib.load()
        distinct, layer_of = {}, np.empty(K, dtype=np.int32)
        self.geoms = []
        for k, g in enumerate(geoms):
            layer_of[k] = distinct.setdefault(id(g), len(distinct))
            if layer_of[k] == len(self.geoms):
                self.geoms.append(g)
        self.views = [track_view(g, S) for g in self.geoms]
        view = np.array([[self.views[s][key] for key in ("scale", "offset_x", "offset_y")] for s in layer_of],
                        dtype=np.float64)
        ids = np.arange(K, dtype=np.int32) if env_ids is None else np.asarray(env_ids, dtype=np.int32).reshape(K)
        if ids.min() < 0:
            raise ValueError("env_ids must not be negative")
        self._min_envs = int(ids.max()) + 1
        if backend == "device":
            import torch
            self.torch = torch
            dev = torch.device("cuda" if device is None else device)
            if dev.type != "cuda":
                raise ValueError(f"the device backend runs on a HIP device, got {dev}")
            # with its index, so that it compares equal to the device of the tensors handed in
            self.device = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        else:
            self.device = None
        self.env_ids, self.layer_of, self.view = self._put(ids), self._put(layer_of), self._put(view)
        self.layer = None
        self.trail = self._empty((K, S, S))
        self.last = self._empty((K, self.A, 3), "int32")
        self._offs = {}
        self.begin()

    # ------------------------------------------------------------ arrays of either backend
    def _put(self, a):
        return self.torch.from_numpy(a).to(self.device) if self.backend == "device" else a

    def _empty(self, shape, dtype="uint8"):
        if self.backend == "device":
            return self.torch.empty(shape, dtype=getattr(self.torch, dtype), device=self.device)
        return np.empty(shape, dtype=dtype)

    def _pose(self, a, name):
        if self.backend == "device":
            ok = isinstance(a, self.torch.Tensor) and a.dtype == self.torch.float64 and a.device == self.device
        else:
            ok = isinstance(a, np.ndarray) and a.dtype == np.float64
        if not ok:
            raise TypeError(f"{name} must be a float64 " + (f"tensor on {self.device}" if self.device else "ndarray"))
        a = a.reshape(-1)
        n = a.shape[0]
        if n % self.A or n // self.A < self._min_envs:
            raise ValueError(f"{name} has {n} elements: need n_agents * n_envs with n_envs >= {self._min_envs}")
        return np.ascontiguousarray(a) if self.backend == "host" else a.contiguous()

    def _call(self, name, *args):
        if self.backend == "device":
            with self.torch.cuda.device(self.device):
                fn = getattr(self.L, name)
                _lib.check(fn(*args, _lib.stream_ptr(self.torch.cuda.current_stream(self.device))), name)
        else:
            _lib.check(getattr(self.L, name + "_host")(*args, None), name + "_host")

    def _io(self, x, y, angle=None, out=None, out_off=None, pitch=0):
        x, y = self._pose(x, "x"), self._pose(y, "y")
        if y.shape != x.shape:
            raise ValueError("x and y differ in length")
        if angle is not None:
            angle = self._pose(angle, "angle")
            if angle.shape != x.shape:
                raise ValueError("x and angle differ in length")
        io = _lib.RxRasterIO(K=self.K, A=self.A, size=self.size, n_envs=x.shape[0] // self.A,
                             n_layers=len(self.geoms), out_pitch=pitch,
                             out_size=0 if out is None else (out.numel() if self.backend == "device" else out.size))
        keep = dict(env_ids=self.env_ids, x=x, y=y, angle=angle, view=self.view, layer_of=self.layer_of,
                    layer=self.layer, trail=self.trail, last=self.last, out=out, out_off=out_off)
        for k, v in keep.items():
            setattr(io, k, _lib.ptr(v))
        return io, keep  # `keep` holds the arrays alive over the call

    # ------------------------------------------------------------ episode
    def begin(self):
        """Start an episode: build the static layers on first use, clear the trails."""
        if self.layer is None:
            edges = [view_edges(v) for v in self.views]
            off = np.concatenate([[0], np.cumsum([len(e) for e in edges])]).astype(np.int32)
            e = np.ascontiguousarray(np.concatenate(edges))
            layer = self._empty((len(edges), self.size, self.size))
            off_d, e_d = self._put(off), self._put(e)
            self._call("rx_raster_static", len(edges), self.size, len(e), _lib.ptr(off_d), _lib.ptr(e_d),
                       _lib.ptr(layer))
            self.layer = layer
        if self.backend == "device":
            self.trail.zero_()
            self.last.zero_()
        else:
            self.trail[...] = 0
            self.last[...] = 0

    def add_points(self, x, y):
        """Append every car's position to its path (visualization.py:109-113, :226-243)."""
        io, keep = self._io(x, y)
        self._call("rx_raster_trail", io)

    # ------------------------------------------------------------ frames
    def _offsets(self, key, off):
        if key not in self._offs:
            self._offs[key] = self._put(np.ascontiguousarray(off, dtype=np.int64))
        return self._offs[key]

    def compose(self, x, y, angle, out=None):
        """The K frames, uint8 [K, size, size, 3]."""
        K, S = self.K, self.size
        if out is None:
            out = self._empty((K, S, S, 3))
        elif tuple(out.shape) != (K, S, S, 3) or str(out.dtype).split(".")[-1] != "uint8":
            raise ValueError(f"out must be uint8 [{K}, {S}, {S}, 3]")
        elif not (out.is_contiguous() if self.backend == "device" else out.flags.c_contiguous):
            raise ValueError("out must be contiguous")
        off = self._offsets("frames", np.arange(K, dtype=np.int64) * (3 * S * S))
        io, keep = self._io(x, y, angle, out, off, 3 * S)
        self._call("rx_raster_frame", io)
        return out

    def mosaic(self, x, y, angle, rows, cols, padding=10):
        """The K frames laid out as visualization_grid does (visualization.py:456-464):
        a white uint8 [H, W, 3] with frame k at row k // cols, column k % cols,
        ``padding`` pixels around and between; the frames are composed in place."""
        K, S = self.K, self.size
        if rows <= 0 or cols <= 0 or K > rows * cols:
            raise ValueError(f"{K} images do not fit a {rows} x {cols} grid")
        if padding < 0:
            raise ValueError("padding must not be negative")
        H, W = mosaic_shape(S, rows, cols, padding)
        out = self._empty((H, W, 3))
        if self.backend == "device":
            out.fill_(255)
        else:
            out[...] = 255
        k = np.arange(K, dtype=np.int64)
        top, left = padding + (k // cols) * (S + padding), padding + (k % cols) * (S + padding)
        off = self._offsets(("mosaic", rows, cols, padding), (top * W + left) * 3)
        io, keep = self._io(x, y, angle, out, off, 3 * W)
        self._call("rx_raster_frame", io)
        return out


class Renderer:
    """A device ``Canvas`` fed from a vector env's state.

        r = Renderer(venv, env_ids=[0, 3]); venv.reset_device(); r.begin()
        venv.step_device(actions); r.step(); frames = r.frame()   # uint8 [2, 800, 800, 3] on the device

    Only envs with ``autoreset="disabled"`` are accepted -- where the reference
    renders: evaluation pools and single envs; an autoresetting env would jump
    to the start mid-path."""

    def __init__(self, venv, env_ids=None, size=800):
        mode = getattr(venv, "autoreset", None)
        if mode != "disabled":
            raise ValueError(f"Renderer needs a vector env with autoreset='disabled', got {mode!r}")
        N = venv.num_envs
        ids = np.arange(N) if env_ids is None else np.asarray(env_ids, dtype=np.int64).reshape(-1)
        if len(ids) == 0 or ids.min() < 0 or ids.max() >= N:
            raise ValueError(f"env_ids must name envs 0..{N - 1}")
        if len(ids) > MAX_IMAGES:
            raise ValueError(f"{len(ids)} images at once: a Renderer composes at most {MAX_IMAGES} "
                             f"(choose env_ids)")
        self.venv = venv
        self.env_ids = ids
        geoms = [venv.tracks.geoms[venv.track_of_env[e]] for e in ids]
        self.canvas = Canvas(geoms, size, venv.n_agents, backend="device", device=venv.device, env_ids=ids)

    def begin(self):
        """After a reset: new, empty paths."""
        self.canvas.begin()

    def step(self):
        """After each step: append the cars' positions to their paths."""
        st = self.venv.state
        self.canvas.add_points(st["x"], st["y"])

    def frame(self, out=None):
        st = self.venv.state
        return self.canvas.compose(st["x"], st["y"], st["angle"], out)

    def mosaic(self, rows, cols, padding=10):
        st = self.venv.state
        return self.canvas.mosaic(st["x"], st["y"], st["angle"], rows, cols, padding)
