"""An independent NumPy restatement of the renderer's raster rules (DESIGN.md §4,
"Rendering"), for tests/test_render_cpu.py.  It never calls librx and shares
no code with rx.render: whole-image integer arrays in doubled coordinates.

  * vertex (X, Y) -> (2X, 2Y); pixel (column i, row j) is sampled at (2i+1, 2j+1);
  * even-odd fill: edge a->b counts when (a.y < s.y) != (b.y < s.y) and it meets
    the row strictly right of s;
  * a line of width w is the capsule |s - segment| <= w (doubled units);
  * moving screen coordinates are clamped to [-4096, 8191] before truncation;
    a non-finite pose is invisible.
"""
import functools

import numpy as np

BACKGROUND, TRACK, BORDER, START = 0, 1, 2, 3
TRAIL_BITS = (0x10, 0x20)
COLOURS = {BACKGROUND: (50, 50, 50), TRACK: (180, 180, 180), BORDER: (0, 0, 0), START: (0, 255, 0)}
TRAIL_COLOURS = ((255, 100, 100), (100, 100, 255))
CAR_FILL = ((255, 0, 0), (0, 0, 255))
CAR_LINE = ((150, 0, 0), (0, 0, 150))


@functools.lru_cache(maxsize=None)
def sample_geoms():
    """The three tracks of the render tests: the default track at width 6 and
    gen_tracks(2, seed=3) at widths 5 and 9.  gen_tracks draws a track's
    parameters from the global RNG before it seeds it, so the RNG is pinned
    for the call and put back."""
    from rx.track import TrackGeometry, gen_tracks
    state = np.random.get_state()
    np.random.seed(0)
    cps = gen_tracks(2, seed=3)
    np.random.set_state(state)
    return (TrackGeometry(None, 6.0), TrackGeometry(cps[0], 5.0), TrackGeometry(cps[1], 9.0))


def view(geom, size):
    """setup_track_visualization, vectorised: scale, offsets, integer points."""
    pts = np.vstack([geom.left_boundary, geom.right_boundary])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    scale = min(size / ((hi[0] - lo[0]) + 2 * 10), size / ((hi[1] - lo[1]) + 2 * 10))
    ox, oy = -lo[0] + 10, -lo[1] + 10

    def conv(p):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
        return np.column_stack([np.trunc((p[:, 0] + ox) * scale), np.trunc(size - (p[:, 1] + oy) * scale)]).astype(
            np.int64)
    left, right = conv(geom.left_boundary), conv(geom.right_boundary)
    w0, n0, tw = geom.waypoints[0], geom.normals[0], geom.track_width
    return dict(scale=scale, offset_x=ox, offset_y=oy, left=left, right=right,
                polygon=np.concatenate([left, right[::-1], left[:1]]),
                start_left=conv([w0[0] + n0[0] * tw, w0[1] + n0[1] * tw])[0],
                start_right=conv([w0[0] - n0[0] * tw, w0[1] - n0[1] * tw])[0])


def _samples(size):
    s = 2 * np.arange(size, dtype=np.int64) + 1
    return s[None, :], s[:, None]  # x along columns, y along rows


def fill(size, poly):
    """Even-odd interior of the closed polygon ``poly`` [n, 2] -> bool [S, S]."""
    sx, sy = _samples(size)
    inside = np.zeros((size, size), dtype=bool)
    a = 2 * np.asarray(poly, dtype=np.int64)
    b = np.roll(a, -1, axis=0)
    for (ax, ay), (bx, by) in zip(a, b):
        if ay == by:
            continue
        rows = ((ay < sy) != (by < sy))[:, 0]
        if not rows.any():
            continue
        y = sy[rows]
        # the meeting point lies right of s  <=>  (s.y - a.y)(b.x - a.x) - (s.x - a.x)(b.y - a.y) has the sign of b.y - a.y
        cr = (y - ay) * (bx - ax) - (sx - ax) * (by - ay)
        inside[rows] ^= (cr > 0) if by > ay else (cr < 0)
    return inside


def capsule(size, a, b, w, out=None):
    """Pixels whose centre is within w/2 of segment a-b -> bool [S, S] (OR-ed into ``out``)."""
    out = np.zeros((size, size), dtype=bool) if out is None else out
    ax, ay = (2 * int(v) for v in a)
    bx, by = (2 * int(v) for v in b)
    # only pixels of the segment's box grown by the width can be inside
    i0, i1 = max((min(ax, bx) - w) // 2 - 1, 0), min((max(ax, bx) + w) // 2 + 1, size - 1)
    j0, j1 = max((min(ay, by) - w) // 2 - 1, 0), min((max(ay, by) + w) // 2 + 1, size - 1)
    if i0 > i1 or j0 > j1:
        return out
    sx = 2 * np.arange(i0, i1 + 1, dtype=np.int64)[None, :] + 1
    sy = 2 * np.arange(j0, j1 + 1, dtype=np.int64)[:, None] + 1
    dx, dy = bx - ax, by - ay
    px, py = sx - ax, sy - ay
    L = dx * dx + dy * dy
    u = px * dx + py * dy
    near_a = px * px + py * py <= w * w
    near_b = (sx - bx) ** 2 + (sy - by) ** 2 <= w * w
    cr = px * dy - py * dx
    band = cr * cr <= w * w * L
    inside = np.where((L == 0) | (u <= 0), near_a, np.where(u >= L, near_b, band))
    out[j0:j1 + 1, i0:i1 + 1] |= inside
    return out


def polyline(size, pts, w, closed, out=None):
    out = np.zeros((size, size), dtype=bool) if out is None else out
    pts = np.asarray(pts)
    n = len(pts)
    for k in range(n if closed else n - 1):
        capsule(size, pts[k], pts[(k + 1) % n], w, out)
    return out


def static_layer(v, size):
    """Class byte per pixel: background, then track, borders, start line."""
    layer = np.zeros((size, size), dtype=np.uint8)
    layer[fill(size, v["polygon"])] = TRACK
    layer[polyline(size, v["left"], 4, True) | polyline(size, v["right"], 4, True)] = BORDER
    layer[capsule(size, v["start_left"], v["start_right"], 5)] = START
    return layer


def screen(v, size, x, y):
    """convert_coords with the clamp; None for a non-finite position."""
    if not (np.isfinite(x) and np.isfinite(y)):
        return None
    sx, sy = (x + v["offset_x"]) * v["scale"], size - (y + v["offset_y"]) * v["scale"]
    if np.isnan(sx) or np.isnan(sy):
        return None
    return int(np.clip(sx, -4096.0, 8191.0)), int(np.clip(sy, -4096.0, 8191.0))


def car_quad(v, size, x, y, angle):
    """Car.get_corners through convert_coords -> int [4, 2], or None (invisible)."""
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(angle)):
        return None
    c, s = np.cos(angle), np.sin(angle)
    quad = []
    for lx, ly in ((2.0, 1.0), (2.0, -1.0), (-2.0, -1.0), (-2.0, 1.0)):
        p = screen(v, size, (c * lx - s * ly) + x, (s * lx + c * ly) + y)
        if p is None:
            return None
        quad.append(p)
    return np.array(quad, dtype=np.int64)


class RefCanvas:
    """One image: static layer, trail layer and the composed frame."""

    def __init__(self, geom, size, n_agents):
        self.size, self.A = size, n_agents
        self.v = view(geom, size)
        self.layer = static_layer(self.v, size)
        self.begin()

    def begin(self):
        self.trail = np.zeros((self.size, self.size), dtype=np.uint8)
        self.last = [None] * self.A

    def add_points(self, x, y):
        for q in range(self.A):
            p = screen(self.v, self.size, x[q], y[q])
            if p is None:
                continue
            if self.last[q] is not None:
                self.trail[capsule(self.size, self.last[q], p, 3)] |= TRAIL_BITS[q]
            self.last[q] = p

    def frame(self, x, y, angle):
        S = self.size
        img = np.empty((S, S, 3), dtype=np.uint8)
        for cls, col in COLOURS.items():
            img[self.layer == cls] = col
        for q in range(2):
            img[(self.trail & TRAIL_BITS[q]) != 0] = TRAIL_COLOURS[q]
        for q in range(self.A):
            quad = car_quad(self.v, S, x[q], y[q], angle[q])
            if quad is None:
                continue
            img[fill(S, quad)] = CAR_FILL[q]
            img[polyline(S, quad, 2, True)] = CAR_LINE[q]
        return img
