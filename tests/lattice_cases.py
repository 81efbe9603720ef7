"""Lattice tracks: inputs on which the exactness rules of the kernels actually decide
(DESIGN.md §4 "Lattice tracks").

The spline tracks and random states of the other cases are generic doubles: no two
waypoints are ever equidistant from a car, no ray direction has a sine of exactly 0, no
origin lies exactly on a wall, a vertex or the plane of a chunk box.  On a track whose
waypoints are integers all of these happen exactly:

* ``rect60x30``   a 60 x 30 rectangle, waypoints every 2, width 4 (W = 90: not a multiple of
                  RX_WP_CHUNK = 8); every normal is (0, +-1) or (+-1, 0), every boundary vertex an
                  integer;
* ``rect100x12``  a 100 x 12 rectangle, waypoints every 1, width 7 (W = 224: seven waypoint
                  super-chunks): the width exceeds half the distance between the straights, so
                  the points of the centre line are INSIDE the track and tie between waypoints
                  of opposite straights, half a lap apart;
* ``diamond40``   |x| + |y| = 40, width 5 (W = 160): integer waypoints, irrational normals.

Slots of the table (and of the env's TrackSet): 0 and 1 are the golden spline tracks 0 and
16 (the default track), 2 .. 4 the lattice tracks above.

The KAT inputs here are pure NumPy (tests/golden/gen_golden.py's ``lattice`` target feeds
them to the reference; tests/golden/lattice.npz holds what it answered):

* ``ray_kats``     (track, ox, oy, dir, progress): origins on wall lines, boundary vertices and
                   the planes of the chunk boxes for G = 6, 8, 16 (``chunk_boxes``), and 1e-9 to
                   either side of those; directions exactly 0.0, k pi / 2 (k = -2 .. 6), their
                   1-ulp neighbours, offsets of 1e-12 .. 1e-7, exact wall directions, arctan2
                   aimed at vertices.
* ``single_kats``  state-injected single-agent steps: cars parked on tie points at 0, pi/2, pi,
                   3 pi / 2 and generic angles, moving cars that cross a tie point, `progress`
                   (the kernels' window centre) near the answer or half a lap away, per-env
                   speed weights.
* ``multi_kats``   state-injected two-car steps: axis-aligned parked cars at integer and
                   half-integer offsets (a ray that leaves exactly 0.5 from the other centre, runs
                   along an edge of the other car, meets one of its corners; equal placement
                   scores).  A two-car throttle is (a + 1) / 2, so "parked" is action (0, -1).

``parked_single`` / ``parked_multi`` are 24-step traces of parked cars on non-crashed tie
points stepped by the device-libm oracle (tests/lap_cases.py's runners): nothing may move,
so every step repeats step 0.  24 steps reach the deep launch schedule of rx_steps.

``census_*`` count, per track, how often each edge occurs; tests/test_lattice_cpu.py holds
them to floors.
"""
import numpy as np

from oracle.orc import F_CP25, TrackTable, multi_state, sensor_angles, single_state
from tests import lap_cases as lc

REL1 = sensor_angles(11, np.pi / 3)
REL2 = sensor_angles(11, np.pi / 2)
GOLDEN_SLOTS = (0, 16)
L0 = len(GOLDEN_SLOTS)  # slot of the first lattice track
CULL_G = (6, 8, 16)
PARKED_STEPS = 24
HALF_PI = np.pi / 2
_LOCAL = np.array([[2.0, 1.0], [2.0, -1.0], [-2.0, -1.0], [-2.0, 1.0]])  # car.py:26-43


# ------------------------------------------------------------------------------ tracks
def rect(w, h, step):
    """Integer waypoints round the rectangle [0, w] x [0, h], counter-clockwise from (0, 0)."""
    xs, ys = np.arange(0, w, step), np.arange(0, h, step)
    pts = ([(x, 0) for x in xs] + [(w, y) for y in ys] + [(w - x, h) for x in xs] + [(0, h - y) for y in ys])
    return np.array(pts, dtype=np.int64)


def diamond(r):
    """Integer waypoints round |x| + |y| = r, counter-clockwise from (r, 0)."""
    k = np.arange(r)
    return np.concatenate([np.stack([r - k, k], 1), np.stack([-k, r - k], 1), np.stack([k - r, -k], 1),
                           np.stack([k, k - r], 1)]).astype(np.int64)


SPECS = (("rect60x30", rect(60, 30, 2), 4.0), ("rect100x12", rect(100, 12, 1), 7.0), ("diamond40", diamond(40), 5.0))
NAMES = tuple(s[0] for s in SPECS)
_CACHE = {}


def geometry(wp_int, width):
    from rx.track import TrackGeometry
    return TrackGeometry.from_waypoints(wp_int, width, wp_int.astype(np.float64))


def _record(name, wp_int, width):
    g = geometry(wp_int, width)
    st = g.get_start_pos()
    return dict(cp=wp_int, wp=g.waypoints, nrm=g.normals, starts=g.segment_cache["starts"], v2=g.segment_cache["v2"],
                start=np.array([float(st[0]), float(st[1]), float(st[2])]), width=float(width),
                maxd=float(g.max_track_distance), label=name)


def tracks():
    """The lattice tracks as golden-style records (tests/golden_util.py Golden.tracks)."""
    if "tracks" not in _CACHE:
        _CACHE["tracks"] = [_record(*s) for s in SPECS]
    return _CACHE["tracks"]


def slot_records(golden):
    return [golden.tracks[k] for k in GOLDEN_SLOTS] + tracks()


def table(golden):
    if "table" not in _CACHE:
        _CACHE["table"] = TrackTable(slot_records(golden))
    return _CACHE["table"]


def _cp(rec):
    from rx.track import DEFAULT_CONTROL_POINTS
    return DEFAULT_CONTROL_POINTS if rec["label"] == "default" else rec["cp"]


def track_set(golden):
    """A TrackSet whose slots are ``slot_records``: the two spline slots from their control points,
    the lattice slots from their waypoints (keyed by the integer waypoint array)."""
    from rx.track import TrackSet
    ts = TrackSet()
    for rec in slot_records(golden):
        if rec["label"] in NAMES:
            ts._index[TrackSet._key(rec["cp"], rec["width"])] = len(ts.geoms)
            ts.geoms.append(geometry(rec["cp"], rec["width"]))
            ts._packed = None
        else:
            ts.slot(_cp(rec), rec["width"])
    return ts


def env_args(golden, slots):
    """(control_points, widths, track_set) for RacingVectorEnv with env e on slot slots[e]."""
    recs = slot_records(golden)
    cps = [_cp(r) for r in recs]
    return [cps[k] for k in slots], [recs[k]["width"] for k in slots], track_set(golden)


def chunk_boxes(rec, G):
    """[2 ceil(W / G), 4] (x0, y0, x1, y1): the boxes of the end points of G consecutive
    boundary segments, left side then right side (include/rx.h's chunk_box)."""
    W = len(rec["wp"])
    s, e = rec["starts"], rec["starts"] + rec["v2"]
    out = []
    for side in range(2):
        for c in range(-(-W // G)):
            r = slice(side * W + c * G, side * W + min(W, (c + 1) * G))
            p = np.concatenate([s[r], e[r]])
            out.append((p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()))
    return np.array(out)


# ------------------------------------------------------------------------------ ties
def tied(wp, x, y):
    """[P, W] bool: the waypoints at exactly the smallest squared distance from each point
    (Track.closest_waypoint_idx's expression)."""
    d = (wp[None, :, 0] - np.asarray(x)[:, None]) ** 2 + (wp[None, :, 1] - np.asarray(y)[:, None]) ** 2
    return d == d.min(1, keepdims=True)


def tie_kinds(wp, x, y):
    """Per point: (number of tied waypoints, is the tied set NOT one run of consecutive indices)."""
    t = tied(wp, x, y)
    n = t.sum(1)
    runs = (t & ~np.roll(t, 1, axis=1)).sum(1)  # circular runs of tied indices
    return n, (n >= 2) & (runs >= 2)


def crashed_at(rec, x, y, ang):
    """Track.check_collision for cars at (x, y, ang), NumPy."""
    wp, nrm = rec["wp"], rec["nrm"]
    c, s = np.cos(ang), np.sin(ang)
    cx = c[:, None] * _LOCAL[:, 0] - s[:, None] * _LOCAL[:, 1] + x[:, None]
    cy = s[:, None] * _LOCAL[:, 0] + c[:, None] * _LOCAL[:, 1] + y[:, None]
    out = np.zeros(len(x), bool)
    for q in range(4):
        i = ((wp[None, :, 0] - cx[:, q, None]) ** 2 + (wp[None, :, 1] - cy[:, q, None]) ** 2).argmin(1)
        out |= np.abs((cx[:, q] - wp[i, 0]) * nrm[i, 0] + (cy[:, q] - wp[i, 1]) * nrm[i, 1]) > rec["width"]
    return out


def tie_points(rec):
    """Half-integer grid points within width + 2 of the track with an exact closest-waypoint
    tie: dict x, y, n (tied waypoints), apart (non-neighbouring), free (a car at angle 0 stands
    there without crashing)."""
    wp = rec["wp"]
    m = rec["width"] + 2.0
    gx = np.arange(wp[:, 0].min() - m, wp[:, 0].max() + m + 0.25, 0.5)
    gy = np.arange(wp[:, 1].min() - m, wp[:, 1].max() + m + 0.25, 0.5)
    x, y = (a.reshape(-1) for a in np.meshgrid(gx, gy, indexing="ij"))
    d = ((wp[None, :, 0] - x[:, None]) ** 2 + (wp[None, :, 1] - y[:, None]) ** 2).min(1)
    near = d <= m * m
    x, y = x[near], y[near]
    n, apart = tie_kinds(wp, x, y)
    keep = n >= 2
    x, y, n, apart = x[keep], y[keep], n[keep], apart[keep]
    return dict(x=x, y=y, n=n, apart=apart, free=~crashed_at(rec, x, y, np.zeros(len(x))))


def _pick(rng, pts, count, free_only=False):
    """Up to `count` distinct tie points: a third non-neighbouring, a third three or more wide, the
    rest any."""
    ok = pts["free"] if free_only else np.ones(len(pts["x"]), bool)
    third = count // 3
    idx = np.concatenate([rng.permutation(np.flatnonzero(ok & pts["apart"]))[:third],
                          rng.permutation(np.flatnonzero(ok & (pts["n"] >= 3)))[:third],
                          rng.permutation(np.flatnonzero(ok))])
    _, first = np.unique(idx, return_index=True)
    return idx[np.sort(first)][:count]


def closest(wp, x, y):
    return ((wp[None, :, 0] - np.asarray(x)[:, None]) ** 2 + (wp[None, :, 1] - np.asarray(y)[:, None]) ** 2).argmin(1)


# ------------------------------------------------------------------------------ ray KATs
def _directions():
    base = np.array([k * HALF_PI for k in range(-2, 7)])
    ulps = np.concatenate([np.nextafter(base, -np.inf), np.nextafter(base, np.inf)])
    offs = np.concatenate([base + s * e for e in (1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7) for s in (-1.0, 1.0)])
    return base, ulps, offs


def _ray_origins(rec, rng):
    """Origins on boundary vertices, on wall lines, on the chunk-box planes, inside and outside the
    track -- and 1e-9 to either side of a third of them."""
    wp, nrm, w = rec["wp"], rec["nrm"], rec["width"]
    s, v2 = rec["starts"], rec["v2"]
    pick = lambda a, k: a[rng.permutation(len(a))[:k]]  # noqa: E731
    parts = [pick(s, 24), pick(s + v2 * 0.5, 12), pick(s + v2 * 0.25, 6)]
    for G in CULL_G:
        b = pick(chunk_boxes(rec, G), 5)
        cx, cy = 0.5 * (b[:, 0] + b[:, 2]), 0.5 * (b[:, 1] + b[:, 3])
        parts += [np.stack([b[:, 0], cy], 1), np.stack([b[:, 2], cy], 1), np.stack([cx, b[:, 1]], 1),
                  np.stack([cx, b[:, 3]], 1), b[:2, :2], b[2:, 2:]]
    i = rng.permutation(len(wp))
    parts += [wp[i[:8]], wp[i[8:14]] + nrm[i[8:14]] * (w / 2), wp[i[14:20]] - nrm[i[14:20]] * (w / 2),
              wp[i[20:32]] - nrm[i[20:32]] * (w + 3.0), wp[i[32:36]] + nrm[i[32:36]] * (w + 3.0)]
    o = np.concatenate(parts)
    j = rng.permutation(len(o))[:len(o) // 4]
    eps = np.where(rng.random((len(j), 2)) < 0.5, -1e-9, 1e-9) * (rng.random((len(j), 2)) < 0.7)
    return np.concatenate([o, o[j] + eps])


def ray_kats(seed=11):
    """dict track, ox, oy, dir, progress (the window centre: the closest waypoint, or half a lap
    away on odd rows)."""
    if "rays" in _CACHE:
        return _CACHE["rays"]
    rng = np.random.default_rng(seed)
    base, ulps, offs = _directions()
    rows = []
    for j, rec in enumerate(tracks()):
        s, v2 = rec["starts"], rec["v2"]
        walls = np.unique(np.arctan2(v2[:, 1], v2[:, 0]))
        for ox, oy in _ray_origins(rec, rng):
            aim = s[rng.integers(len(s), size=2)]
            aimed = np.arctan2(aim[:, 1] - oy, aim[:, 0] - ox)
            ds = [0.0, rng.choice(base), rng.choice(ulps), rng.choice(offs), rng.choice(walls), aimed[0], aimed[1]]
            rows += [(L0 + j, ox, oy, float(d)) for d in ds]
    a = np.array(rows)
    k = a[:, 0].astype(np.int32)
    prog = np.zeros(len(a))
    for j, rec in enumerate(tracks()):
        m = k == L0 + j
        W = len(rec["wp"])
        c = closest(rec["wp"], a[m, 1], a[m, 2])
        prog[m] = np.where(np.arange(m.sum()) % 2 == 0, c, (c + W // 2) % W) / W
    _CACHE["rays"] = dict(track=k, ox=a[:, 1].copy(), oy=a[:, 2].copy(), dir=a[:, 3].copy(), progress=prog)
    return _CACHE["rays"]


def ray_details(rec, ox, oy, d):
    """Track.raycast (environment/track.py:173-199) in NumPy, vectorised over rays, with what the
    census needs: t (50 without a hit), parallel (|dotp| <= 1e-10 against some segment), vertex (a
    segment that gives the winning t is met at s exactly 0 or 1)."""
    s, v2 = rec["starts"], rec["v2"]
    c, sn = np.cos(d)[:, None], np.sin(d)[:, None]
    v3x, v3y = -sn, c
    v1x, v1y = ox[:, None] - s[None, :, 0], oy[:, None] - s[None, :, 1]
    dotp = v2[None, :, 0] * v3x + v2[None, :, 1] * v3y
    ok = np.abs(dotp) > 1e-10
    safe = np.where(ok, dotp, 1.0)
    t = np.where(ok, (v2[None, :, 0] * v1y - v2[None, :, 1] * v1x) / safe, 50.0)
    sv = np.where(ok, (v1x * v3x + v1y * v3y) / safe, -1.0)
    hit = ok & (t >= 0) & (sv >= 0) & (sv <= 1)
    th = np.where(hit, t, np.inf)
    tmin = th.min(1)
    win = hit & (th == tmin[:, None])
    return dict(t=np.where(np.isfinite(tmin), tmin, 50.0), parallel=(~ok).any(1),
                vertex=(win & ((sv == 0) | (sv == 1))).any(1), sin0=np.sin(d) == 0.0)


def census_rays(kat, t=None):
    """Per lattice track: the counts of each ray edge.  ``t``: the recorded Track.raycast results
    (default: the NumPy restatement's)."""
    out = {}
    for j, rec in enumerate(tracks()):
        m = kat["track"] == L0 + j
        ox, oy, d = kat["ox"][m], kat["oy"][m], kat["dir"][m]
        det = ray_details(rec, ox, oy, d)
        tt = det["t"] if t is None else t[m]
        c = dict(rows=int(m.sum()), sin0=int(det["sin0"].sum()), parallel=int(det["parallel"].sum()),
                 t0=int((tt == 0).sum()), t50=int((tt == 50).sum()), vertex=int(det["vertex"].sum()))
        for G in CULL_G:
            b = chunk_boxes(rec, G)
            c[f"plane_G{G}"] = int((np.isin(ox, b[:, [0, 2]]) | np.isin(oy, b[:, [1, 3]])).sum())
        out[rec["label"]] = c
    return out


# ------------------------------------------------------------------------------ single-agent step KATs
ANGLES = (0.0, HALF_PI, np.pi, 3 * HALF_PI)
SINGLE_COLS = ("track", "x", "y", "angle", "vx", "vy", "progress", "crashed", "finished", "steps", "last_progress",
               "last_steering", "cp", "action", "speed_weight")


def single_kats(seed=12, per_track=700):
    """step_single.npz's input columns.  Per track: 400 parked cars (v = 0, action 0) on 80 tie points
    x (0, pi/2, pi, 3 pi/2, one generic angle), 300 moving cars whose step crosses a tie point."""
    if "single" in _CACHE:
        return _CACHE["single"]
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in SINGLE_COLS}
    cols["parked"] = []
    for j, rec in enumerate(tracks()):
        wp, W = rec["wp"], len(rec["wp"])
        pts = tie_points(rec)
        n_park = (per_track * 4 // 7) // 5
        at = np.concatenate([_pick(rng, pts, n_park // 2, free_only=True), _pick(rng, pts, n_park - n_park // 2)])
        px, py = pts["x"][at], pts["y"][at]
        x = np.repeat(px, 5)
        y = np.repeat(py, 5)
        ang = np.tile(np.array(ANGLES + (0.0,)), len(at))
        ang[4::5] = rng.uniform(0, 2 * np.pi, len(at))
        vx, vy = np.zeros(len(x)), np.zeros(len(x))
        act = np.zeros((len(x), 2), np.float32)
        parked = np.ones(len(x), bool)
        # moving: the tie point lies half a step ahead
        n_mv = per_track - len(x)
        mv = _pick(rng, pts, n_mv)
        mv = mv[rng.integers(len(mv), size=n_mv)]
        head = np.where(rng.random(n_mv) < 0.6, np.array(ANGLES)[rng.integers(4, size=n_mv)],
                        rng.uniform(0, 2 * np.pi, n_mv))
        spd = rng.uniform(4.0, 28.0, n_mv)
        mvx, mvy = spd * np.cos(head), spd * np.sin(head)
        x = np.concatenate([x, pts["x"][mv] - mvx * 0.025])
        y = np.concatenate([y, pts["y"][mv] - mvy * 0.025])
        ang = np.concatenate([ang, head])
        vx, vy = np.concatenate([vx, mvx]), np.concatenate([vy, mvy])
        a2 = np.stack([rng.uniform(-0.3, 0.3, n_mv), rng.uniform(0.0, 1.0, n_mv)], 1).astype(np.float32)
        a2[rng.random(n_mv) < 0.3, 0] = 0.0
        act = np.concatenate([act, a2])
        parked = np.concatenate([parked, np.zeros(n_mv, bool)])
        n = len(x)
        c = closest(wp, x, y)
        far = np.arange(n) % 2 == 1
        prog = np.where(far, (c + W // 2) % W, c) / W
        bits = rng.integers(8, size=n)
        cols["track"].append(np.full(n, L0 + j, np.int64))
        cols["x"].append(x), cols["y"].append(y), cols["angle"].append(ang), cols["vx"].append(vx), cols["vy"].append(vy)
        cols["progress"].append(prog)
        cols["crashed"].append(np.zeros(n, bool)), cols["finished"].append(np.zeros(n, bool))
        cols["steps"].append(np.where(rng.random(n) < 0.1, 2999, rng.integers(0, 2900, n)).astype(np.int64))
        cols["last_progress"].append(np.where(rng.random(n) < 0.7, c / W, rng.choice([0.05, 0.95, 0.24, 0.49, 0.74], n)))
        cols["last_steering"].append(np.where(parked, 0.0, rng.uniform(-1, 1, n)))
        cols["cp"].append(np.stack([bits & 1, (bits >> 1) & 1, (bits >> 2) & 1], 1).astype(np.uint8))
        cols["action"].append(act)
        cols["speed_weight"].append(np.where(rng.random(n) < 0.6, 8.0, rng.uniform(8.0, 14.0, n)))
        cols["parked"].append(parked)
    _CACHE["single"] = {k: np.concatenate(v) for k, v in cols.items()}
    return _CACHE["single"]


def census_ties(track, x, y):
    """Per lattice track: rows whose point has a closest-waypoint tie, a non-neighbouring tie, a
    tie three or more wide.  x, y [n] or [n, 2] (two cars: a row counts if either car ties)."""
    out = {}
    x, y = np.asarray(x).reshape(len(track), -1), np.asarray(y).reshape(len(track), -1)
    for j, rec in enumerate(tracks()):
        m = track == L0 + j
        n, apart = zip(*(tie_kinds(rec["wp"], x[m, q], y[m, q]) for q in range(x.shape[1])))
        n, apart = np.stack(n, 1), np.stack(apart, 1)
        out[rec["label"]] = dict(rows=int(m.sum()), tie=int((n >= 2).any(1).sum()), apart=int(apart.any(1).sum()),
                                 wide=int((n >= 3).any(1).sum()))
    return out


# ------------------------------------------------------------------------------ two-car step KATs
MULTI_COLS = ("track", "order", "x", "y", "angle", "vx", "vy", "progress", "crashed", "finished", "has_crashed",
              "finished_step", "last_progress", "last_steering", "cp", "steps", "action")
# (dx, dy, angle of car 1) by kind; car 0 stands at angle 0 on a lattice point
HALF = ((0.5, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, -0.5, 0.0), (0.5, 0.0, np.pi), (0.0, 0.5, HALF_PI))
NEAR = ((0.25, 0.0, 0.0), (0.0, -0.25, 0.0), (-0.375, 0.0, np.pi), (0.25, 0.25, 0.0), (0.0, 0.4375, HALF_PI))
EDGE = ((6.0, 1.0, 0.0), (6.0, -1.0, 0.0), (7.5, 1.0, 0.0), (5.0, -1.0, np.pi), (-2.0, 4.0, 0.0), (2.0, 4.0, 0.0),
        (2.0, -4.0, 0.0), (-2.0, -3.5, 0.0), (1.0, 5.0, HALF_PI), (-1.0, -5.0, HALF_PI))
PLACE = ((0.0, 3.0, 0.0), (0.0, -3.0, 0.0), (0.0, 3.5, 0.0), (0.0, 2.5, np.pi))
FREE = ((3.0, 3.0, 0.3), (-4.5, 1.5, 2.0), (0.5, 0.5, 1.0), (9.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 2.0, 0.0))
KINDS = dict(half=HALF, edge=EDGE, place=PLACE, free=FREE, near=NEAR)


def multi_kats(seed=13, per_track=800):
    """step_multi.npz's input columns.  Car 0 at angle 0 on an integer or half-integer point inside the
    track, car 1 offset by one of KINDS' rows; both parked (action (0, -1): throttle 0).  `place` rows
    end the episode with equal scores: at step 2999 (truncation) or with both cars crashed before."""
    if "multi" in _CACHE:
        return _CACHE["multi"]
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in MULTI_COLS}
    cols["kind"] = []
    for j, rec in enumerate(tracks()):
        wp, W, w = rec["wp"], len(rec["wp"]), rec["width"]
        i = rng.integers(W, size=per_track)
        lat = rng.integers(-int(w) * 2 + 4, int(w) * 2 - 3, size=per_track) * 0.5  # half-integer lateral offsets
        if rec["label"] == "diamond40":  # moved along x, so the points stay on the half-integer grid
            bx, by = wp[i, 0] - np.where(wp[i, 0] >= 0, 1.0, -1.0) * np.clip(lat, -2.0, 2.0), wp[i, 1] + 0.0
        else:
            bx, by = wp[i, 0] + rec["nrm"][i, 0] * lat, wp[i, 1] + rec["nrm"][i, 1] * lat
        kind_names = list(KINDS)
        kind = np.arange(per_track) % len(KINDS)
        sub = rng.integers(64, size=per_track)
        off = np.array([KINDS[kind_names[k]][s % len(KINDS[kind_names[k]])] for k, s in zip(kind, sub)])
        x = np.stack([bx, bx + off[:, 0]], 1)
        y = np.stack([by, by + off[:, 1]], 1)
        ang = np.stack([np.zeros(per_track), off[:, 2]], 1)
        turn = rng.random(per_track) < 0.25  # the pair as a whole turned by pi: car 0 looks along -x
        x[turn, 1], y[turn, 1] = 2 * x[turn, 0] - x[turn, 1], 2 * y[turn, 0] - y[turn, 1]
        ang[turn] = np.where(ang[turn] == 0.0, np.pi, np.where(ang[turn] == np.pi, 0.0, ang[turn]))
        swap = rng.random(per_track) < 0.5  # which car is car 0
        x[swap], y[swap], ang[swap] = x[swap][:, ::-1], y[swap][:, ::-1], ang[swap][:, ::-1]
        c = np.stack([closest(wp, x[:, q], y[:, q]) for q in range(2)], 1)
        far = (np.arange(per_track) // len(KINDS)) % 2 == 1
        prog = np.where(far[:, None], (c + W // 2) % W, c) / W
        place = kind == 2
        crashed = np.zeros((per_track, 2), bool)
        both = place & (rng.random(per_track) < 0.5)
        crashed[both] = True
        steps = np.where(place & ~both, 2999, rng.integers(0, 2900, per_track))
        # equal scores need equal progress: the frozen cars of `both` keep what they are given
        prog[both, 1] = prog[both, 0]
        bits = rng.integers(8, size=(per_track, 2))
        n = per_track
        cols["track"].append(np.full(n, L0 + j, np.int64)), cols["order"].append(np.full(n, -1, np.int64))
        cols["x"].append(x), cols["y"].append(y), cols["angle"].append(ang)
        cols["vx"].append(np.zeros((n, 2))), cols["vy"].append(np.zeros((n, 2)))
        cols["progress"].append(prog), cols["crashed"].append(crashed), cols["finished"].append(np.zeros((n, 2), bool))
        cols["has_crashed"].append(crashed.copy())
        cols["finished_step"].append(np.full((n, 2), -1, np.int64))
        cols["last_progress"].append(np.where(rng.random((n, 2)) < 0.8, c / W, 0.5))
        cols["last_steering"].append(np.zeros((n, 2)))
        cols["cp"].append(np.stack([bits & 1, (bits >> 1) & 1, (bits >> 2) & 1], 2).astype(np.uint8))
        cols["steps"].append(steps.astype(np.int64))
        act = np.zeros((n, 2, 2), np.float32)
        act[:, :, 1] = -1.0
        cols["action"].append(act)
        cols["kind"].append(kind.astype(np.int64))
    _CACHE["multi"] = {k: np.concatenate(v) for k, v in cols.items()}
    return _CACHE["multi"]


def _car_corners(x, y, ang):
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    return np.stack([c * _LOCAL[:, 0] - s * _LOCAL[:, 1] + x[:, None], s * _LOCAL[:, 0] + c * _LOCAL[:, 1] + y[:, None]], 2)


def census_multi(kat, done=None, placement=None, progress=None, crashed=None):
    """Per lattice track, over both cars' 11 rays against the OTHER car (multi_track.py:5-41, NumPy):
    half (the origin exactly 0.5 from the other centre: not excluded), near (closer: excluded),
    along (|dotp| < 1e-10 against an edge the origin is collinear with), corner (an edge met at s
    exactly 0 or 1 with t >= 0), contact-free rows aside; tie: rows that end with equal placement
    scores (needs the step's outputs)."""
    out = {}
    x, y, ang = kat["x"], kat["y"], kat["angle"]
    n = len(x)
    half, near, along, corner = (np.zeros(n, bool) for _ in range(4))
    for q in range(2):
        o = 1 - q
        dist = np.linalg.norm(np.stack([x[:, o] - x[:, q], y[:, o] - y[:, q]], 1), axis=1)
        half |= dist == 0.5
        near |= dist < 0.5
        C = _car_corners(x[:, o], y[:, o], ang[:, o])
        for r in REL2:
            d = ang[:, q] + r
            v3 = np.stack([-np.sin(d), np.cos(d)], 1)
            for e in range(4):
                s0, s1 = C[:, e], C[:, (e + 1) % 4]
                v1 = np.stack([x[:, q], y[:, q]], 1) - s0
                v2 = s1 - s0
                dotp = (v2 * v3).sum(1)
                par = np.abs(dotp) < 1e-10
                cr = v2[:, 0] * v1[:, 1] - v2[:, 1] * v1[:, 0]
                along |= par & (np.abs(cr) < 1e-9) & (dist >= 0.5)
                safe = np.where(par, 1.0, dotp)
                t, sv = cr / safe, (v1 * v3).sum(1) / safe
                corner |= ~par & (t >= 0) & ((sv == 0) | (sv == 1)) & (dist >= 0.5)
    tie = np.zeros(n, bool)
    if done is not None:
        score = progress * 100 + (~crashed) * 10 + 1.0 / 10000  # place(): nobody finished in these KATs
        tie = done & (score[:, 0] == score[:, 1])
        assert np.all(placement[tie, 1] == 1), "equal scores: the sort puts car 1 first"
    for j, rec in enumerate(tracks()):
        m = kat["track"] == L0 + j
        out[rec["label"]] = dict(rows=int(m.sum()), half=int(half[m].sum()), near=int(near[m].sum()),
                                 along=int(along[m].sum()), corner=int(corner[m].sum()), tie=int(tie[m].sum()))
    return out


# ------------------------------------------------------------------------------ fixture views and states
class View:
    """The columns of one KAT set of lattice.npz (prefix ``ray_`` / ``single_`` / ``multi_``)."""

    def __init__(self, npz, prefix):
        self.npz, self.prefix = npz, prefix

    def __getitem__(self, k):
        return self.npz[self.prefix + k]


def ray_state(kat):
    """The single-agent state that casts the ray KATs: parked at the origin, sensor 5 (relative
    angle exactly 0) along `dir`."""
    n = len(kat["ox"])
    st = single_state(n)
    st["x"][:], st["y"][:], st["angle"][:] = kat["ox"], kat["oy"], kat["dir"]
    st["progress"][:] = st["last_progress"][:] = kat["progress"]
    st["track"][:] = kat["track"]
    return st


# ------------------------------------------------------------------------------ the oracle on the KATs
OBS_TOL = 1e-5  # tests/test_env_gpu.py: float observations and rewards against the reference


def oracle_rays(golden, orc):
    """[n, 11] float32: the normalised rays of the ray KATs."""
    return lc.state_obs(table(golden), orc, ray_state(ray_kats()))[:, :11]


def oracle_single(step, tab, orc):
    """(state after, (obs, reward, terminated, truncated, info)) of single-agent KAT columns."""
    from tests.golden_util import single_state_from
    st = single_state_from(step)
    return st, orc.single_step(tab, st, step["action"], REL1, speed_weight=step["speed_weight"])


def oracle_multi(step, tab, orc):
    """(state after, (obs, reward, done, done_all, truncated, placement, info)) of two-car KAT columns."""
    from tests.golden_util import multi_state_from
    st = multi_state_from(step)
    return st, orc.multi_step(tab, st, step["action"], REL2)


def comparable(fix, golden, oracle, oracle_dev):
    """Per KAT set the rows on which the glibc and the device-libm oracle builds agree: every mask
    and `progress` equal, the floats within OBS_TOL.  On these rows a kernel that equals the
    device-libm build must also meet the reference's recorded outputs (masks exactly, floats to
    OBS_TOL); tests/test_lattice_cpu.py caps the share of the other rows at 1 %."""
    tab = table(golden)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    rays = (np.abs(f64(oracle_rays(golden, oracle)) - oracle_rays(golden, oracle_dev)) <= OBS_TOL).all(1)
    (sa, a), (sb, b) = (oracle_single(View(fix, "single_"), tab, o) for o in (oracle, oracle_dev))
    single = (sa["flags"] == sb["flags"]) & (sa["steps"] == sb["steps"]) & (sa["progress"] == sb["progress"])
    single &= (a[2] == b[2]) & (a[3] == b[3])
    single &= (np.abs(f64(a[0]) - b[0]) <= OBS_TOL).all(1) & (np.abs(a[1] - b[1]) <= OBS_TOL)
    (sa, a), (sb, b) = (oracle_multi(View(fix, "multi_"), tab, o) for o in (oracle, oracle_dev))
    multi = (sa["flags"] == sb["flags"]).all(1) & (sa["progress"] == sb["progress"]).all(1)
    multi &= (sa["finished_step"] == sb["finished_step"]).all(1) & (sa["steps"] == sb["steps"])
    multi &= (a[2] == b[2]) & (a[3] == b[3]) & (a[4] == b[4]) & (a[5] == b[5]).all(1)
    multi &= (np.abs(f64(a[0]) - b[0]) <= OBS_TOL).all((1, 2)) & (np.abs(a[1] - b[1]) <= OBS_TOL).all(1)
    return dict(rays=rays, single=single, multi=multi)


# ------------------------------------------------------------------------------ parked traces
def parked_single(golden, oracle, per_track=40, seed=14):
    """PARKED_STEPS steps of v = 0, action 0 on non-crashed tie points of every lattice track (five
    angles each) and on the start poses of the two spline slots."""
    rng = np.random.default_rng(seed)
    tab = table(golden)
    rows = []
    for j, rec in enumerate(tracks()):
        pts = tie_points(rec)
        at = _pick(rng, pts, per_track, free_only=True)
        for a in range(5):
            ang = np.full(len(at), ANGLES[a]) if a < 4 else rng.uniform(0, 2 * np.pi, len(at))
            rows.append((np.full(len(at), L0 + j), pts["x"][at], pts["y"][at], ang))
    for k in range(L0):
        rows.append((np.full(24, k), np.full(24, tab.meta[k, 0]), np.full(24, tab.meta[k, 1]),
                     np.full(24, np.mod(tab.meta[k, 2], 2 * np.pi))))
    slot, x, y, ang = (np.concatenate(c) for c in zip(*rows))
    order = rng.permutation(len(slot))  # the 64 lanes of a wave stand on different tracks
    slot, x, y, ang = slot[order], x[order], y[order], ang[order]
    st = single_state(len(slot))
    st["track"][:], st["x"][:], st["y"][:], st["angle"][:] = slot, x, y, ang
    W = (tab.wp_off[slot + 1] - tab.wp_off[slot]).astype(np.int64)
    for e in range(len(slot)):
        c = int(closest(tab.waypoints(int(slot[e])), x[e:e + 1], y[e:e + 1])[0])
        st["progress"][e] = st["last_progress"][e] = (c if e % 2 == 0 else (c + W[e] // 2) % W[e]) / W[e]
    st["steps"][:] = rng.integers(0, 2000, len(slot))
    st["flags"][:] = (rng.integers(8, size=len(slot)) * F_CP25).astype(np.uint8)  # any checkpoint flags
    keep = _stays_free(tab, oracle, st)
    st = {k: np.ascontiguousarray(v[keep]) for k, v in st.items()}
    return lc.run_single(tab, oracle, st, PARKED_STEPS, actions=np.zeros((PARKED_STEPS, len(st["x"]), 2), np.float32))


def _stays_free(tab, oracle, st):
    """The envs whose parked car is not crashed after one oracle step (generic angles may touch a wall)."""
    from oracle.orc import F_CRASHED
    probe = {k: v.copy() for k, v in st.items()}
    oracle.single_step(tab, probe, np.zeros((len(st["x"]), 2), np.float32), REL1)
    return (probe["flags"] & F_CRASHED) == 0


def parked_multi(golden, oracle, per_track=50, seed=15, draw_seed=78):
    """As parked_single for two cars side by side at angle 0 (action (0, -1)): car 1 is 3 to the
    side of car 0 where both stay inside the track."""
    from oracle.orc import F_CRASHED
    rng = np.random.default_rng(seed)
    tab = table(golden)
    rows = []
    for j, rec in enumerate(tracks()):
        pts = tie_points(rec)
        at = _pick(rng, pts, 4 * per_track, free_only=True)
        for dx, dy in ((0.0, 3.0), (0.0, -3.0), (3.0, 0.0), (-3.0, 0.0), (4.5, 0.5)):
            x1, y1 = pts["x"][at] + dx, pts["y"][at] + dy
            ok = ~crashed_at(rec, x1, y1, np.zeros(len(at)))
            rows.append((np.full(ok.sum(), L0 + j), pts["x"][at][ok], pts["y"][at][ok], x1[ok], y1[ok],
                         pts["apart"][at][ok]))
    slot, x0, y0, x1, y1, apart = (np.concatenate(c) for c in zip(*rows))
    order = rng.permutation(len(slot))
    order = np.concatenate([order[apart[order]][:per_track], order[~apart[order]]])[:3 * per_track]  # rare ties first
    order = rng.permutation(order)
    slot, x0, y0, x1, y1 = slot[order], x0[order], y0[order], x1[order], y1[order]
    n = len(slot)
    st = multi_state(n)
    st["track"][:] = slot
    st["x"][:], st["y"][:] = np.stack([x0, x1], 1), np.stack([y0, y1], 1)
    for e in range(n):
        wp = tab.waypoints(int(slot[e]))
        W = len(wp)
        for q in range(2):
            c = int(closest(wp, st["x"][e, q:q + 1], st["y"][e, q:q + 1])[0])
            st["progress"][e, q] = st["last_progress"][e, q] = (c if e % 2 == 0 else (c + W // 2) % W) / W
    st["steps"][:] = rng.integers(0, 2000, n)
    act = np.zeros((PARKED_STEPS, n, 2, 2), np.float32)
    act[..., 1] = -1.0
    probe = {k: v.copy() for k, v in st.items()}
    oracle.multi_step(tab, probe, act[0], REL2)
    keep = ((probe["flags"] & F_CRASHED) == 0).all(1)
    st = {k: np.ascontiguousarray(v[keep]) for k, v in st.items()}
    return lc.run_multi(tab, oracle, st, PARKED_STEPS, draw_seed, actions=np.ascontiguousarray(act[:, keep]))


_BUILDERS = {"parked_single": parked_single, "parked_multi": parked_multi}


def get(name, golden, oracle):
    """The named trace on the device-libm oracle, built once and shared (read only)."""
    assert oracle.device_libm
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name](golden, oracle)
    return _CACHE[name]
