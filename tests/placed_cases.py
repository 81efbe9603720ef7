"""Placed tracks: the culling margins away from the origin and from unit scale (DESIGN.md §4
"Placed tracks").

Every bound by which the ray kernels and the closest-waypoint search skip work is a function
of magnitudes -- mb, mt ~ L (Rr, T) 1e10 2^-52; mbf adds 3 (|ox| + |oy| + 1) 2^-24 +
(|ox| + |oy| + mbf0) 2^-22; e2 = 2^-17 (|ox| + |oy| + |cx| + |cy| + 2 rad + L + 1) -- and the
generator's tracks (radius 50 .. 120 round the origin) and the lattice tracks ([-40, 100]) hold
every one of them at one size.  Here the same two spline tracks stand elsewhere and at other
sizes: their waypoints and width mapped by p -> s p + c.

Slots of the table (and of the env's TrackSet):

    0, 1       the golden spline tracks 0 and 16 (the default track), unchanged: controls
    2          the lattice track diamond40, unchanged
    3 + 7 b + m  base track b (0: golden 0, 1: golden 16) under map m of ``MAPS``

The mapped array IS the track (TrackGeometry.from_waypoints, as the lattice slots): the oracle's
TrackTable and the device table come from the same arrays, nothing depends on the map being
exact.  For s = 64 the longest segment is ~99 and mb ~ 5 (the L^2 growth); for s = 1/16 the
4 x 2 car is wider than the track; at |c| = 2^26 float32 resolves a position to 8 units.

KAT inputs, pure NumPy (tests/golden/gen_golden.py's ``placed`` target feeds a thinned half of
them to the reference, tests/golden/placed.npz holds what it answered):

* ``ray_kats``     ~300 per slot, (track, ox, oy, dir, progress) + okind, dkind: origins on the centre
                   line, both walls and boundary vertices; on the planes of the chunk boxes for
                   G = 6, 8, 16 beside the vertex that spans them, and 1e-9 max(1, |coord|) to
                   either side; at the slot's circle centre and 2, 10, 100 radii outside it;
                   directions aimed at one of the nearest vertices, random, k pi / 2 and their
                   1-ulp neighbours; `progress` (the visit-order hint) at the nearest waypoint on
                   even rows, half a lap away on odd ones.
* ``single_kats``  ~150 per slot: poses along the centre line at mixed speeds and steering, a third
                   of them straddling a wall; `progress` near the answer or half a lap away (the
                   window miss of argmin_culled's phase 2); per-env speed weights.
* ``multi_kats``   on slots (0, (-2^20, 3 2^18)) and (0, s = 16): the lattice set's two-car offsets
                   (lattice_cases.KINDS) round half-integer points of the placed track -- moved
                   with the track, not scaled with it.
* ``trace``        24 steps of cars driving on the two (1, (-2^20, 3 2^18)) slots with the golden
                   trajectories' actions, stepped by the device-libm oracle (lap_cases.run_single).

``census`` counts per slot what the cases exist for; tests/test_placed_cpu.py holds it to floors.
"""
import numpy as np

from oracle.orc import F_CRASHED, TrackTable
from tests import lap_cases as lc
from tests import lattice_cases as lat

REL1, REL2 = lat.REL1, lat.REL2
BASES = (0, 16)  # golden tracks
MAPS = ((1.0, (1e3, -1e3)), (1.0, (2.0 ** 17, 2.0 ** 17)), (1.0, (-2.0 ** 20, 3 * 2.0 ** 18)),
        (1.0, (2.0 ** 26, -2.0 ** 26)), (1.0 / 16, (0.0, 0.0)), (16.0, (0.0, 0.0)), (64.0, (2.0 ** 17, 0.0)))
N_CONTROL = 3
N_SLOTS = N_CONTROL + len(BASES) * len(MAPS)
CULL_G = lat.CULL_G
MAX_RANGE = 50.0  # RX_MAX_RANGE
WINDOW = 2        # the default argmin_window (rx_assign_plan.h)
TRACE_STEPS = 24
MULTI_SLOTS = (3 + 2, 3 + 5)   # base 0 at (-2^20, 3 2^18); base 0 at s = 16
TRACE_SLOTS = (3 + 2, 10 + 2)  # both bases at (-2^20, 3 2^18)
OKINDS = ("centre_line", "wall", "vertex", "plane", "beside_plane", "circle_centre", "outside2", "outside10",
          "outside100")
DKINDS = ("aimed", "random", "axis", "axis_ulp")
_CACHE = {}


def _copy(kat):
    """The KAT sets are handed out as copies: the oracle steps the arrays it is given in place."""
    return {k: v.copy() for k, v in kat.items()}


def slot_of(base, m):
    return N_CONTROL + len(MAPS) * base + m


def slot_map(k):
    """(s, (cx, cy)) of slot k (the controls: the identity)."""
    return (1.0, (0.0, 0.0)) if k < N_CONTROL else MAPS[(k - N_CONTROL) % len(MAPS)]


# ------------------------------------------------------------------------------ tracks
def _placed(rec, s, c, label):
    from rx.track import TrackGeometry
    wp = np.ascontiguousarray(rec["wp"] * s + np.array(c))
    width = float(rec["width"] * s)
    g = TrackGeometry.from_waypoints(wp, width, wp)
    st = g.get_start_pos()
    return dict(cp=wp, wp=g.waypoints, nrm=g.normals, starts=g.segment_cache["starts"], v2=g.segment_cache["v2"],
                start=np.array([float(st[0]), float(st[1]), float(st[2])]), width=width,
                maxd=float(g.max_track_distance), label=label)


def slot_records(golden):
    if "recs" not in _CACHE:
        recs = [golden.tracks[k] for k in BASES] + [lat.tracks()[lat.NAMES.index("diamond40")]]
        for b, k in enumerate(BASES):
            for m, (s, c) in enumerate(MAPS):
                recs.append(_placed(golden.tracks[k], s, c, f"placed[{b}][{m}]"))
        _CACHE["recs"] = recs
    return _CACHE["recs"]


def labels():
    return ["golden0", "golden16", "diamond40"] + [f"t{k}*{s:g}+({c[0]:g},{c[1]:g})" for k in BASES for s, c in MAPS]


def table(golden):
    if "table" not in _CACHE:
        _CACHE["table"] = TrackTable(slot_records(golden))
    return _CACHE["table"]


def _is_waypoint_slot(rec):
    return rec["label"] == "diamond40" or rec["label"].startswith("placed")


def track_set(golden):
    """A TrackSet whose slots are ``slot_records``: the spline slots from their control points, the
    others from their waypoints (keyed by the waypoint array)."""
    from rx.track import TrackGeometry, TrackSet
    ts = TrackSet()
    for rec in slot_records(golden):
        if _is_waypoint_slot(rec):
            ts._index[TrackSet._key(rec["cp"], rec["width"])] = len(ts.geoms)
            ts.geoms.append(TrackGeometry.from_waypoints(rec["cp"], rec["width"], rec["wp"]))
            ts._packed = None
        else:
            ts.slot(lat._cp(rec), rec["width"])
    return ts


def env_args(golden, slots):
    """(control_points, widths, track_set) for RacingVectorEnv with env e on slot slots[e]."""
    recs = slot_records(golden)
    cps = [lat._cp(r) for r in recs]
    return [cps[k] for k in slots], [recs[k]["width"] for k in slots], track_set(golden)


def circle(rec):
    """(cx, cy, rad) as rx_cull_geo: the centre of the box of all boundary points and the reach."""
    p = np.concatenate([rec["starts"], rec["starts"] + rec["v2"]])
    c = 0.5 * (p.min(0) + p.max(0))
    return c[0], c[1], float(np.hypot(p[:, 0] - c[0], p[:, 1] - c[1]).max())


# ------------------------------------------------------------------------------ ray KATs
def _nearest_vertices(rec, ox, oy, k=6):
    s = rec["starts"]
    return s[np.argsort((s[:, 0] - ox) ** 2 + (s[:, 1] - oy) ** 2)[:k]]


def _ray_origins(rec, scale, rng):
    """[(okind, x, y)]"""
    wp, s, v2 = rec["wp"], rec["starts"], rec["v2"]
    pick = lambda n, k: rng.permutation(n)[:k]  # noqa: E731
    out = [(0, *wp[i]) for i in pick(len(wp), 12)]
    out += [(1, *(s[i] + v2[i] * f)) for i, f in zip(pick(len(s), 24), rng.choice([0.5, 0.25, 0.75], 24))]
    out += [(2, *s[i]) for i in pick(len(s), 20)]
    reach = 12.0 * min(1.0, scale)
    verts = np.concatenate([s, s + v2])
    for G in CULL_G:
        b = lat.chunk_boxes(rec, G)
        for row, j in enumerate(pick(len(b), 4)):
            for a in range(4):  # the plane x = x0, y = y0, x = x1, y = y1 beside the vertex that spans it
                v = verts[np.flatnonzero(verts[:, a % 2] == b[j, a])[0]]
                p = v.copy()
                p[1 - a % 2] += rng.uniform(-reach, reach)
                out.append((3, *p))
                if (row + a) % 2 == 0:  # 1e-9 max(1, |coord|) to one side
                    q = p.copy()
                    q[a % 2] += (1.0 if (row // 2 + a // 2) % 2 else -1.0) * 1e-9 * max(1.0, abs(q[a % 2]))
                    out.append((4, *q))
    cx, cy, rad = circle(rec)
    out += [(5, cx, cy)] * 5
    for kind, m in ((6, 2.0), (7, 10.0), (8, 100.0)):
        for a in rng.uniform(-np.pi, np.pi, 5):
            out.append((kind, cx + (1.0 + m) * rad * np.cos(a), cy + (1.0 + m) * rad * np.sin(a)))
    return out


def ray_kats(golden, seed=21):
    """dict track, ox, oy, dir, progress, okind, dkind."""
    if "rays" in _CACHE:
        return _copy(_CACHE["rays"])
    rng = np.random.default_rng(seed)
    base, ulps, _ = lat._directions()
    rows = []
    for k, rec in enumerate(slot_records(golden)):
        scale = slot_map(k)[0]
        for i, (okind, ox, oy) in enumerate(_ray_origins(rec, scale, rng)):
            near = _nearest_vertices(rec, ox, oy)
            v = near[rng.integers(len(near))]
            if v[0] == ox and v[1] == oy:
                v = near[1] if (near[0] == v).all() else near[0]
            aimed = np.arctan2(v[1] - oy, v[0] - ox)
            other = (rng.uniform(-np.pi, np.pi), rng.choice(base), rng.choice(ulps))[i % 3]
            rows += [(k, ox, oy, float(aimed), okind, 0), (k, ox, oy, float(other), okind, 1 + i % 3)]
    a = np.array(rows)
    trk = a[:, 0].astype(np.int64)
    prog = np.zeros(len(a))
    for k, rec in enumerate(slot_records(golden)):
        m = trk == k
        W = len(rec["wp"])
        c = lat.closest(rec["wp"], a[m, 1], a[m, 2])
        prog[m] = np.where(np.arange(m.sum()) % 4 < 2, c, (c + W // 2) % W) / W  # pairs share an origin
    _CACHE["rays"] = dict(track=trk, ox=a[:, 1].copy(), oy=a[:, 2].copy(), dir=a[:, 3].copy(), progress=prog,
                          okind=a[:, 4].astype(np.int64), dkind=a[:, 5].astype(np.int64))
    return _copy(_CACHE["rays"])


def ray_t(rec, ox, oy, d):
    """Track.raycast's minimum over the hit segments (environment/track.py:173-199) in NumPy; inf
    without a hit."""
    s, v2 = rec["starts"], rec["v2"]
    v3x, v3y = -np.sin(d)[:, None], np.cos(d)[:, None]
    v1x, v1y = ox[:, None] - s[None, :, 0], oy[:, None] - s[None, :, 1]
    dotp = v2[None, :, 0] * v3x + v2[None, :, 1] * v3y
    ok = np.abs(dotp) > 1e-10
    safe = np.where(ok, dotp, 1.0)
    t = (v2[None, :, 0] * v1y - v2[None, :, 1] * v1x) / safe
    sv = (v1x * v3x + v1y * v3y) / safe
    return np.where(ok & (t >= 0) & (sv >= 0) & (sv <= 1), t, np.inf).min(1)


def on_plane(rec, ox, oy):
    m = np.zeros(len(ox), bool)
    for G in CULL_G:
        b = lat.chunk_boxes(rec, G)
        m |= np.isin(ox, b[:, [0, 2]]) | np.isin(oy, b[:, [1, 3]])
    return m


# ------------------------------------------------------------------------------ single-agent step KATs
SINGLE_COLS = lat.SINGLE_COLS


def single_kats(golden, seed=22, per_slot=150):
    if "single" in _CACHE:
        return _copy(_CACHE["single"])
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in SINGLE_COLS}
    for k, rec in enumerate(slot_records(golden)):
        wp, nrm, W, w = rec["wp"], rec["nrm"], len(rec["wp"]), rec["width"]
        n = per_slot
        i = rng.integers(W, size=n)
        straddle = np.arange(n) % 3 == 0  # a corner of the car beyond the wall
        latl = np.where(straddle, rng.choice([-1.0, 1.0], n) * w * rng.uniform(0.75, 1.05, n), rng.uniform(-0.5, 0.5, n) * w)
        x, y = wp[i, 0] + nrm[i, 0] * latl, wp[i, 1] + nrm[i, 1] * latl
        nxt = wp[(i + 1) % W] - wp[i]
        ang = np.mod(np.arctan2(nxt[:, 1], nxt[:, 0]) + rng.normal(0.0, 0.3, n), 2 * np.pi)
        spd = np.where(rng.random(n) < 0.2, 0.0, rng.uniform(0.0, 29.0, n))
        drift = rng.normal(0.0, 0.15, n)
        vx, vy = spd * np.cos(ang + drift), spd * np.sin(ang + drift)
        c = lat.closest(wp, x, y)
        far = np.arange(n) % 2 == 1
        bits = rng.integers(8, size=n)
        act = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 1.0, n)], 1).astype(np.float32)
        act[rng.random(n) < 0.2, 0] = 0.0
        cols["track"].append(np.full(n, k, np.int64))
        cols["x"].append(x), cols["y"].append(y), cols["angle"].append(ang), cols["vx"].append(vx), cols["vy"].append(vy)
        cols["progress"].append(np.where(far, (c + W // 2) % W, c) / W)
        cols["crashed"].append(np.zeros(n, bool)), cols["finished"].append(np.zeros(n, bool))
        cols["steps"].append(np.where(rng.random(n) < 0.1, 2999, rng.integers(0, 2900, n)).astype(np.int64))
        cols["last_progress"].append(np.where(rng.random(n) < 0.7, c / W, rng.choice([0.05, 0.95, 0.24, 0.49, 0.74], n)))
        cols["last_steering"].append(rng.uniform(-1, 1, n))
        cols["cp"].append(np.stack([bits & 1, (bits >> 1) & 1, (bits >> 2) & 1], 1).astype(np.uint8))
        cols["action"].append(act)
        cols["speed_weight"].append(np.where(rng.random(n) < 0.6, 8.0, rng.uniform(8.0, 14.0, n)))
    _CACHE["single"] = {k: np.concatenate(v) for k, v in cols.items()}
    return _copy(_CACHE["single"])


# ------------------------------------------------------------------------------ two-car step KATs
MULTI_COLS = lat.MULTI_COLS


def multi_kats(golden, seed=23, per_slot=400):
    """lattice_cases.multi_kats' poses on the placed slots: car 0 at angle 0 on a half-integer point
    near the centre line, car 1 offset by a row of lattice_cases.KINDS (not scaled), both parked."""
    if "multi" in _CACHE:
        return _copy(_CACHE["multi"])
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in MULTI_COLS}
    cols["kind"] = []
    kind_names = list(lat.KINDS)
    for k in MULTI_SLOTS:
        rec = slot_records(golden)[k]
        wp, nrm, W, w = rec["wp"], rec["nrm"], len(rec["wp"]), rec["width"]
        n = per_slot
        i = rng.integers(W, size=n)
        latl = rng.uniform(-0.6, 0.6, n) * min(w, 9.0)
        bx = np.rint(2.0 * (wp[i, 0] + nrm[i, 0] * latl)) / 2.0  # half-integer grid: the offsets stay exact
        by = np.rint(2.0 * (wp[i, 1] + nrm[i, 1] * latl)) / 2.0
        kind = np.arange(n) % len(lat.KINDS)
        sub = rng.integers(64, size=n)
        off = np.array([lat.KINDS[kind_names[a]][s % len(lat.KINDS[kind_names[a]])] for a, s in zip(kind, sub)])
        x, y = np.stack([bx, bx + off[:, 0]], 1), np.stack([by, by + off[:, 1]], 1)
        ang = np.stack([np.zeros(n), off[:, 2]], 1)
        turn = rng.random(n) < 0.25
        x[turn, 1], y[turn, 1] = 2 * x[turn, 0] - x[turn, 1], 2 * y[turn, 0] - y[turn, 1]
        ang[turn] = np.where(ang[turn] == 0.0, np.pi, np.where(ang[turn] == np.pi, 0.0, ang[turn]))
        swap = rng.random(n) < 0.5
        x[swap], y[swap], ang[swap] = x[swap][:, ::-1], y[swap][:, ::-1], ang[swap][:, ::-1]
        c = np.stack([lat.closest(wp, x[:, q], y[:, q]) for q in range(2)], 1)
        far = (np.arange(n) // len(lat.KINDS)) % 2 == 1
        prog = np.where(far[:, None], (c + W // 2) % W, c) / W
        place = kind == 2
        crashed = np.zeros((n, 2), bool)
        both = place & (rng.random(n) < 0.5)
        crashed[both] = True
        steps = np.where(place & ~both, 2999, rng.integers(0, 2900, n))
        prog[both, 1] = prog[both, 0]
        bits = rng.integers(8, size=(n, 2))
        cols["track"].append(np.full(n, k, np.int64)), cols["order"].append(np.full(n, -1, np.int64))
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
    return _copy(_CACHE["multi"])


# ------------------------------------------------------------------------------ the reference's share
def thinned(kat, per_slot, seed):
    """Row indices of at most per_slot rows of every slot (the rows tests/golden/placed.npz pins)."""
    rng = np.random.default_rng(seed)
    idx = []
    for k in np.unique(kat["track"]):
        rows = np.flatnonzero(kat["track"] == k)
        idx.append(np.sort(rng.permutation(rows)[:per_slot]))
    return np.concatenate(idx)


PIN = dict(ray=(150, 31), single=(60, 32), multi=(150, 33))  # (rows per slot, seed) of placed.npz


def pinned(golden, name):
    """(row indices, the KAT columns on those rows) of the set the reference answered."""
    kat = dict(ray=ray_kats, single=single_kats, multi=multi_kats)[name](golden)
    idx = thinned(kat, *PIN[name])
    return idx, {k: v[idx] for k, v in kat.items()}


# ------------------------------------------------------------------------------ the oracle on the KATs
def oracle_rays(golden, orc, kat=None):
    """[n, 11] float32: the normalised rays of the ray KATs."""
    return lc.state_obs(table(golden), orc, lat.ray_state(kat or ray_kats(golden)))[:, :11]


def comparable(fix, golden, oracle, oracle_dev):
    """lattice_cases.comparable's rule on the pinned rows of placed.npz: the rows on which the
    glibc and the device-libm oracle builds agree."""
    tab = table(golden)
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    rk = lat.View(fix, "ray_")
    rays = (np.abs(f64(oracle_rays(golden, oracle, rk)) - oracle_rays(golden, oracle_dev, rk)) <= lat.OBS_TOL).all(1)
    (sa, a), (sb, b) = (lat.oracle_single(lat.View(fix, "single_"), tab, o) for o in (oracle, oracle_dev))
    single = (sa["flags"] == sb["flags"]) & (sa["steps"] == sb["steps"]) & (sa["progress"] == sb["progress"])
    single &= (a[2] == b[2]) & (a[3] == b[3])
    single &= (np.abs(f64(a[0]) - b[0]) <= lat.OBS_TOL).all(1) & (np.abs(a[1] - b[1]) <= lat.OBS_TOL)
    (sa, a), (sb, b) = (lat.oracle_multi(lat.View(fix, "multi_"), tab, o) for o in (oracle, oracle_dev))
    multi = (sa["flags"] == sb["flags"]).all(1) & (sa["progress"] == sb["progress"]).all(1)
    multi &= (sa["finished_step"] == sb["finished_step"]).all(1) & (sa["steps"] == sb["steps"])
    multi &= (a[2] == b[2]) & (a[3] == b[3]) & (a[4] == b[4]) & (a[5] == b[5]).all(1)
    multi &= (np.abs(f64(a[0]) - b[0]) <= lat.OBS_TOL).all((1, 2)) & (np.abs(a[1] - b[1]) <= lat.OBS_TOL).all(1)
    return dict(rays=rays, single=single, multi=multi)


# ------------------------------------------------------------------------------ census
def census(golden, orc):
    """Per slot (``labels()``): rays, in_range (a wall hit inside RX_MAX_RANGE), no_hit, plane (origins
    on a chunk-box plane), the rows of every origin and direction kind; steps, crash (steps that end
    crashed), window_miss (the closest waypoint of the car AFTER the step lies outside +-WINDOW of
    the injected `progress`)."""
    from tests.golden_util import single_state_from
    rk, sk = ray_kats(golden), single_kats(golden)
    tab = table(golden)
    st0 = single_state_from(single_kats(golden))  # (a copy: the oracle steps sk's arrays in place)
    st, _ = lat.oracle_single(sk, tab, orc)
    out = {}
    for k, (rec, name) in enumerate(zip(slot_records(golden), labels())):
        m = rk["track"] == k
        t = ray_t(rec, rk["ox"][m], rk["oy"][m], rk["dir"][m])
        c = dict(rays=int(m.sum()), in_range=int((t < MAX_RANGE).sum()), no_hit=int(np.isinf(t).sum()),
                 plane=int(on_plane(rec, rk["ox"][m], rk["oy"][m]).sum()))
        for j, o in enumerate(OKINDS):
            c["o_" + o] = int((rk["okind"][m] == j).sum())
        for j, d in enumerate(DKINDS):
            c["d_" + d] = int((rk["dkind"][m] == j).sum())
        m = sk["track"] == k
        W = len(rec["wp"])
        prev = np.rint(st0["progress"][m] * W).astype(np.int64)
        now = lat.closest(rec["wp"], st["x"][m], st["y"][m])
        gap = np.abs((now - prev + W // 2) % W - W // 2)
        c.update(steps=int(m.sum()), crash=int(((st["flags"][m] & F_CRASHED) != 0).sum()), window_miss=int((gap > WINDOW).sum()))
        out[name] = c
    return out


# ------------------------------------------------------------------------------ the trace
def trace(golden, oracle, n=192, seed=24):
    """TRACE_STEPS steps on the two TRACE_SLOTS: env e starts on waypoint ~ e W / n of its slot at
    speed U(4, 20) along the track and replays the first 24 actions of golden trajectory e mod 8
    (traj_single.npz: the scripted controllers' float32 actions); next-step autoreset."""
    rng = np.random.default_rng(seed)
    tab = table(golden)
    tj = golden["traj_single"]
    off = tj["off"]
    assert np.all(np.diff(off) >= TRACE_STEPS)
    slots = np.asarray(TRACE_SLOTS, np.int32)[rng.integers(len(TRACE_SLOTS), size=n)]
    st, _ = lc.single_state0(tab, slots, seed, horizon=TRACE_STEPS, extras=False)
    for e in range(n):
        s = int(slots[e])
        W = int(tab.wp_off[s + 1] - tab.wp_off[s])
        i = int(rng.integers(W))
        x, y, ang, vx, vy = lc._pose(tab, s, i, float(rng.uniform(4.0, 20.0)), lateral=float(rng.uniform(-2.0, 2.0)))
        st["x"][e], st["y"][e], st["angle"][e], st["vx"][e], st["vy"][e] = x, y, ang, vx, vy
        st["progress"][e] = st["last_progress"][e] = i / W
        st["flags"][e] = lc._cp_flags(i, W)
    acts = np.stack([tj["actions"][off[e % 8]:off[e % 8] + TRACE_STEPS] for e in range(n)], 1)
    return lc.run_single(tab, oracle, st, TRACE_STEPS, actions=np.ascontiguousarray(acts, dtype=np.float32))


def get(name, golden, oracle):
    """The trace on the device-libm oracle, built once and shared (read only)."""
    assert oracle.device_libm and name == "trace"
    if name not in _CACHE:
        _CACHE[name] = trace(golden, oracle)
    return _CACHE[name]
