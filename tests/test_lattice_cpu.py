"""Lattice-track cases on the CPU (DESIGN.md §4 "Lattice tracks"; tests/lattice_cases.py).

tests/golden/lattice.npz holds what the reference answered to the KATs on its own Track
with gen_waypoints overridden.  Here: the geometry the reference derived equals
TrackGeometry.from_waypoints byte for byte; the glibc oracle (and NpTrack.raycast for the
rays) reproduces every recorded output bit for bit; the census of the edges the cases
exist for stays above its floors; the device-libm oracle build -- the checker of the GPU
tests -- agrees with the glibc build on all but at most 1 % of the rows; a parked car
repeats step 0 for 24 steps; and the shared host pieces (rx_build_cull_tables_host, the
float32 segment pre-filter's emulation) are exact on these tables.
"""
import numpy as np
import pytest

from oracle.orc import F_CRASHED
from tests import lattice_cases as lat
from tests import test_cull_tables_cpu as ct
from tests import test_oracle_golden as og
from tests import test_prefilter_cpu as pf

TOTAL_FLOOR, TRACK_FLOOR = 200, 50
CAP = 0.01


@pytest.fixture(scope="module")
def fix(golden):
    return golden["lattice"]


def _off(fix, key, j):
    o = fix["geo_" + key + "_off"]
    return fix["geo_" + key][o[j]:o[j + 1]]


def test_reference_geometry_equals_from_waypoints(fix):
    assert [str(s) for s in fix["geo_labels"]] == list(lat.NAMES)
    for j, rec in enumerate(lat.tracks()):
        for key in ("wp", "nrm", "starts", "v2"):
            ref = _off(fix, key, j)
            assert ref.dtype == rec[key].dtype and ref.shape == rec[key].shape, (j, key)
            assert ref.tobytes() == np.ascontiguousarray(rec[key]).tobytes(), (j, key)
        assert fix["geo_start"][j].tobytes() == rec["start"].tobytes()
        assert fix["geo_maxd"][j] == rec["maxd"] and fix["geo_width"][j] == rec["width"]
    # the rectangles: unit axis normals, integer boundary vertices; the diamond: neither
    for j in (0, 1):
        rec = lat.tracks()[j]
        assert np.all(np.isin(rec["nrm"], (-1.0, 0.0, 1.0))) and np.all(rec["starts"] == np.rint(rec["starts"]))
    assert not np.any(np.isin(lat.tracks()[2]["nrm"], (-1.0, 0.0, 1.0)))
    W = [len(r["wp"]) for r in lat.tracks()]
    assert any(w % 8 for w in W) and all(w > 64 for w in W), W


def test_fixture_inputs_are_the_cases(fix):
    """The committed inputs are what tests/lattice_cases.py builds today."""
    for prefix, kat, cols in (("ray_", lat.ray_kats(), ("track", "ox", "oy", "dir", "progress")),
                              ("single_", lat.single_kats(), lat.SINGLE_COLS + ("parked",)),
                              ("multi_", lat.multi_kats(), lat.MULTI_COLS + ("kind",))):
        for k in cols:
            assert np.array_equal(fix[prefix + k], kat[k]), prefix + k
        assert 2000 <= len(kat["track"]) <= 4096, (prefix, len(kat["track"]))


def test_rays_bit_exact(fix, golden, oracle):
    from oracle.np_env import make_track
    tab = lat.table(golden)
    rc = lat.View(fix, "ray_")
    got = np.array([oracle.raycast(tab.segments(int(k)), ox, oy, d)
                    for k, ox, oy, d in zip(rc["track"], rc["ox"], rc["oy"], rc["dir"])])
    assert np.array_equal(got, rc["t"])
    nt = {lat.L0 + j: make_track(rec) for j, rec in enumerate(lat.tracks())}
    got = np.array([nt[int(k)].raycast(np.array([ox, oy]), d)
                    for k, ox, oy, d in zip(rc["track"], rc["ox"], rc["oy"], rc["dir"])])
    assert np.array_equal(got, rc["t"])
    for j, rec in enumerate(lat.tracks()):  # the census' own restatement
        m = rc["track"] == lat.L0 + j
        assert np.array_equal(lat.ray_details(rec, rc["ox"][m], rc["oy"][m], rc["dir"][m])["t"], rc["t"][m])


def test_closest_waypoint_on_every_tie_point(oracle, oracle_dev):
    """First index on ties: both oracle builds against np.argmin on every tie point of the grid."""
    for rec in lat.tracks():
        p = lat.tie_points(rec)
        want = lat.closest(rec["wp"], p["x"], p["y"])
        for orc in (oracle, oracle_dev):
            got = np.array([orc.closest_wp(rec["wp"], x, y) for x, y in zip(p["x"], p["y"])])
            assert np.array_equal(got, want), rec["label"]


def test_single_steps_bit_exact(fix, golden, oracle):
    step = lat.View(fix, "single_")
    st, out = lat.oracle_single(step, lat.table(golden), oracle)
    og._check_single(step, st, *out, exact=True)


def test_multi_steps_bit_exact(fix, golden, oracle):
    step = lat.View(fix, "multi_")
    st, out = lat.oracle_multi(step, lat.table(golden), oracle)
    og._check_multi(step, st, *out, exact=True)


# ------------------------------------------------------------------------------ census floors
def _floors(census, kinds, what):
    print(f"\n{what}: " + "; ".join(f"{t}: " + ", ".join(f"{k} {c[k]}" for k in ("rows",) + tuple(kinds))
                                    for t, c in census.items()))
    for k in kinds:
        per = [c[k] for c in census.values()]
        assert sum(per) >= TOTAL_FLOOR, (what, k, per)
        assert min(per) >= TRACK_FLOOR, (what, k, per)


def test_census_floors(fix):
    rc = lat.View(fix, "ray_")
    _floors(lat.census_rays(lat.ray_kats(), rc["t"]),
            ("sin0", "parallel", "t0", "t50", "vertex") + tuple(f"plane_G{G}" for G in lat.CULL_G), "rays")
    # where the car stands after the step (a parked car: where it stood)
    s = lat.View(fix, "single_")
    _floors(lat.census_ties(s["track"], s["o_x"], s["o_y"]), ("tie", "apart", "wide"), "single steps")
    p = s["parked"]
    assert np.array_equal(s["o_x"][p], s["x"][p]) and np.array_equal(s["o_y"][p], s["y"][p])  # parked: stayed
    _floors(lat.census_ties(s["track"][p], s["x"][p], s["y"][p]), ("tie", "apart", "wide"), "parked single steps")
    m = lat.View(fix, "multi_")
    assert np.array_equal(m["o_x"], m["x"]) and np.array_equal(m["o_y"], m["y"])  # every two-car KAT is parked
    c = lat.census_multi(lat.multi_kats(), m["o_done_all"], m["o_placement"], m["o_progress"], m["o_crashed"])
    _floors(c, ("half", "near", "along", "corner", "tie"), "two cars")
    _floors(lat.census_ties(m["track"], m["x"], m["y"]), ("tie",), "two cars' ties")


# ------------------------------------------------------------------------------ agreement of the two oracle builds
def test_oracle_builds_agree_on_all_but_one_percent(fix, golden, oracle, oracle_dev):
    """A row is comparable if every mask and `progress` are equal and the floats agree within
    1e-5 between the glibc and the device-libm build (lattice_cases.comparable); the GPU tests hold
    the kernels to the recorded reference outputs on those rows.  Measured: 0 non-comparable rows
    of 4,011 rays, 2,100 single-agent and 2,400 two-car steps."""
    shares = {}
    for name, ok in lat.comparable(fix, golden, oracle, oracle_dev).items():
        shares[name] = float((~ok).mean())
        print(f"\n{name}: {int((~ok).sum())} of {len(ok)} rows not comparable ({100 * shares[name]:.3f} %)")
    assert all(s <= CAP for s in shares.values()), shares


# ------------------------------------------------------------------------------ parked traces
@pytest.mark.parametrize("name", ["parked_single", "parked_multi"])
def test_parked_trace_repeats_step_0(golden, oracle_dev, name):
    case = lat.get(name, golden, oracle_dev)
    tr = case.trace
    assert case.T == lat.PARKED_STEPS >= 20 and case.n >= 100
    assert not tr["done"].any() and not tr["reset"].any()
    assert not (case.final["flags"] & F_CRASHED).any()
    for t in range(1, case.T):
        assert np.array_equal(tr["obs"][t], tr["obs"][0]), t
        assert np.array_equal(tr["info"][t, ..., 1], tr["info"][0, ..., 1]), t  # progress
    for k in ("x", "y", "angle", "vx", "vy"):
        assert np.array_equal(case.final[k], case.state0[k]), k
    # the cars stand on ties, on every slot, lattice and spline lanes mixed inside one wave
    slots = case.slots
    on = slots >= lat.L0
    x, y = case.state0["x"], case.state0["y"]
    c = lat.census_ties(slots[on], x[on].reshape(on.sum(), -1)[:, 0], y[on].reshape(on.sum(), -1)[:, 0])
    print(f"\n{name}: {case.n} envs; " + str(c))
    # (rect60x30 has 16 non-neighbouring tie points on which a car stands free, all near its corners)
    assert all(v["tie"] == v["rows"] >= 20 and v["apart"] >= 3 for v in c.values()), c
    if name == "parked_single":
        assert set(np.unique(slots)) == set(range(lat.L0 + len(lat.NAMES)))
        assert all(len(np.unique(slots[i:i + 64])) >= 3 for i in range(0, case.n - 63, 64))
    # the window centre half a lap away changes nothing: progress after step 0 is the closest waypoint
    tab = lat.table(golden)
    p0 = tr["info"][0, ..., 1].reshape(case.n, -1)
    xs, ys = x.reshape(case.n, -1), y.reshape(case.n, -1)
    for e in range(0, case.n, 7):
        wp = tab.waypoints(int(slots[e]))
        assert p0[e, 0] == lat.closest(wp, xs[e, :1], ys[e, :1])[0] / len(wp), e


# ------------------------------------------------------------------------------ shared host pieces
@pytest.mark.parametrize("G,SG", [(6, 5), (8, 8), (16, 0), (8, 0)])
def test_cull_tables_host_twin_on_the_lattice_table(golden, G, SG):
    a = lat.track_set(golden).arrays()
    t = dict(wp_off=a["wp_off"], wp=a["wp"], seg=a["seg"], meta=a["meta"])
    want, reach = ct.np_tables(t, G, SG)
    ct.check_against(ct.decode(ct.host_build(t, G, SG)), want, reach, f"lattice G={G} SG={SG}")
    tab = lat.table(golden)  # the env's table is the oracle's
    for k in ("wp_off", "wp", "nrm", "seg", "meta"):
        assert np.array_equal(a[k], getattr(tab, k)), k
    for j, rec in enumerate(lat.tracks()):  # and lattice_cases' boxes are the table's
        o, n = want["chunk_off"][lat.L0 + j], want["chunk_off"][lat.L0 + j + 1]
        assert np.array_equal(want["chunk_box"][o:n], lat.chunk_boxes(rec, G))


def test_prefilter_emulation_keeps_every_exact_hit_of_the_ray_kats():
    """The float32 segment pre-filter (seg_may_hit, emulated in tests/test_prefilter_cpu.py) on
    axis rays, on-wall origins and vertex hits: no segment the exact test hits is rejected."""
    rk = lat.ray_kats()
    hits = 0
    for j, rec in enumerate(lat.tracks()):
        m = rk["track"] == lat.L0 + j
        ox, oy, d = (rk[k][m][:, None] for k in ("ox", "oy", "dir"))
        s, v2 = rec["starts"], rec["v2"]
        shape = (int(m.sum()), len(s))
        ox, oy, v3x, v3y = (np.broadcast_to(a, shape).reshape(-1) for a in (ox, oy, -np.sin(d), np.cos(d)))
        sx, sy, v2x, v2y = (np.broadcast_to(a[None, :], shape).reshape(-1) for a in (s[:, 0], s[:, 1], v2[:, 0], v2[:, 1]))
        e = s + v2
        cx, cy = 0.5 * (min(s[:, 0].min(), e[:, 0].min()) + max(s[:, 0].max(), e[:, 0].max())), \
            0.5 * (min(s[:, 1].min(), e[:, 1].min()) + max(s[:, 1].max(), e[:, 1].max()))
        hit = pf.exact_hit(ox, oy, sx, sy, v2x, v2y, v3x, v3y)
        keep = pf.prefilter(ox, oy, sx, sy, v2x, v2y, v3x, v3y, pf._e2(ox, oy, s[:, 0], s[:, 1], v2[:, 0], v2[:, 1], cx, cy))
        assert not (hit & ~keep).any(), rec["label"]
        hits += int(hit.sum())
    assert hits > 10000
