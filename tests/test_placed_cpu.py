"""Placed-track cases on the CPU (DESIGN.md §4 "Placed tracks"; tests/placed_cases.py).

tests/golden/placed.npz holds what the reference answered to the pinned rows of the KATs on its
own Track with gen_waypoints overridden.  Here: the committed inputs are what placed_cases builds
today; the glibc oracle reproduces every recorded output bit for bit; the census stays above its
floors (a slot whose rays all miss tests nothing); the device-libm oracle build -- the checker
of the GPU tests -- agrees with the glibc build on all but at most 1 % of the pinned rows; the
host twin of the culling tables and the float32 segment pre-filter's emulation are exact on
these tables; the trace drives, crashes and resets.
"""
import numpy as np
import pytest

from tests import lattice_cases as lat
from tests import placed_cases as pc
from tests import test_cull_tables_cpu as ct
from tests import test_oracle_golden as og
from tests import test_prefilter_cpu as pf

CAP = 0.01
IN_RANGE_SHARE, WINDOW_MISSES, PER_KIND = 0.40, 20, 10


@pytest.fixture(scope="module")
def fix(golden):
    return golden["placed"]


def test_slots(golden):
    recs = pc.slot_records(golden)
    assert len(recs) == pc.N_SLOTS == len(pc.labels()) == 17
    for b, k in enumerate(pc.BASES):
        for m, (s, c) in enumerate(pc.MAPS):
            r = recs[pc.slot_of(b, m)]
            assert np.array_equal(r["wp"], golden.tracks[k]["wp"] * s + np.array(c)) and r["width"] == golden.tracks[k]["width"] * s
            assert pc.slot_map(pc.slot_of(b, m)) == (s, c)
    # the magnitudes the slots exist for
    L = [np.hypot(r["v2"][:, 0], r["v2"][:, 1]).max() for r in recs]
    assert max(L) > 90.0 and min(L) < 0.1, (max(L), min(L))
    assert max(np.abs(r["wp"]).max() for r in recs) > 2.0 ** 26
    assert all(recs[pc.slot_of(b, 4)]["width"] < 1.0 for b in range(2))  # the 4 x 2 car is wider than the track
    assert len({len(r["wp"]) for r in recs}) >= 3 and any(len(r["wp"]) % 8 for r in recs)


def test_fixture_inputs_are_the_cases(fix, golden):
    """The committed inputs are the pinned rows of what tests/placed_cases.py builds today."""
    for name, cols in (("ray", ("track", "ox", "oy", "dir", "progress", "okind", "dkind")),
                       ("single", pc.SINGLE_COLS), ("multi", pc.MULTI_COLS + ("kind",))):
        idx, kat = pc.pinned(golden, name)
        assert np.array_equal(fix[name + "_idx"], idx)
        for k in cols:
            assert np.array_equal(fix[f"{name}_{k}"], kat[k]), (name, k)
    for kat, per in ((pc.ray_kats(golden), 296), (pc.single_kats(golden), 150)):
        assert np.array_equal(np.bincount(kat["track"]), np.full(pc.N_SLOTS, per))
        assert len(kat["track"]) <= 8000
    assert set(pc.multi_kats(golden)["track"]) == set(pc.MULTI_SLOTS)


def test_rays_bit_exact(fix, golden, oracle):
    tab = pc.table(golden)
    rc = lat.View(fix, "ray_")
    got = np.array([oracle.raycast(tab.segments(int(k)), ox, oy, d)
                    for k, ox, oy, d in zip(rc["track"], rc["ox"], rc["oy"], rc["dir"])])
    assert np.array_equal(got, rc["t"])
    recs = pc.slot_records(golden)
    for k in range(pc.N_SLOTS):  # the census' own restatement
        m = rc["track"] == k
        t = pc.ray_t(recs[k], rc["ox"][m], rc["oy"][m], rc["dir"][m])
        assert np.array_equal(np.where(np.isfinite(t), t, 50.0), rc["t"][m]), k


def test_single_steps_bit_exact(fix, golden, oracle):
    step = lat.View(fix, "single_")
    st, out = lat.oracle_single(step, pc.table(golden), oracle)
    og._check_single(step, st, *out, exact=True)


def test_multi_steps_bit_exact(fix, golden, oracle):
    step = lat.View(fix, "multi_")
    st, out = lat.oracle_multi(step, pc.table(golden), oracle)
    og._check_multi(step, st, *out, exact=True)


def test_census_floors(golden, oracle_dev):
    c = pc.census(golden, oracle_dev)
    for name, v in c.items():
        print(f"\n{name}: " + ", ".join(f"{k} {n}" for k, n in v.items()))
    for k, (name, v) in enumerate(c.items()):
        if pc.slot_map(k)[0] >= 1.0:
            assert v["in_range"] >= IN_RANGE_SHARE * v["rays"], (name, v)
        assert v["in_range"] > 0 and v["no_hit"] >= PER_KIND and v["plane"] >= PER_KIND, (name, v)
        assert v["window_miss"] >= WINDOW_MISSES, (name, v)
        for kind in [f"o_{o}" for o in pc.OKINDS] + [f"d_{d}" for d in pc.DKINDS]:
            assert v[kind] >= PER_KIND, (name, kind, v[kind])
        assert v["crash"] >= 5, (name, v)
    # two cars: the 0.5 exclusion, edges and corners of the other car survive the move
    mk = pc.multi_kats(golden)
    d = np.hypot(mk["x"][:, 0] - mk["x"][:, 1], mk["y"][:, 0] - mk["y"][:, 1])
    for k in pc.MULTI_SLOTS:
        m = mk["track"] == k
        assert (d[m] == 0.5).sum() >= 50 and (d[m] < 0.5).sum() >= 50, k


def test_oracle_builds_agree_on_all_but_one_percent(fix, golden, oracle, oracle_dev):
    """lattice_cases.comparable's rule on the pinned rows.  Measured: 0 non-comparable rows of 2,550
    rays, 1,020 single-agent and 300 two-car steps."""
    shares = {}
    for name, ok in pc.comparable(fix, golden, oracle, oracle_dev).items():
        shares[name] = float((~ok).mean())
        print(f"\n{name}: {int((~ok).sum())} of {len(ok)} rows not comparable ({100 * shares[name]:.3f} %)")
    assert all(s <= CAP for s in shares.values()), shares


def test_trace_drives_crashes_and_resets(golden, oracle_dev):
    case = pc.get("trace", golden, oracle_dev)
    tr = case.trace
    assert case.T == pc.TRACE_STEPS >= 20 and case.n >= 128
    assert set(np.unique(case.slots)) == set(pc.TRACE_SLOTS)
    assert tr["done"].sum() >= 20 and tr["reset"].sum() >= 20 and case.events["crash"].sum() >= 10
    moved = np.hypot(case.final["x"] - case.state0["x"], case.final["y"] - case.state0["y"])
    assert np.median(moved) > 5.0
    assert np.abs(case.final["x"]).min() > 2.0 ** 19  # nobody left the placed slots


@pytest.mark.parametrize("G,SG", [(6, 5), (8, 8), (16, 4), (8, 0)])
def test_cull_tables_host_twin_on_the_placed_table(golden, G, SG):
    a = pc.track_set(golden).arrays()
    t = dict(wp_off=a["wp_off"], wp=a["wp"], seg=a["seg"], meta=a["meta"])
    want, reach = ct.np_tables(t, G, SG)
    ct.check_against(ct.decode(ct.host_build(t, G, SG)), want, reach, f"placed G={G} SG={SG}")
    tab = pc.table(golden)  # the env's table is the oracle's
    for k in ("wp_off", "wp", "nrm", "seg", "meta"):
        assert np.array_equal(a[k], getattr(tab, k)), k
    for k, rec in enumerate(pc.slot_records(golden)):  # and the KATs' boxes are the table's
        o, n = want["chunk_off"][k], want["chunk_off"][k + 1]
        assert np.array_equal(want["chunk_box"][o:n], lat.chunk_boxes(rec, G)), k


def test_prefilter_emulation_keeps_every_exact_hit_of_the_ray_kats(golden):
    """The float32 segment pre-filter (seg_may_hit, tests/test_prefilter_cpu.py) with the kernel's
    threshold e2 = 2^-17 (|ox| + |oy| + |cx| + |cy| + 2 rad + L + 1) at every slot's magnitudes."""
    rk = pc.ray_kats(golden)
    hits = 0
    for k, rec in enumerate(pc.slot_records(golden)):
        m = rk["track"] == k
        ox, oy, d = (rk[c][m][:, None] for c in ("ox", "oy", "dir"))
        s, v2 = rec["starts"], rec["v2"]
        shape = (int(m.sum()), len(s))
        ox, oy, v3x, v3y = (np.broadcast_to(a, shape).reshape(-1) for a in (ox, oy, -np.sin(d), np.cos(d)))
        sx, sy, v2x, v2y = (np.broadcast_to(a[None, :], shape).reshape(-1) for a in (s[:, 0], s[:, 1], v2[:, 0], v2[:, 1]))
        cx, cy, _ = pc.circle(rec)
        hit = pf.exact_hit(ox, oy, sx, sy, v2x, v2y, v3x, v3y)
        keep = pf.prefilter(ox, oy, sx, sy, v2x, v2y, v3x, v3y, pf._e2(ox, oy, s[:, 0], s[:, 1], v2[:, 0], v2[:, 1], cx, cy))
        assert not (hit & ~keep).any(), pc.labels()[k]
        hits += int(hit.sum())
    assert hits > 5000


def test_box_test_emulation_keeps_the_chunk_of_every_exact_hit(golden):
    """The float32 box test (tests/test_slab_cpu.py's emulation of chunk_needed_f / _q) on the ray
    KATs against the slots' own chunk boxes (G = 6, 8, 16) and geo rows: the leaf box of every
    segment the exact test hits is kept under every bound above the hit's t."""
    from tests import test_slab_cpu as sl
    rk = pc.ray_kats(golden)
    required = 0
    for k, rec in enumerate(pc.slot_records(golden)):
        m = rk["track"] == k
        s, v2 = rec["starts"], rec["v2"]
        W = len(rec["wp"])
        n_r, n_s = int(m.sum()), len(s)
        ray, seg = (a.reshape(-1) for a in np.meshgrid(np.arange(n_r), np.arange(n_s), indexing="ij"))
        cx, cy, rad = pc.circle(rec)
        d = rk["dir"][m][ray]
        full = dict(ox=rk["ox"][m][ray], oy=rk["oy"][m][ray], cs=np.cos(d), sn=np.sin(d), sx=s[seg, 0], sy=s[seg, 1],
                    v2x=v2[seg, 0], v2y=v2[seg, 1])
        hit, t = sl.exact(full)
        r = {c: v[hit] for c, v in full.items()}
        n = int(hit.sum())
        r.update(cx=np.full(n, cx), cy=np.full(n, cy), rad=np.full(n, rad * (1.0 + 1e-12) + 1e-9),
                 L=np.full(n, np.hypot(v2[:, 0], v2[:, 1]).max() * (1.0 + 1e-12) + 1e-12))
        seg, t = seg[hit], t[hit]
        side, j = seg // W, seg % W
        for G in pc.CULL_G:
            b = lat.chunk_boxes(rec, G)[side * (-(-W // G)) + j // G]
            n_lost, n_req = sl.lost(r, np.ones(n, bool), t, b, b)
            assert n_lost == 0, (pc.labels()[k], G, n_lost)
            required += n_req
    assert required > 500_000
