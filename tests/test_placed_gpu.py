"""Every launch form on the placed-track cases (DESIGN.md §4 "Placed tracks";
tests/placed_cases.py, tests/test_placed_cpu.py, tests/test_slab_cpu.py).

The two golden spline tracks moved to (1e3, -1e3), (2^17, 2^17), (-2^20, 3 2^18) and (2^26, -2^26)
and scaled by 1/16, 16 and 64: the coordinate and length terms of every culling margin (mb, mt,
mbf, e2, the slab slack, the waypoint boxes' bound) at magnitudes no other test reaches.  All 17
slots stand in one env.  For every form:

* every output and the whole state equal the device-libm oracle BIT FOR BIT on every row;
* on the comparable ones of the rows tests/golden/placed.npz pins (lattice_cases.comparable's
  rule) the masks equal the reference's recorded outputs exactly and the floats agree within
  OBS_TOL / STATE_TOL, as in tests/test_lattice_gpu.py.

Not vacuous: with the culling counters on, every slot with |c| <= 2^20 and s <= 16 scans strictly
fewer leaves and waypoint chunks than the brute-force counts (one lane per ray / per env, so
the counters count per ray / per env).  At 2^26 and s = 64 the margins may keep nearly
everything; that is correct behaviour and only printed (`pytest -s`; DESIGN.md §4 has the table).
"""
import numpy as np
import pytest

from tests import kat_forms as kf
from tests import lattice_cases as lat
from tests import placed_cases as pc
from tests.kat_forms import PATHS, SPLIT, TWO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix(golden):
    return golden["placed"]


@pytest.fixture(scope="module")
def comparable(fix, golden, oracle, oracle_dev):
    return pc.comparable(fix, golden, oracle, oracle_dev)


# =============================================================================== ray KATs
@pytest.fixture(scope="module")
def rays(fix, golden, oracle_dev):
    return dict(kat=pc.ray_kats(golden), dev=pc.oracle_rays(golden, oracle_dev), t=fix["ray_t"], idx=fix["ray_idx"])


def _cast(golden, rays, comparable, sched, expect=None, **kw):
    kf.cast(pc, golden, rays, comparable["rays"], sched, expect, **kw)


@pytest.mark.parametrize("chunk,sup", [(0, 0), (6, 5), (8, 0), (8, 8), (16, 4)])
def test_rays_culling(golden, rays, comparable, chunk, sup):
    _cast(golden, rays, comparable, dict(wide_n=-1), cull_chunk=chunk, cull_super=sup, sort_interval=0)


@pytest.mark.parametrize("lpr", [1, 2, 4])
def test_rays_lanes_per_ray(golden, rays, comparable, lpr):
    _cast(golden, rays, comparable, dict(wide_n=-1, ray_lpr=lpr), dict(ray_lpr=lpr, wide=0))


@pytest.mark.parametrize("key", ["seg_filter", "box_quadrants"])
@pytest.mark.parametrize("val", [-1, 1])
def test_rays_filters(golden, rays, comparable, key, val):
    _cast(golden, rays, comparable, dict(wide_n=-1, ray_lpr=1, **{key: val}), {key: max(val, 0)})


@pytest.mark.parametrize("order", [0, 1, 2])
def test_rays_lane_order(golden, rays, comparable, order):
    _cast(golden, rays, comparable, dict(wide_n=-1), ray_order=order, sort_interval=4)


def test_rays_wide_kernels(golden, rays, comparable):
    _cast(golden, rays, comparable, dict(wide_n=1000000), dict(wide=1))


def test_rays_tail_split(golden, rays, comparable):
    _cast(golden, rays, comparable, dict(wide_n=-1, ray_lpr=1, ray_tail=3, ray_tail_lpr=2),
          dict(ray_tail=3, ray_tail_lpr=2))


@pytest.mark.parametrize("sup", [0, 8])
def test_rays_lane_varying(golden, rays, comparable, sup):
    _cast(golden, rays, comparable, dict(wide_n=-1, lane_tracks=1), dict(lane_tracks=1), cull_super=sup)


# =============================================================================== single-agent step KATs
@pytest.fixture(scope="module")
def single(fix, golden):
    return dict(ref=lat.View(fix, "single_"), idx=fix["single_idx"])


def _step_single(golden, oracle_dev, single, comparable, sched, expect=None, **kw):
    kf.step_single(pc, golden, oracle_dev, pc.single_kats(golden), comparable["single"], sched, expect,
                   ref=single["ref"], idx=single["idx"], **kw)


@pytest.mark.parametrize("path", list(PATHS))
def test_single_dynamics_paths(golden, oracle_dev, single, comparable, path):
    sched, expect = PATHS[path]
    _step_single(golden, oracle_dev, single, comparable, sched, expect)


@pytest.mark.parametrize("lpe", [1, 2, 4])
def test_single_reward_lanes_per_env(golden, oracle_dev, single, comparable, lpe):
    _step_single(golden, oracle_dev, single, comparable, dict(SPLIT, reward_lpe=lpe), dict(split=1, reward_lpe=lpe))


@pytest.mark.parametrize("window", [-1, 1, 2, 32])
def test_single_argmin_window(golden, oracle_dev, single, comparable, window):
    """Half the KATs' `progress` -- the centre of the window -- is half a lap from the answer."""
    _step_single(golden, oracle_dev, single, comparable, dict(SPLIT, argmin_window=window),
                 dict(split=1, argmin_window=max(window, 0)))


def _permuted(kat, idx, seed):
    """The KAT rows in a random order, and where the rows `idx` went."""
    n = len(kat["track"])
    perm = np.random.default_rng(seed).permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return {k: np.ascontiguousarray(v[perm]) for k, v in kat.items()}, inv[idx]


@pytest.mark.parametrize("sup", [0, 8])
def test_single_lane_varying(golden, oracle_dev, single, comparable, sup):
    """lane_tracks = 1 with the rows permuted: the 64 lanes of a wave stand on at least 5 slots."""
    step, idx = _permuted(pc.single_kats(golden), single["idx"], 5)
    n = len(step["track"])
    assert n > 2048 and all(len(np.unique(step["track"][i:i + 64])) >= 5 for i in range(0, n - 63, 64))
    kf.step_single(pc, golden, oracle_dev, step, comparable["single"], dict(SPLIT, lane_tracks=1),
                   dict(split=1, lane_tracks=1), ref=single["ref"], idx=idx, cull_super=sup)


# =============================================================================== two-car step KATs
TWO_PLACED = dict({k: TWO[k] for k in ("one_kernel", "split_lane_per_car", "ray_order2")},
                  lane_cars=(dict(lane_tracks=1, split=1, reward_lpe=1, ray_lpr=1), dict(lane_cars=1),
                             dict(lane_tracks=1, split=1)))


@pytest.mark.parametrize("form", list(TWO_PLACED))
def test_two_cars(fix, golden, oracle_dev, comparable, form):
    sched, kw, expect = TWO_PLACED[form]
    step, idx = pc.multi_kats(golden), fix["multi_idx"]
    if form == "lane_cars":  # both slots inside every wave
        step, idx = _permuted(step, idx, 6)
        assert all(len(np.unique(step["track"][i:i + 64])) == 2 for i in range(0, len(step["track"]) - 63, 64))
    kf.step_two(pc, golden, oracle_dev, step, comparable["multi"], sched, kw, expect, ref=lat.View(fix, "multi_"), idx=idx)


# =============================================================================== the trace
@pytest.fixture(scope="module")
def trace(golden, oracle_dev):
    return pc.get("trace", golden, oracle_dev)


@pytest.mark.parametrize("sort_interval", [0, 3])
def test_trace_per_step(golden, trace, sort_interval):
    kf.per_step_form(pc, golden, trace, SPLIT, dict(split=1), sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 3])
def test_trace_steps_one_call(golden, trace, sort_interval):
    """24 steps in one rx_steps call: the deep launch schedule and its re-sorts."""
    kf.steps_form(pc, golden, trace, SPLIT, expect=dict(split=1, reward_lpe=1), sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 3])
def test_trace_steps_in_calls_of_5_1_2_16(golden, trace, sort_interval):
    kf.steps_form(pc, golden, trace, SPLIT, calls=(5, 1, 2, 16), sort_interval=sort_interval)


# =============================================================================== not vacuous
def _asserted(k):
    s, c = pc.slot_map(k)
    return max(abs(c[0]), abs(c[1])) <= 2.0 ** 20 and s <= 16.0


def _rows_of(kat, k):
    m = kat["track"] == k
    return {c: np.ascontiguousarray(v[m]) for c, v in kat.items()}, m


def test_culled_raycast_scans_fewer_leaves_than_brute_force(golden, rays, comparable):
    """Per slot, G = 8, one lane per ray with its own counters (lane_tracks = 1): leaves scanned
    against rays x 11 sensors x 2 ceil(W / 8)."""
    recs = pc.slot_records(golden)
    pinned = np.zeros(len(rays["kat"]["track"]), bool)
    pinned[rays["idx"]] = True
    for k, name in enumerate(pc.labels()):
        kat, m = _rows_of(rays["kat"], k)
        sub = dict(kat=kat, dev=rays["dev"][m], t=rays["t"][m[rays["idx"]]], idx=np.flatnonzero(pinned[m]))
        c = {}
        kf.cast(pc, golden, sub, comparable["rays"][m[rays["idx"]]], dict(SPLIT, lane_tracks=1),
                dict(lane_tracks=1, ray_lpr=1), counters=c, cull_chunk=8, cull_super=0, sort_interval=0)
        brute = int(m.sum()) * 11 * 2 * -(-len(recs[k]["wp"]) // 8)
        print(f"\n{name}: leaves tested {c['ray_chunk_tests']}, scanned {c['ray_chunks_scanned']} of {brute} "
              f"({c['ray_chunks_scanned'] / brute:.4f})")
        assert c["ray_chunk_tests"] > 0, (name, c)
        if _asserted(k):
            assert 0 < c["ray_chunks_scanned"] < brute, (name, c, brute)


def test_culled_argmin_scans_fewer_chunks_than_brute_force(fix, golden, oracle_dev, single, comparable):
    """Per slot, one lane per env: waypoint chunks scanned against steps x ceil(W / 8)."""
    recs = pc.slot_records(golden)
    full = pc.single_kats(golden)
    pinned = np.zeros(len(full["track"]), bool)
    pinned[single["idx"]] = True
    for k, name in enumerate(pc.labels()):
        step, m = _rows_of(full, k)
        sel = m[single["idx"]]  # the pinned rows of this slot
        ref = kf.Columns(**{c[len("single_"):]: fix[c][sel] for c in fix.files if c.startswith("single_o_")})
        c = {}
        kf.step_single(pc, golden, oracle_dev, step, comparable["single"][sel], dict(SPLIT, lane_tracks=1),
                       dict(split=1, lane_tracks=1), ref=ref, idx=np.flatnonzero(pinned[m]), counters=c)
        brute = int(m.sum()) * -(-len(recs[k]["wp"]) // 8)
        print(f"\n{name}: waypoint boxes tested {c['wp_chunk_tests']}, chunks scanned {c['wp_chunks_scanned']} of {brute} "
              f"({c['wp_chunks_scanned'] / brute:.4f})")
        if _asserted(k):
            assert 0 < c["wp_chunks_scanned"] < brute, (name, c, brute)
