"""Every launch form on the lattice-track cases (DESIGN.md §4 "Lattice tracks";
tests/lattice_cases.py, tests/test_lattice_cpu.py).

Exact closest-waypoint ties, rays along the axes (a sine of exactly 0, |1 / d| ~ 1.6e16), rays
exactly parallel to a wall, origins on walls, vertices and chunk-box planes, t == 0, and for
two cars the 0.5 origin exclusion, rays along an edge and through a corner of the other car
and equal placement scores.  For every form:

* every output and the whole state equal the device-libm oracle BIT FOR BIT (a failure names
  the first env and field that differ);
* on comparable rows (lattice_cases.comparable: the glibc and device-libm oracle builds
  agree) the masks equal the reference's recorded outputs exactly and the floats agree within
  1e-5, as in tests/test_env_gpu.py.

The parked traces (24 steps of v = 0 on tie points; every step repeats step 0) run under
per-step launches, rx_steps in one call and in calls of 5 + 1 + 2 + 16, re-sorts that move the
state rows between steps, lane-varying slots, a captured graph and two cars.
"""
import functools

import numpy as np
import pytest
import torch

from tests import kat_forms as kf
from tests import lattice_cases as lat
from tests.kat_forms import PATHS, SPLIT, TWO, Columns
from tests.trace_checks import _acts, _check_end, _check_last_rows, _check_rows, _rows

pytestmark = pytest.mark.gpu

# the forms both KAT suites share (tests/kat_forms.py), on the lattice slots
_cast = functools.partial(kf.cast, lat)
_step_single = functools.partial(kf.step_single, lat)
_start = functools.partial(kf.start, lat)
_per_step_form = functools.partial(kf.per_step_form, lat)
_steps_form = functools.partial(kf.steps_form, lat)


@pytest.fixture(scope="module")
def fix(golden):
    return golden["lattice"]


@pytest.fixture(scope="module")
def comparable(fix, golden, oracle, oracle_dev):
    return lat.comparable(fix, golden, oracle, oracle_dev)


# =============================================================================== ray KATs
@pytest.fixture(scope="module")
def rays(fix, golden, oracle_dev):
    return dict(kat=lat.ray_kats(), dev=lat.oracle_rays(golden, oracle_dev), t=fix["ray_t"])


@pytest.mark.parametrize("chunk,sup", [(0, 0), (6, 0), (6, 5), (8, 0), (8, 8), (16, 0), (16, 4)])
def test_rays_culling(golden, rays, comparable, chunk, sup):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1), cull_chunk=chunk, cull_super=sup, sort_interval=0)


@pytest.mark.parametrize("lpr", [1, 2, 4])
def test_rays_lanes_per_ray(golden, rays, comparable, lpr):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1, ray_lpr=lpr), dict(ray_lpr=lpr, wide=0))


@pytest.mark.parametrize("key", ["seg_filter", "box_quadrants"])
@pytest.mark.parametrize("val", [-1, 1])
def test_rays_filters(golden, rays, comparable, key, val):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1, ray_lpr=1, **{key: val}), {key: max(val, 0)})


@pytest.mark.parametrize("order", [0, 1, 2])
def test_rays_lane_order(golden, rays, comparable, order):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1), ray_order=order, sort_interval=4)


def test_rays_wide_kernels(golden, rays, comparable):
    _cast(golden, rays, comparable["rays"], dict(wide_n=1000000), dict(wide=1))


def test_rays_tail_split(golden, rays, comparable):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1, ray_lpr=1, ray_tail=3, ray_tail_lpr=2),
          dict(ray_tail=3, ray_tail_lpr=2))


@pytest.mark.parametrize("sup", [0, 8])
def test_rays_lane_varying(golden, rays, comparable, sup):
    _cast(golden, rays, comparable["rays"], dict(wide_n=-1, lane_tracks=1), dict(lane_tracks=1), cull_super=sup)


# =============================================================================== single-agent step KATs
@pytest.fixture(scope="module")
def single(fix):
    return lat.View(fix, "single_")


@pytest.mark.parametrize("path", list(PATHS))
def test_single_dynamics_paths(golden, oracle_dev, single, comparable, path):
    sched, expect = PATHS[path]
    _step_single(golden, oracle_dev, single, comparable["single"], sched, expect)


@pytest.mark.parametrize("lpe", [1, 2, 4])
def test_single_reward_lanes_per_env(golden, oracle_dev, single, comparable, lpe):
    _step_single(golden, oracle_dev, single, comparable["single"], dict(SPLIT, reward_lpe=lpe),
                 dict(split=1, reward_lpe=lpe))


@pytest.mark.parametrize("window", [-1, 1, 2, 32])
def test_single_argmin_window(golden, oracle_dev, single, comparable, window):
    """Half the KATs' `progress` -- the centre of the window -- is half a lap from the answer."""
    _step_single(golden, oracle_dev, single, comparable["single"], dict(SPLIT, argmin_window=window),
                 dict(split=1, argmin_window=max(window, 0)))


def test_single_brute_force_raycast(golden, oracle_dev, single, comparable):
    _step_single(golden, oracle_dev, single, comparable["single"], SPLIT, dict(split=1), cull_chunk=0, sort_interval=0)


@pytest.mark.parametrize("sup", [0, 8])
def test_single_lane_varying(golden, oracle_dev, single, comparable, sup):
    """lane_tracks = 1 on 3,500 envs: the lattice KATs and step_single.npz's rows of the two spline
    slots, permuted so that the 64 lanes of a wave stand on all five tracks; cull_super 8 runs the leaf
    batch path's super boxes, 0 the plain leaf loop."""
    gs = golden["step_single"]
    cols = [k for k in lat.SINGLE_COLS if k != "track"] + [k for k in gs.files if k.startswith("o_")]
    pick = np.concatenate([np.flatnonzero(gs["track"] == t) for t in lat.GOLDEN_SLOTS])
    slot = np.concatenate([np.full(int((gs["track"] == t).sum()), j) for j, t in enumerate(lat.GOLDEN_SLOTS)])
    perm = np.random.default_rng(5).permutation(len(pick) + len(single["x"]))
    step = Columns(track=np.concatenate([slot, single["track"]])[perm],
                   **{k: np.concatenate([gs[k][pick], single[k]])[perm] for k in cols})
    ok = np.concatenate([np.ones(len(pick), bool), comparable["single"]])[perm]  # the spline rows: all, as test_env_gpu
    n = len(perm)
    assert n > 2048 and all(len(np.unique(step["track"][i:i + 64])) == 5 for i in range(0, n - 63, 64))
    _step_single(golden, oracle_dev, step, ok, dict(SPLIT, lane_tracks=1), dict(split=1, lane_tracks=1), cull_super=sup)


# =============================================================================== two-car step KATs
@pytest.mark.parametrize("form", list(TWO))
def test_two_cars(fix, golden, oracle_dev, comparable, form):
    sched, kw, expect = TWO[form]
    kf.step_two(lat, golden, oracle_dev, lat.View(fix, "multi_"), comparable["multi"], sched, kw, expect)


# =============================================================================== parked traces
@pytest.fixture(scope="module")
def parked(golden, oracle_dev):
    return lat.get("parked_single", golden, oracle_dev)


@pytest.fixture(scope="module")
def parked2(golden, oracle_dev):
    return lat.get("parked_multi", golden, oracle_dev)


@pytest.mark.parametrize("sort_interval", [0, 3, 8])
def test_parked_per_step(golden, parked, sort_interval):
    """The cars stand all round the tracks, so every re-sort moves state rows between steps."""
    _per_step_form(golden, parked, SPLIT, dict(split=1), sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 3, 8])
def test_parked_steps_one_call(golden, parked, sort_interval):
    """24 steps in one rx_steps call: the deep launch schedule (calls under 20 steps keep the paired one)."""
    _steps_form(golden, parked, SPLIT, expect=dict(split=1, reward_lpe=1), sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 8])
def test_parked_steps_in_calls_of_5_1_2_16(golden, parked, sort_interval):
    _steps_form(golden, parked, SPLIT, calls=(5, 1, 2, 16), sort_interval=sort_interval)


@pytest.mark.parametrize("form", ["per_step", "steps"])
def test_parked_lane_varying(golden, parked, form):
    sched, expect = dict(SPLIT, lane_tracks=1), dict(split=1, lane_tracks=1)
    if form == "per_step":
        _per_step_form(golden, parked, sched, expect)
    else:
        _steps_form(golden, parked, sched, expect=expect)


def test_parked_captured_graph_replay(golden, parked):
    """One replay of a graph captured over steps_device(24) from the injected state."""
    v = _start(golden, parked, SPLIT, sort_interval=8)
    acts = _acts(parked)
    out = _rows(v, parked.T)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap, capture_error_mode="thread_local"):
        v.steps_device(acts, obs_out=out["obs"], reward_out=out["reward"], done_out=out["done"], full_info=True)
    graph.replay()
    torch.cuda.synchronize()
    _check_rows(parked, out)
    _check_last_rows(parked, v)
    _check_end(parked, v)
    del graph
    v.close()


@pytest.mark.parametrize("form", ["one_kernel", "split_lane_per_car", "steps"])
def test_parked_two_cars(golden, parked2, form):
    if form == "steps":
        _steps_form(golden, parked2, {}, sort_interval=3)
    else:
        sched, kw, expect = TWO[form]
        _per_step_form(golden, parked2, sched, expect, **kw)
