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
import numpy as np
import pytest
import torch

from oracle.orc import F_CP25, F_CP50, F_CP75, F_CRASHED, F_FINISHED, F_HAS_CRASHED
from tests import lattice_cases as lat
from tests.golden_util import multi_state_from, single_state_from
from tests.trace_checks import _acts, _check_end, _check_last_rows, _check_rows, _differs, _per_step, _rows, inject

pytestmark = pytest.mark.gpu

OBS_TOL = lat.OBS_TOL  # north star: float observations / rewards against the reference
STATE_TOL = 1e-9       # f64 state after one step: ulp-level libm differences only (tests/test_env_gpu.py)
SPLIT = dict(wide_n=-1, dyn_lpe=1, split=1, reward_lpe=1, ray_lpr=1)
FLOATS = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering")


@pytest.fixture(scope="module")
def fix(golden):
    return golden["lattice"]


@pytest.fixture(scope="module")
def comparable(fix, golden, oracle, oracle_dev):
    return lat.comparable(fix, golden, oracle, oracle_dev)


def _env(golden, slots, n_agents=1, sched=None, expect=None, **kw):
    from rx.vector_env import RacingVectorEnv
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a HIP device")
    slots = np.asarray(slots, dtype=np.int32)
    cps, ws, ts = lat.env_args(golden, slots)
    v = RacingVectorEnv(cps, ws, n_agents=n_agents, device="cuda", track_set=ts, sched=dict(sched or {}), **kw)
    assert np.array_equal(v.track_of_env, slots)  # the env's slot ids are lattice_cases'
    s = v.schedule()
    for key, val in (expect or {}).items():
        assert s[key] == val, (key, s)
    return v


# =============================================================================== ray KATs
@pytest.fixture(scope="module")
def rays(fix, golden, oracle_dev):
    return dict(kat=lat.ray_kats(), dev=lat.oracle_rays(golden, oracle_dev), t=fix["ray_t"])


def _cast(golden, rays, comparable, sched, expect=None, **kw):
    """step_device(phases=2): the raycast alone from the injected poses."""
    kat = rays["kat"]
    n = len(kat["ox"])
    v = _env(golden, kat["track"], sched=sched, expect=expect, autoreset="disabled", **kw)
    v.set_state(x=kat["ox"], y=kat["oy"], angle=kat["dir"], progress=kat["progress"], last_progress=kat["progress"])
    obs = v.step_device(torch.zeros((n, 2), device="cuda"), phases=2)[0].cpu().numpy()[:, :11]
    v.close()
    _differs([("rays", obs[None], rays["dev"][None])])
    ok = comparable["rays"]
    want = rays["t"].astype(np.float32) / np.float32(50.0)  # sensor 5: relative angle exactly 0
    np.testing.assert_allclose(obs[ok, 5], want[ok], rtol=0, atol=OBS_TOL)
    assert np.array_equal(obs[ok, 5] == 0, rays["t"][ok] == 0)  # a mask of its own: the origin ON a wall


@pytest.mark.parametrize("chunk,sup", [(0, 0), (6, 0), (6, 5), (8, 0), (8, 8), (16, 0), (16, 4)])
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
def _inject(v, st):
    v.set_state(**{k: st[k] for k in FLOATS + ("flags", "steps")})
    if "finished_step" in st:
        v.set_state(finished_step=st["finished_step"])
    v.set_state(env_flags=np.zeros(v.num_envs, np.uint8))


class Columns:
    """KAT columns from arrays (the lane-varying form's mix of two fixtures)."""

    def __init__(self, **cols):
        self.cols = cols

    def __getitem__(self, k):
        return self.cols[k]


def _single_vs_reference(step, ok, g, obs, rew64, rew, term, trunc, info):
    """tests/test_env_gpu.py::test_single_step_vs_golden_and_oracle's reference half on rows `ok`."""
    fl = g["flags"]
    for name, got, want in (("crashed", (fl & F_CRASHED) != 0, step["o_crashed"]),
                            ("finished", (fl & F_FINISHED) != 0, step["o_finished"]),
                            ("terminated", term, step["o_terminated"]), ("truncated", trunc, step["o_truncated"]),
                            ("cp", np.stack([(fl & F_CP25) != 0, (fl & F_CP50) != 0, (fl & F_CP75) != 0], 1),
                             step["o_cp"].astype(bool)),
                            ("steps", g["steps"], step["o_steps"]), ("progress", g["progress"], step["o_progress"])):
        assert np.array_equal(got[ok], want[ok]), name
    for k in ("x", "y", "angle", "vx", "vy"):
        np.testing.assert_allclose(g[k][ok], step["o_" + k][ok], rtol=0, atol=STATE_TOL, err_msg=k)
    np.testing.assert_allclose(obs[ok], step["o_obs"][ok], rtol=0, atol=OBS_TOL)
    np.testing.assert_allclose(rew64[ok], step["o_reward"][ok], rtol=0, atol=OBS_TOL)
    np.testing.assert_allclose(rew[ok], step["o_reward"][ok].astype(np.float32), rtol=0, atol=OBS_TOL)
    np.testing.assert_allclose(info[ok, 0], step["o_info_speed"][ok], atol=1e-9)
    np.testing.assert_allclose(info[ok, 1], step["o_info_progress"][ok], atol=0)
    np.testing.assert_allclose(info[ok, 2], step["o_progress_delta"][ok], atol=1e-12)


def _step_single(golden, oracle_dev, step, ok, sched, expect=None, **kw):
    v = _env(golden, step["track"], sched=sched, expect=expect, autoreset="disabled", **kw)
    _inject(v, single_state_from(step))
    v.set_speed_weights(step["speed_weight"])
    obs, rew, _ = v.step_device(torch.from_numpy(step["action"]).cuda(), full_info=True)
    torch.cuda.synchronize()
    g = v.get_state()
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    rew64 = v.buf["reward64"].cpu().numpy()
    term, trunc = v.buf["terminated"].cpu().numpy(), v.buf["truncated"].cpu().numpy()
    info = v.buf["info"].cpu().numpy()[:, 0]
    v.close()
    st, (o_obs, o_rew, o_term, o_trunc, o_info) = lat.oracle_single(step, lat.table(golden), oracle_dev)
    fields = [("terminated", term, o_term.astype(np.uint8)), ("truncated", trunc, o_trunc.astype(np.uint8)),
              ("reward64", rew64, o_rew), ("info", info[:, :3], o_info), ("obs", obs, o_obs)]
    fields += [("state " + k, g[k], st[k]) for k in ("progress", "flags", "steps", "x", "y", "angle", "vx", "vy",
                                                     "last_progress", "last_steering")]
    _differs([(name, dev[None], ref[None]) for name, dev, ref in fields])
    _single_vs_reference(step, ok, g, obs, rew64, rew, term.astype(bool), trunc.astype(bool), info)


@pytest.fixture(scope="module")
def single(fix):
    return lat.View(fix, "single_")


PATHS = {"default": (dict(wide_n=-1), dict(wide=0)), "split": (SPLIT, dict(split=1, dyn_lpe=1, wide=0)),
         "wide": (dict(wide_n=1000000), dict(wide=1))}


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
TWO = {"one_kernel": (dict(split=-1), {}, dict(split=0)),
       "split_lane_per_env": (dict(split=1, reward_lpe=1), {}, dict(split=1, reward_lpe=1)),
       "split_lane_per_car": (dict(split=1, reward_lpe=2), {}, dict(split=1, reward_lpe=2)),
       "ray_order1": ({}, dict(sort_interval=2, ray_order=1), {}),
       "ray_order2": ({}, dict(sort_interval=2, ray_order=2), {})}


@pytest.mark.parametrize("form", list(TWO))
def test_two_cars(fix, golden, oracle_dev, comparable, form):
    sched, kw, expect = TWO[form]
    step = lat.View(fix, "multi_")
    v = _env(golden, step["track"], n_agents=2, sched=sched, expect=expect, autoreset="disabled", **kw)
    st0 = multi_state_from(step)
    flat = {k: st0[k].reshape(-1) for k in FLOATS + ("flags", "finished_step")}
    flat["steps"] = st0["steps"]
    _inject(v, flat)
    obs, _, _ = v.step_device(torch.from_numpy(step["action"]).cuda(), full_info=True)
    torch.cuda.synchronize()
    g = v.get_state()
    obs = obs.cpu().numpy()
    rew64 = v.buf["reward64"].cpu().numpy()
    term, trunc = v.buf["terminated"].cpu().numpy(), v.buf["truncated"].cpu().numpy()
    info = v.buf["info"].cpu().numpy()
    v.close()
    st, (o_obs, o_rew, o_done, o_all, o_trunc, o_place, o_info) = lat.oracle_multi(step, lat.table(golden), oracle_dev)
    fields = [("terminated", term, o_done.astype(np.uint8)), ("truncated", trunc, o_trunc.astype(np.uint8)),
              ("placement", info[..., 3], o_place.astype(np.float64)), ("reward64", rew64, o_rew),
              ("info", info[..., :2], o_info), ("obs", obs, o_obs), ("state steps", g["steps"], st["steps"])]
    fields += [("state " + k, g[k].reshape(-1, 2), st[k]) for k in ("progress", "flags", "finished_step", "x", "y",
                                                                   "angle", "vx", "vy", "last_progress",
                                                                   "last_steering")]
    _differs([(name, dev[None], ref[None]) for name, dev, ref in fields])
    ok = comparable["multi"]
    fl = g["flags"].reshape(-1, 2)
    term, trunc = term.astype(bool), trunc.astype(bool)
    for name, got, want in (("crashed", (fl & F_CRASHED) != 0, step["o_crashed"]),
                            ("finished", (fl & F_FINISHED) != 0, step["o_finished"]),
                            ("has_crashed", (fl & F_HAS_CRASHED) != 0, step["o_has_crashed"]),
                            ("finished_step", g["finished_step"].reshape(-1, 2), step["o_finished_step"]),
                            ("done", term, step["o_done"]), ("done_all", term | trunc, step["o_done_all"]),
                            ("truncated", trunc, step["o_truncated"]),
                            ("placement", info[..., 3].astype(np.int32), step["o_placement"]),
                            ("progress", g["progress"].reshape(-1, 2), step["o_progress"])):
        assert np.array_equal(got[ok], want[ok]), name
    np.testing.assert_allclose(obs[ok], step["o_obs"][ok], rtol=0, atol=OBS_TOL)
    np.testing.assert_allclose(rew64[ok], step["o_reward"][ok], rtol=0, atol=OBS_TOL)


# =============================================================================== parked traces
@pytest.fixture(scope="module")
def parked(golden, oracle_dev):
    return lat.get("parked_single", golden, oracle_dev)


@pytest.fixture(scope="module")
def parked2(golden, oracle_dev):
    return lat.get("parked_multi", golden, oracle_dev)


def _start(golden, case, sched, expect=None, **kw):
    v = _env(golden, case.slots, n_agents=case.n_agents, sched=sched, expect=expect, autoreset="next_step", **kw)
    if case.n_agents == 2:  # resets take their start side from the reference's stream, as the trace did
        v.use_numpy_start_draws()
        np.random.seed(case.draw_seed)
    v.reset_device()
    inject(v, case)
    return v


def _per_step_form(golden, case, sched, expect=None, **kw):
    v = _start(golden, case, sched, expect, **kw)
    out = _per_step(v, case)
    torch.cuda.synchronize()
    _check_rows(case, out)
    _check_end(case, v)
    v.close()


def _steps_form(golden, case, sched, calls=None, expect=None, **kw):
    v = _start(golden, case, sched, expect, **kw)
    out = _rows(v, case.T)
    lo = 0
    for c in calls or (case.T,):
        sl = slice(lo, lo + c)
        v.steps_device(_acts(case, lo, lo + c), obs_out=out["obs"][sl], reward_out=out["reward"][sl],
                       done_out=out["done"][sl], full_info=True)
        lo += c
    assert lo == case.T
    torch.cuda.synchronize()
    _check_rows(case, out)
    _check_last_rows(case, v)
    _check_end(case, v)
    v.close()


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
