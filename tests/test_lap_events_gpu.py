"""Every step schedule against ONE oracle trace full of lap events (DESIGN.md §4 "Lap
events under every schedule").

tests/lap_cases.py places cars all round the lap, a few waypoints before a checkpoint or
the line and a few steps before the step limit, and the device-libm oracle steps them
under a scripted controller: checkpoints, finishes, refused finishes, truncations, both
progress wraps, the speed cap, crashes, and -- for two cars -- a frozen crashed car beside
a racing one, contact, finished_step and both kinds of placement, with the autoreset that
follows each ending, on every step index of the 64.  The env is reset, the case's state is
injected, and each launch form runs the same 64 steps: every step's obs / reward / done
(with full_info also reward64, terminated, truncated and the info rows), the whole state
after the last step and the episode counts and lengths must equal the trace BIT FOR BIT.
The sum of the episode returns is compared to 1e-9 relative: a re-sort orders the envs of
one bin by the arrival of the REWARD waves' atomics, so the f64 partial sums are taken over
other env sets (tests/test_steps_cross_gpu.py RET_REL).  A failure names the first step, env
and field that differ.
"""
import numpy as np
import pytest
import torch

from tests import lap_cases as lc
from tests.trace_checks import _acts, _check_end, _check_last_rows, _check_rows, _differs, _per_step, _rows, inject

pytestmark = pytest.mark.gpu

SPLIT = dict(wide_n=-1, dyn_lpe=1, split=1, reward_lpe=1, ray_lpr=1)


@pytest.fixture(scope="module")
def single(golden, oracle_dev):
    return lc.get("single", golden, oracle_dev)


@pytest.fixture(scope="module")
def lane(golden, oracle_dev):
    return lc.get("lane", golden, oracle_dev)


@pytest.fixture(scope="module")
def multi(golden, oracle_dev):
    return lc.get("multi", golden, oracle_dev)


def _start(golden, case, sched, **kw):
    """The env on the case's slots, reset, with the case's state injected."""
    from rx.track import DEFAULT_CONTROL_POINTS
    from rx.vector_env import RacingVectorEnv
    cps = [golden.tracks[k]["cp"] if golden.tracks[k]["label"] != "default" else DEFAULT_CONTROL_POINTS
           for k in case.slots]
    ws = [golden.tracks[k]["width"] for k in case.slots]
    v = RacingVectorEnv(cps, ws, n_agents=case.n_agents, device="cuda", autoreset="next_step", sched=dict(sched), **kw)
    if case.n_agents == 2:  # resets take their start side from the reference's stream, as the trace did
        v.use_numpy_start_draws()
        np.random.seed(case.draw_seed)
    v.reset_device()
    # the env's slot ids are its TrackSet's (golden tracks with equal control points and width share
    # one): envs of one slot must stand on one golden geometry
    tab, dev = golden.table(), v.get_state()["track"]
    for k in np.unique(dev):
        gs = np.unique(case.slots[dev == k])
        assert all(np.array_equal(tab.waypoints(gs[0]), tab.waypoints(j)) and tab.meta[gs[0], 3] == tab.meta[j, 3]
                   for j in gs[1:]), (k, gs)
    inject(v, case)
    return v


def _census(case, out, label):
    """The device's own masks give the census of the CPU trace."""
    masks = lc.single_masks if case.n_agents == 1 else lc.multi_masks
    want = masks(case.trace["terminated"], case.trace["truncated"], case.trace["info"])
    if "info" in out:
        info = out["info"].cpu().numpy()
        got = masks(out["terminated"].cpu().numpy() != 0, out["truncated"].cpu().numpy() != 0,
                    info[:, :, 0, :] if case.n_agents == 1 else info)
    else:  # steps_device: the per-step rows are obs / reward / done
        want = dict(done=case.trace["done"].sum(1).astype(int))
        got = dict(done=(out["done"].cpu().numpy() != 0).sum(1).astype(int))
    print(f"\n{label}: device census " + ", ".join(f"{k} {int(v.sum())}" for k, v in got.items())
          + " | oracle events (even/odd): " + lc.census_text(case.events))
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())


def _step_form(golden, case, sched, label, expect=None, **kw):
    v = _start(golden, case, sched, **kw)
    s = v.schedule()
    for key, val in (expect or {}).items():
        assert s[key] == val, (key, s)
    out = _per_step(v, case)
    torch.cuda.synchronize()
    _check_rows(case, out)
    _check_end(case, v)
    _census(case, out, label)
    v.close()


# =============================================================================== single agent, step_device
PATHS = {"default": (dict(wide_n=-1), dict(wide=0)), "split": (SPLIT, dict(split=1, dyn_lpe=1, wide=0)),
         "wide": (dict(wide_n=1000000), dict(wide=1))}


@pytest.mark.parametrize("path", list(PATHS))
def test_dynamics_paths(golden, single, path):
    sched, expect = PATHS[path]
    _step_form(golden, single, sched, f"path {path}", expect)


@pytest.mark.parametrize("lpe", [1, 2, 4])
def test_reward_lanes_per_env(golden, single, lpe):
    _step_form(golden, single, dict(SPLIT, reward_lpe=lpe), f"reward_lpe {lpe}", dict(split=1, reward_lpe=lpe))


@pytest.mark.parametrize("lpr", [1, 2, 4])
def test_lanes_per_ray(golden, single, lpr):
    _step_form(golden, single, dict(SPLIT, ray_lpr=lpr), f"ray_lpr {lpr}", dict(split=1, ray_lpr=lpr))


@pytest.mark.parametrize("window", [-1, 1, 2, 32])
def test_argmin_window(golden, single, window):
    """The closest-waypoint scan around the previous waypoint: off, 1, 2 (the default) and 32, with
    cars whose window wraps at W - 1 -> 0 and cars that moved backwards across the line."""
    _step_form(golden, single, dict(SPLIT, argmin_window=window), f"argmin_window {window}",
               dict(split=1, argmin_window=max(window, 0)))


@pytest.mark.parametrize("key", ["seg_filter", "box_quadrants"])
@pytest.mark.parametrize("val", [-1, 1])
def test_ray_filters(golden, single, key, val):
    _step_form(golden, single, dict(SPLIT, **{key: val}), f"{key} {val}", {"split": 1, key: max(val, 0)})


@pytest.mark.parametrize("chunk,sort,order,sup", [(16, 1, 0, 0), (8, 3, 0, 0), (32, 0, 0, 0), (16, 4, 1, 0),
                                                  (16, 0, 1, 0), (8, 16, 1, 8), (6, 0, 0, 5), (24, 16, 1, 3),
                                                  (12, 16, 2, 6), (16, 3, 2, 0), (12, 0, 2, 6)])
def test_culling_and_sort(golden, single, chunk, sort, order, sup):
    """The cull visit starts wherever each car stands: a wave's cars are spread over the lap."""
    _step_form(golden, single, SPLIT, f"cull_chunk {chunk} sort {sort} ray_order {order} cull_super {sup}",
               dict(split=1), cull_chunk=chunk, sort_interval=sort, ray_order=order, cull_super=sup)


def test_brute_force_raycast(golden, single):
    _step_form(golden, single, SPLIT, "cull_chunk 0", dict(split=1), cull_chunk=0, sort_interval=0)


@pytest.mark.parametrize("interval", [1, 7])
def test_task_sort(golden, single, interval):
    _step_form(golden, single, dict(SPLIT, task_sort=interval), f"task_sort {interval}",
               dict(split=1, task_sort=interval))


@pytest.mark.parametrize("tail,tail_lpr,dispatch", [(3, 2, 0), (11, 4, 0), (5, 2, 1), (2, 4, 2)])
def test_ray_tail_split(golden, single, tail, tail_lpr, dispatch):
    sched = dict(SPLIT, ray_tail=tail, ray_tail_lpr=tail_lpr, ray_dispatch=dispatch)
    _step_form(golden, single, sched, f"ray_tail {tail} x {tail_lpr} dispatch {dispatch}",
               dict(split=1, ray_tail=tail, ray_tail_lpr=tail_lpr))


@pytest.mark.parametrize("sort_interval", [1, 3, 8])
def test_resort_moves_rows(golden, single, sort_interval):
    """The cars stand all round the lap, so the FIRST re-sort already moves rows (from a reset
    every car of a slot shares a bin and it moves none)."""
    v = _start(golden, single, SPLIT, sort_interval=sort_interval)
    d0 = v.schedule()["dyn_calls"]
    due = [k for k in range(single.T) if (d0 + k) % sort_interval == 0]
    assert due == lc.resort_steps(sort_interval)
    perms = {}

    def hook(k):
        if k in (due[0], due[0] + 2):
            perms[k] = v.env_order()[0].copy()

    out = _per_step(v, single, hook)
    torch.cuda.synchronize()
    a, b = perms[due[0]], perms[due[0] + 2]
    assert np.array_equal(np.sort(b), np.arange(single.n)) and not np.array_equal(a, b), "the first re-sort moved no row"
    assert np.array_equal(single.slots[a], single.slots[b])  # slot groups stay in place
    _check_rows(single, out)
    _check_end(single, v)
    _census(single, out, f"sort_interval {sort_interval}")
    v.close()


def test_lane_tracks(golden, lane):
    _step_form(golden, lane, dict(SPLIT, lane_tracks=1), "lane_tracks 1", dict(split=1, lane_tracks=1))


# =============================================================================== single agent, steps_device
def _steps_form(golden, case, sched, label, calls=None, expect=None, **kw):
    v = _start(golden, case, sched, **kw)
    s = v.schedule()
    for key, val in (expect or {}).items():
        assert s[key] == val, (key, s)
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
    _census(case, out, label)
    v.close()


@pytest.mark.parametrize("sort_interval", [0, 3, 8])
def test_steps_one_call(golden, single, sort_interval):
    """64 steps in one rx_steps call: sort_interval 0 carried and paired throughout, 3 and 8 with
    crossing re-sort steps.  KIN of step k + 1 reads, in the same launch, the flags, progress and
    step count REWARD of step k stored: the autoreset after a finish or a truncation."""
    _steps_form(golden, single, SPLIT, f"steps_device(64) sort_interval {sort_interval}",
                expect=dict(split=1, reward_lpe=1), sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 8])
def test_steps_in_calls_of_5_1_2_9_47(golden, single, sort_interval):
    _steps_form(golden, single, SPLIT, f"steps_device 5+1+2+9+47 sort_interval {sort_interval}", calls=(5, 1, 2, 9, 47),
                sort_interval=sort_interval)


@pytest.mark.parametrize("sort_interval", [0, 8])
def test_steps_stride0_rows(golden, single, sort_interval):
    """The env's own rows (stride 0): after the call they hold the trace's last step."""
    v = _start(golden, single, SPLIT, sort_interval=sort_interval)
    obs, rew, done = v.steps_device(_acts(single), full_info=True)
    assert obs is v.buf["obs"]
    torch.cuda.synchronize()
    _check_last_rows(single, v, outputs=True)
    _check_end(single, v)
    v.close()


def test_steps_captured_graph_replay(golden, single):
    """One replay of a graph captured over steps_device(64) from the injected state."""
    v = _start(golden, single, SPLIT, sort_interval=8)
    acts = _acts(single)
    out = _rows(v, single.T)
    torch.cuda.synchronize()
    cap = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap, capture_error_mode="thread_local"):
        v.steps_device(acts, obs_out=out["obs"], reward_out=out["reward"], done_out=out["done"], full_info=True)
    graph.replay()
    torch.cuda.synchronize()
    _check_rows(single, out)
    _check_last_rows(single, v)
    _check_end(single, v)
    _census(single, out, "captured graph")
    del graph
    v.close()


def test_steps_task_sort2(golden, single):
    _steps_form(golden, single, dict(SPLIT, task_sort=2), "steps_device task_sort 2", expect=dict(task_sort=2),
                sort_interval=5)


def test_steps_reward_lpe2_fallback(golden, single):
    _steps_form(golden, single, dict(SPLIT, reward_lpe=2), "steps_device reward_lpe 2", expect=dict(reward_lpe=2),
                sort_interval=3)


def test_steps_lane_tracks(golden, lane):
    _steps_form(golden, lane, dict(SPLIT, lane_tracks=1), "steps_device lane_tracks 1", expect=dict(lane_tracks=1))


# =============================================================================== two cars
TWO = {"one_kernel": (dict(split=-1), {}, dict(split=0)),
       "split_lane_per_env": (dict(split=1, reward_lpe=1), {}, dict(split=1, reward_lpe=1)),
       "split_lane_per_car": (dict(split=1, reward_lpe=2), {}, dict(split=1, reward_lpe=2)),
       "ray_lpr1": (dict(ray_lpr=1), {}, dict(ray_lpr=1)),
       "ray_lpr2": (dict(ray_lpr=2), {}, dict(ray_lpr=2)),
       "ray_order1": ({}, dict(sort_interval=2, ray_order=1), {}),
       "ray_order2": ({}, dict(sort_interval=2, ray_order=2), {})}


@pytest.mark.parametrize("form", list(TWO))
def test_two_cars(golden, multi, form):
    """One car crashed and frozen while the other races on, contact, a finish that ends the episode
    with a placement, a truncation placed by progress, finished_step and the start side of every
    autoreset: rewards of both cars, placement and info rows, and the whole state."""
    sched, kw, expect = TWO[form]
    _step_form(golden, multi, sched, f"two cars {form}", expect, **kw)


def test_two_cars_steps_fallback(golden, multi):
    _steps_form(golden, multi, {}, "two cars steps_device", sort_interval=3)


# =============================================================================== policy in the loop
def _agent():
    from rx.agent import Agent
    from rx.optim import FlatAdam
    from rx.spaces import Box
    torch.manual_seed(9)
    ag = Agent(Box(-1, 1, (15,)), Box(-1, 1, (2,))).cuda()
    fl = FlatAdam(ag, torch.optim.Adam(ag.parameters(), lr=1e-3, eps=1e-5), 0.5)
    return ag, fl


@pytest.mark.parametrize("form", ["k_rollout", "rollout_steps_split", "rollout_steps_default"])
def test_policy_in_the_loop(golden, oracle_dev, form):
    """rx_rollout (the persistent k_rollout) and rx_rollout_steps, fp32, from the short-lead state
    with a fixed noise tensor: the policy decides the actions, the oracle replays the recorded ones
    from the same state, and observations, rewards, dones, next_obs and the final state are equal."""
    from rx.ppo_fused import Rollout, StepRollout
    T = 16
    tab = golden.table()
    st0 = lc.policy_state0(golden, n_steps=T)
    n = len(st0["x"])
    shell = lc.run_single(tab, oracle_dev, st0, 1, actions=np.zeros((1, n, 2), np.float32))  # slots / state0 holder
    sched = dict(wide_n=-1) if form == "rollout_steps_default" else (SPLIT if form == "rollout_steps_split" else {})
    v = _start(golden, shell, sched)
    ag, fl = _agent()
    obs = torch.zeros((T, n, 15), device="cuda")
    actions = torch.zeros((T, n, 2), device="cuda")
    logprobs, dones, rewards, values = (torch.zeros((T, n), device="cuda") for _ in range(4))
    nobs, nd = torch.zeros((n, 15), device="cuda"), torch.zeros(n, device="cuda")
    obs[0].copy_(torch.from_numpy(lc.state_obs(tab, oracle_dev, st0)))
    eps = torch.randn((T, n, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    if form == "k_rollout":
        assert v.schedule()["wide"] == 1
        ro = Rollout(ag, fl, v, T)
    else:
        assert v.schedule()["wide"] == 0 and v.schedule()["split"] == 1
        ro = StepRollout(ag, fl, v, T)
    ro(obs, actions, logprobs, dones, rewards, values, nobs, nd, eps=eps)
    torch.cuda.synchronize()
    case = lc.run_single(tab, oracle_dev, st0, T, actions=actions.cpu().numpy())
    ev = case.events
    print(f"\n{form}: oracle events on the recorded actions (even/odd): " + lc.census_text(ev))
    assert ev["cp25"].sum() + ev["cp50"].sum() + ev["cp75"].sum() >= 5 and ev["finish"].sum() >= 5
    assert ev["trunc"].sum() >= 5 and case.trace["reset"][1:-1].sum() >= 5
    tr = case.trace
    _differs([("dones (of the step before)", dones[1:], tr["done"][:-1].astype(np.float32)),
              ("rewards", rewards, tr["reward64"].astype(np.float32)),
              ("obs (of the step before)", obs[1:], tr["obs"][:-1])])
    _differs([("next_done", nd[None], tr["done"][-1:].astype(np.float32)), ("next_obs", nobs[None], tr["obs"][-1:])],
             T - 1)
    assert np.array_equal((dones[1:].cpu().numpy() != 0).sum(1), tr["done"][:-1].sum(1))  # the device's own census
    _check_end(case, v)
    v.close()
