"""What the KAT tests of the lattice and the placed tracks share (tests/test_lattice_gpu.py,
tests/test_placed_gpu.py): an env on a cases module's slots, and the launch forms -- the raycast
alone, a state-injected single-agent step, a two-car step, a trace per step and under rx_steps --
each held BIT FOR BIT to the device-libm oracle over all rows, and to the reference's recorded
outputs on the comparable rows (masks exactly, floats within OBS_TOL / STATE_TOL).

``cases`` is tests.lattice_cases or tests.placed_cases: ``env_args(golden, slots)`` and
``table(golden)``.  The reference's rows may be a subset of the KAT rows (``idx``: placed.npz pins
a thinned share); the oracle comparison always takes every row.
"""
import numpy as np
import pytest
import torch

from oracle.orc import F_CP25, F_CP50, F_CP75, F_CRASHED, F_FINISHED, F_HAS_CRASHED
from tests import lattice_cases as lat
from tests.golden_util import multi_state_from, single_state_from
from tests.trace_checks import _acts, _check_end, _check_last_rows, _check_rows, _differs, _per_step, _rows, inject

OBS_TOL = lat.OBS_TOL  # north star: float observations / rewards against the reference
STATE_TOL = 1e-9       # f64 state after one step: ulp-level libm differences only (tests/test_env_gpu.py)
SPLIT = dict(wide_n=-1, dyn_lpe=1, split=1, reward_lpe=1, ray_lpr=1)
FLOATS = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering")
PATHS = {"default": (dict(wide_n=-1), dict(wide=0)), "split": (SPLIT, dict(split=1, dyn_lpe=1, wide=0)),
         "wide": (dict(wide_n=1000000), dict(wide=1))}
TWO = {"one_kernel": (dict(split=-1), {}, dict(split=0)),
       "split_lane_per_env": (dict(split=1, reward_lpe=1), {}, dict(split=1, reward_lpe=1)),
       "split_lane_per_car": (dict(split=1, reward_lpe=2), {}, dict(split=1, reward_lpe=2)),
       "ray_order1": ({}, dict(sort_interval=2, ray_order=1), {}),
       "ray_order2": ({}, dict(sort_interval=2, ray_order=2), {})}


def make_env(cases, golden, slots, n_agents=1, sched=None, expect=None, **kw):
    from rx.vector_env import RacingVectorEnv
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a HIP device")
    slots = np.asarray(slots, dtype=np.int32)
    cps, ws, ts = cases.env_args(golden, slots)
    v = RacingVectorEnv(cps, ws, n_agents=n_agents, device="cuda", track_set=ts, sched=dict(sched or {}), **kw)
    assert np.array_equal(v.track_of_env, slots)  # the env's slot ids are the cases'
    s = v.schedule()
    for key, val in (expect or {}).items():
        assert s[key] == val, (key, s)
    return v


def _all(idx):
    return slice(None) if idx is None else idx


# =============================================================================== ray KATs
def cast(cases, golden, rays, ok, sched, expect=None, counters=None, **kw):
    """step_device(phases=2): the raycast alone from the injected poses.  rays: kat, dev (the oracle's
    [n, 11]), t (the reference's, on rows ``idx`` of the KATs -- default all); ok: the comparable ones of
    those rows.  counters: a dict that receives the env's culling counters."""
    kat = rays["kat"]
    n = len(kat["ox"])
    v = make_env(cases, golden, kat["track"], sched=sched, expect=expect, autoreset="disabled", **kw)
    if counters is not None:
        v.enable_counters()
    v.set_state(x=kat["ox"], y=kat["oy"], angle=kat["dir"], progress=kat["progress"], last_progress=kat["progress"])
    obs = v.step_device(torch.zeros((n, 2), device="cuda"), phases=2)[0].cpu().numpy()[:, :11]
    if counters is not None:
        counters.update(v.read_counters())
    v.close()
    _differs([("rays", obs[None], rays["dev"][None])])
    obs = obs[_all(rays.get("idx"))]
    want = rays["t"].astype(np.float32) / np.float32(50.0)  # sensor 5: relative angle exactly 0
    np.testing.assert_allclose(obs[ok, 5], want[ok], rtol=0, atol=OBS_TOL)
    assert np.array_equal(obs[ok, 5] == 0, rays["t"][ok] == 0)  # a mask of its own: the origin ON a wall


# =============================================================================== single-agent step KATs
def inject_state(v, st):
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


def single_vs_reference(step, ok, g, obs, rew64, rew, term, trunc, info):
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


def step_single(cases, golden, oracle_dev, step, ok, sched, expect=None, ref=None, idx=None, counters=None, **kw):
    """One state-injected step of the KAT columns `step`.  ref / idx: the reference's recorded outputs
    and the KAT rows they belong to (default: `step` itself, every row)."""
    v = make_env(cases, golden, step["track"], sched=sched, expect=expect, autoreset="disabled", **kw)
    if counters is not None:
        v.enable_counters()
    inject_state(v, single_state_from(step))
    v.set_speed_weights(step["speed_weight"])
    obs, rew, _ = v.step_device(torch.from_numpy(step["action"]).cuda(), full_info=True)
    torch.cuda.synchronize()
    g = v.get_state()
    obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
    rew64 = v.buf["reward64"].cpu().numpy()
    term, trunc = v.buf["terminated"].cpu().numpy(), v.buf["truncated"].cpu().numpy()
    info = v.buf["info"].cpu().numpy()[:, 0]
    if counters is not None:
        counters.update(v.read_counters())
    v.close()
    st, (o_obs, o_rew, o_term, o_trunc, o_info) = lat.oracle_single(step, cases.table(golden), oracle_dev)
    fields = [("terminated", term, o_term.astype(np.uint8)), ("truncated", trunc, o_trunc.astype(np.uint8)),
              ("reward64", rew64, o_rew), ("info", info[:, :3], o_info), ("obs", obs, o_obs)]
    fields += [("state " + k, g[k], st[k]) for k in ("progress", "flags", "steps", "x", "y", "angle", "vx", "vy",
                                                     "last_progress", "last_steering")]
    _differs([(name, dev[None], ref_[None]) for name, dev, ref_ in fields])
    r = _all(idx)
    gg = g if idx is None else {k: g[k][idx] for k in ("flags", "steps", "progress", "x", "y", "angle", "vx", "vy")}
    single_vs_reference(step if ref is None else ref, ok, gg, obs[r], rew64[r], rew[r], term.astype(bool)[r],
                        trunc.astype(bool)[r], info[r])


# =============================================================================== two-car step KATs
def step_two(cases, golden, oracle_dev, step, ok, sched, kw, expect, ref=None, idx=None):
    v = make_env(cases, golden, step["track"], n_agents=2, sched=sched, expect=expect, autoreset="disabled", **kw)
    st0 = multi_state_from(step)
    flat = {k: st0[k].reshape(-1) for k in FLOATS + ("flags", "finished_step")}
    flat["steps"] = st0["steps"]
    inject_state(v, flat)
    obs, _, _ = v.step_device(torch.from_numpy(step["action"]).cuda(), full_info=True)
    torch.cuda.synchronize()
    g = v.get_state()
    obs = obs.cpu().numpy()
    rew64 = v.buf["reward64"].cpu().numpy()
    term, trunc = v.buf["terminated"].cpu().numpy(), v.buf["truncated"].cpu().numpy()
    info = v.buf["info"].cpu().numpy()
    v.close()
    st, (o_obs, o_rew, o_done, o_all, o_trunc, o_place, o_info) = lat.oracle_multi(step, cases.table(golden), oracle_dev)
    fields = [("terminated", term, o_done.astype(np.uint8)), ("truncated", trunc, o_trunc.astype(np.uint8)),
              ("placement", info[..., 3], o_place.astype(np.float64)), ("reward64", rew64, o_rew),
              ("info", info[..., :2], o_info), ("obs", obs, o_obs), ("state steps", g["steps"], st["steps"])]
    fields += [("state " + k, g[k].reshape(-1, 2), st[k]) for k in ("progress", "flags", "finished_step", "x", "y",
                                                                   "angle", "vx", "vy", "last_progress",
                                                                   "last_steering")]
    _differs([(name, dev[None], ref_[None]) for name, dev, ref_ in fields])
    step, r = (step if ref is None else ref), _all(idx)
    fl = g["flags"].reshape(-1, 2)[r]
    term, trunc, info, obs, rew64 = term.astype(bool)[r], trunc.astype(bool)[r], info[r], obs[r], rew64[r]
    for name, got, want in (("crashed", (fl & F_CRASHED) != 0, step["o_crashed"]),
                            ("finished", (fl & F_FINISHED) != 0, step["o_finished"]),
                            ("has_crashed", (fl & F_HAS_CRASHED) != 0, step["o_has_crashed"]),
                            ("finished_step", g["finished_step"].reshape(-1, 2)[r], step["o_finished_step"]),
                            ("done", term, step["o_done"]), ("done_all", term | trunc, step["o_done_all"]),
                            ("truncated", trunc, step["o_truncated"]),
                            ("placement", info[..., 3].astype(np.int32), step["o_placement"]),
                            ("progress", g["progress"].reshape(-1, 2)[r], step["o_progress"])):
        assert np.array_equal(got[ok], want[ok]), name
    np.testing.assert_allclose(obs[ok], step["o_obs"][ok], rtol=0, atol=OBS_TOL)
    np.testing.assert_allclose(rew64[ok], step["o_reward"][ok], rtol=0, atol=OBS_TOL)


# =============================================================================== traces
def start(cases, golden, case, sched, expect=None, **kw):
    v = make_env(cases, golden, case.slots, n_agents=case.n_agents, sched=sched, expect=expect, autoreset="next_step",
                 **kw)
    if case.n_agents == 2:  # resets take their start side from the reference's stream, as the trace did
        v.use_numpy_start_draws()
        np.random.seed(case.draw_seed)
    v.reset_device()
    inject(v, case)
    return v


def per_step_form(cases, golden, case, sched, expect=None, **kw):
    v = start(cases, golden, case, sched, expect, **kw)
    out = _per_step(v, case)
    torch.cuda.synchronize()
    _check_rows(case, out)
    _check_end(case, v)
    v.close()


def steps_form(cases, golden, case, sched, calls=None, expect=None, **kw):
    v = start(cases, golden, case, sched, expect, **kw)
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
