"""rx_assign uploads rx_assign_plan's plan (include/rx.h, DESIGN.md §3 "Plan, then upload"):
on small handles rx_schedule, rx_ray_waves and rx_env_order report, entry for entry, what the
pure function returns for the same config, track table and slots (its tables are held to the
kernels' rules on the CPU, tests/test_assign_plan_cpu.py); and an rx_assign that is refused
leaves the handle as it was.
"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HANDLES = {
    "defaults": ((1, 64, 65), 1, {}),
    "lane_varying": ((1, 64, 65), 1, dict(lane_tracks=1, dyn_lpe=1)),
    "tail": ((1, 64, 65), 1, dict(ray_lpr=1, ray_dispatch=3, ray_tail=3, ray_tail_lpr=4)),
    "wide": ((64,), 1, {}),
    "two_car": ((33, 37), 2, {}),
}


def _env(counts, n_agents, sched):
    from rx.track import gen_tracks
    from rx.vector_env import RacingVectorEnv
    random.seed(3)
    np.random.seed(3)
    tracks = gen_tracks(num_tracks=len(counts), seed=None)
    pool = [tracks[k] for k, n in enumerate(counts) for _ in range(n)]
    widths = [6 + k for k, n in enumerate(counts) for _ in range(n)]
    order = np.random.RandomState(5).permutation(len(pool))  # the slots interleaved in env order
    return RacingVectorEnv([pool[i] for i in order], [widths[i] for i in order], n_agents=n_agents, device="cuda",
                           sched=sched)


def _raw_ray_waves(env):
    t = env.ray_wave_table()
    return np.stack([t[k] for k in ("track", "perm_start", "task_start", "count")], axis=1)


@pytest.mark.parametrize("name", list(HANDLES))
def test_handle_reports_the_plan(name):
    counts, A, sched = HANDLES[name]
    env = _env(counts, A, sched)
    assert sorted(np.bincount(env.track_of_env)) == sorted(counts)
    plan = env.assign_plan()
    got = env.schedule()
    assert got.pop("dyn_calls") >= 0 and plan["schedule"].pop("dyn_calls") == 0
    assert got == plan["schedule"]
    if name == "lane_varying":
        assert got["lane_tracks"] == 1
    if name == "wide":
        assert got["wide"] == 1
    assert np.array_equal(_raw_ray_waves(env), plan["ray_waves"])
    perm, bins, shift = env.env_order()
    assert np.array_equal(perm, plan["perm"]) and (bins, shift) == (plan["sort_bins"], plan["sort_shift"])
    env.close()


def test_refused_assign_leaves_the_handle_as_it_was():
    from rx import _lib
    counts, A, sched = HANDLES["defaults"]
    seen, clean = _env(counts, A, sched), _env(counts, A, sched)
    bad = seen.track_of_env.copy()
    bad[77] = len(counts)
    assert seen.L.rx_assign(seen._h, _lib.ptr(bad)) == _lib.RX_EINVAL
    assert f"env 77 assigned to track {len(counts)}" in seen.L.rx_last_error().decode()
    assert seen.schedule() == clean.schedule()
    assert np.array_equal(_raw_ray_waves(seen), _raw_ray_waves(clean))
    assert torch.equal(seen.reset_device(), clean.reset_device())
    g = torch.Generator(device="cuda").manual_seed(11)
    for t in range(3):
        a = torch.rand((seen.num_envs, 2), device="cuda", generator=g) * 2 - 1
        for x, y in zip(seen.step_device(a), clean.step_device(a)):
            assert torch.equal(x, y), t
    sa, sb = seen.get_state(), clean.get_state()
    for k in ("x", "y", "angle", "vx", "vy", "progress", "steps", "flags"):
        assert np.array_equal(sa[k], sb[k]), k
    seen.close()
    clean.close()
