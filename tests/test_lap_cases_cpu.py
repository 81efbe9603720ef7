"""The lap-event cases are not vacuous (tests/lap_cases.py; DESIGN.md §4 "Lap events under
every schedule").

Every condition is a FLOOR on the census of the oracle's own trace: how often each event
occurs, on which parity of the step index (the two sub-steps of a paired launch) and on
which re-sort steps.  A missed floor is an input problem: change the placement or the seed,
never the floor.  No GPU is needed.
"""
import numpy as np
import pytest

from oracle.orc import F_FINISHED
from tests import lap_cases as lc


@pytest.fixture(scope="module")
def single(golden, oracle_dev):
    return lc.get("single", golden, oracle_dev)


@pytest.fixture(scope="module")
def multi(golden, oracle_dev):
    return lc.get("multi", golden, oracle_dev)


def _parity(ev, name):
    return int(ev[name][0::2].sum()), int(ev[name][1::2].sum())


def test_single_census_floors(single):
    ev = single.events
    print("\nsingle-agent census (even/odd steps):", lc.census_text(ev))
    assert single.n == 200 and np.bincount(single.slots).tolist() == [67, 67, 66] and single.T == 64
    for name in ("cp25", "cp50", "cp75", "finish", "trunc"):
        even, odd = _parity(ev, name)
        assert even >= 10 and odd >= 10, (name, even, odd)
        for si in (3, 8):
            on = int(ev[name][lc.resort_steps(si)].sum())
            print(f"  {name} on the re-sort steps of sort_interval {si}: {on}")
            assert on >= 1, (name, si)
        steps_hit = int((ev[name].sum(1) > 0).sum())
        assert steps_hit >= 16, (name, steps_hit)  # spread over the window, not one burst
    assert ev["crash"].sum() >= 5
    assert ev["back_wrap"].sum() >= 1 and ev["refused"].sum() >= 1
    # the cap: 29.9 on full throttle reaches (v + 0.5) 0.985 > 30 at the third step
    assert ev["capped"].sum() >= 1
    # resets inside the window, and episodes that go on after them
    assert single.stats[2] >= 50 and single.trace["reset"][1:-1].sum() >= 50


def test_single_trace_semantics(single):
    """The trace is a next-step-autoreset run: the step after an ending is a reset step
    (reward 0, not done, zero info), and every event implies its outputs."""
    tr, ev = single.trace, single.events
    done = tr["done"]
    assert np.array_equal(tr["reset"][1:], done[:-1]) and not tr["reset"][0].any()
    assert (tr["reward64"][tr["reset"]] == 0).all() and not done[tr["reset"]].any()
    assert (tr["info"][tr["reset"]] == 0).all()
    assert (tr["info"][..., 1][ev["finish"]] == 1.0).all() and tr["terminated"][ev["finish"]].all()
    assert (tr["reward64"][ev["finish"]] > 100).all()  # + 100 and the time bonus
    assert (tr["info"][..., 2][ev["back_wrap"]] < 0).all()
    assert not tr["terminated"][ev["refused"] & ~ev["crash"]].any()
    assert (tr["actions"].dtype == np.float32) and np.isfinite(tr["actions"]).all()


def test_single_case_is_deterministic(golden, oracle_dev, single):
    again = lc.single_case(golden, oracle_dev)
    for k, v in single.trace.items():
        assert np.array_equal(v, again.trace[k]), k
    for k, v in single.final.items():
        assert np.array_equal(v, again.final[k]), k


def test_first_step_masks_match_the_glibc_oracle(golden, oracle, oracle_dev, single, multi):
    """The reference's numerics (glibc sin / cos / pow) on the same states and actions: the
    first step's masks and flags are identical, so the placement rule's flags are what the
    reference's rules expect."""
    tab = golden.table()
    ref = lc.run_single(tab, oracle, single.state0, 1, actions=single.trace["actions"][:1])
    for k in ("terminated", "truncated"):
        assert np.array_equal(ref.trace[k][0], single.trace[k][0]), k
    dev = lc.run_single(tab, oracle_dev, single.state0, 1, actions=single.trace["actions"][:1])
    assert np.array_equal(ref.final["flags"], dev.final["flags"])
    assert np.array_equal(ref.final["steps"], dev.final["steps"])
    assert np.array_equal(ref.final["progress"], dev.final["progress"])
    ref2 = lc.run_multi(tab, oracle, multi.state0, 1, multi.draw_seed, actions=multi.trace["actions"][:1])
    dev2 = lc.run_multi(tab, oracle_dev, multi.state0, 1, multi.draw_seed, actions=multi.trace["actions"][:1])
    for k in ("terminated", "truncated"):
        assert np.array_equal(ref2.trace[k][0], multi.trace[k][0]), k
    assert np.array_equal(ref2.trace["info"][0, ..., 3], multi.trace["info"][0, ..., 3])  # placement
    for k in ("flags", "steps", "progress", "finished_step"):
        assert np.array_equal(ref2.final[k], dev2.final[k]), k


def test_lane_layout_has_events(golden, oracle_dev):
    case = lc.get("lane", golden, oracle_dev)
    ev = case.events
    print("\n21-slot layout census (even/odd steps):", lc.census_text(ev))
    assert case.n == 130 and len(np.unique(case.slots)) == 21
    for name in ("cp25", "cp50", "cp75", "finish", "trunc"):
        assert min(_parity(ev, name)) >= 5, name
    assert ev["crash"].sum() >= 5


def test_multi_census_floors(multi):
    ev = multi.events
    print("\ntwo-car census (even/odd steps):", lc.census_text(ev))
    assert multi.n == 130 and len(np.unique(multi.slots)) == 4
    assert min(_parity(ev, "checkpoint")) >= 20
    assert min(_parity(ev, "finish")) >= 5
    assert min(_parity(ev, "trunc_unfinished")) >= 10
    lone = int(ev["lone_crash"].any(0).sum())
    print(f"  envs with one car crashed and the other racing on: {lone}; frozen env-steps: "
          f"{int(ev['frozen'].sum())}; steps with contact: {int(ev['contact'].sum())}")
    assert lone >= 5
    assert ev["frozen"].sum() >= 100
    assert ev["contact"].sum() >= 3
    assert ev["placed_by_progress"].sum() >= 1 and ev["placed_by_finish"].sum() >= 1
    tr = multi.trace
    # F_HAS_CRASHED is charged once: a car frozen since an earlier step earns 0 (no progress, no speed
    # reward, no second - 160), or the - 5 of a contact, unless the step places the cars
    quiet = tr["frozen_car"] & ~tr["done"][:, :, None]
    assert quiet.sum() >= 50 and np.isin(tr["reward64"][quiet], (0.0, -5.0)).all()
    fs = tr["info"][..., 1][ev["placed_by_finish"]]
    assert (fs == 1.0).any(1).all()
    assert ((multi.final["flags"] & F_FINISHED) != 0).sum() == (multi.final["finished_step"] > 0).sum()
    assert 0 < ev["contact"].mean() < 1  # the hook is neither always nor never true
    assert np.array_equal(tr["reset"][1:], tr["done"][:-1])
    assert (tr["reward64"][tr["reset"]] == 0).all() and (tr["info"][tr["reset"]] == 0).all()


def test_policy_case_reaches_its_lines(golden, oracle_dev):
    """Short leads and T = 16 with synthetic policy-like actions N(0, 1) exp(log_std): the cars
    reach their checkpoint, line or step limit by inertia."""
    st = lc.policy_state0(golden)
    for log_std in (0.0, -0.3):
        a = (np.random.default_rng(3).normal(size=(16, len(st["x"]), 2)) * np.exp(log_std)).astype(np.float32)
        case = lc.run_single(golden.table(), oracle_dev, st, 16, actions=a)
        ev = case.events
        print(f"\npolicy case census, log_std {log_std} (even/odd steps):", lc.census_text(ev))
        cp = ev["cp25"].sum() + ev["cp50"].sum() + ev["cp75"].sum()
        assert cp >= 5 and ev["finish"].sum() >= 5 and ev["trunc"].sum() >= 5
        assert case.trace["reset"][1:-1].sum() >= 5  # autoresets inside the rollout
