"""Two-car episodes and the two-car evaluation pinned to the reference, without a GPU.

tests/golden/traj_multi.npz holds whole MultiRacingEnv episodes (multi_racing_env.py:118-269)
from the reference's own reset to dones['__all__']; eval_multi.npz what utils/metrics.py:80-150
eval_multi_agent returned on the evaluation pool (gen_golden.py gen_traj_multi / gen_eval_multi).
Here:

* the census the trajectory set was built to meet is asserted again from the file alone;
* every step of every episode is replayed from ``multi_reset(order)`` through
  ``oracle.multi_step``.  The glibc build must equal every recorded column bit for bit (the
  README's claim for the oracle).  The device-libm build must have every mask, ``progress``,
  ``steps``, ``finished_step`` and ``placement`` equal, observations and rewards within
  OBS_TOL = 1e-5 (a missed or extra -5 of a contact step would show there) and the state
  within STATE_TOL = 1e-9: tests/test_env_gpu.py's bounds;
* a NumPy restatement of eval_multi_agent's bookkeeping over the oracle's replay of the
  recorded evaluation actions reproduces the recorded dictionaries, and so does
  rx.evaluate._record_summary (the fused evaluator's host half) on a record built from the
  same replay.
"""
import numpy as np
import pytest

from tests import multi_traj_cases as mtc
from tests.golden_util import load

OBS_TOL = 1e-5      # tests/test_env_gpu.py
STATE_TOL = 1e-9


@pytest.fixture(scope="module")
def tm():
    return load("traj_multi.npz")


@pytest.fixture(scope="module")
def em():
    return load("eval_multi.npz")


def test_census(tm, golden):
    c = mtc.census(tm)
    mtc.check_census(c, [t["width"] for t in golden.tracks])
    mtc.check_placement_column(tm)
    L = np.diff(tm["off"])
    # the wrapper rows: the two shortest episodes, at most 400 steps of each
    assert sorted(tm["wrap_episode"]) == sorted(np.argsort(L, kind="stable")[:2])
    assert np.array_equal(tm["wrap_len"], np.minimum(L[tm["wrap_episode"]], 400))
    assert np.array_equal(tm["steps"], np.concatenate([np.arange(1, n + 1) for n in L]))


def _replay(orc, golden, tm):
    return mtc.replay(orc, golden.table(), tm["slot"], tm["order"], tm["actions"], tm["off"])


def test_glibc_oracle_replays_every_episode_bit_for_bit(tm, golden, oracle):
    reset, rows, off = _replay(oracle, golden, tm)
    assert np.array_equal(off, tm["off"])
    assert np.array_equal(reset["obs"], tm["reset_obs"])
    for k in ("x", "y", "angle"):
        assert np.array_equal(reset[k], tm["reset_" + k]), k
    for k in ("obs", "reward", "done", "done_all", "truncated", "placement", "info_speed", "info_progress",
              "finished_step", "steps") + mtc.F64_COLS:
        bad = np.nonzero((rows[k] != tm[k]).reshape(len(rows[k]), -1).any(axis=1))[0]
        assert bad.size == 0, (k, "first differing step", int(bad[0]), "of", bad.size)
    assert np.array_equal(rows["flags"], mtc.flags_of(tm))


def test_device_libm_oracle_replays_every_episode(tm, golden, oracle_dev):
    reset, rows, _ = _replay(oracle_dev, golden, tm)
    assert np.array_equal(reset["obs"], tm["reset_obs"])
    for k in ("done", "done_all", "truncated", "placement", "finished_step", "steps", "progress", "last_progress",
              "info_progress"):
        assert np.array_equal(rows[k], tm[k]), k
    assert np.array_equal(rows["flags"], mtc.flags_of(tm))
    worst = max(float(np.abs(rows["obs"] - tm["obs"]).max()), float(np.abs(rows["reward"] - tm["reward"]).max()))
    state = max(float(np.abs(rows[k] - tm[k]).max()) for k in ("x", "y", "angle", "vx", "vy", "last_steering",
                                                                  "info_speed"))
    print(f"\ndevice-libm oracle vs reference over {len(tm['steps'])} two-car steps: "
          f"max |obs/reward| {worst:.3g}, max |state| {state:.3g}")
    assert worst <= OBS_TOL and state <= STATE_TOL


def _eval_replays(orc, em):
    table, _, _ = mtc.eval_table(em)
    main = mtc.replay(orc, table, np.arange(8), em["orders"][:8], em["actions"], em["off"][:9])
    short = mtc.replay(orc, table, [0], em["orders"][8:9], em["actions"], em["off"][8:10])
    return main, short


def test_eval_pool_is_the_protocols(em):
    from rx.evaluate import eval_pool
    cps, ws, ids = eval_pool(4, 2)
    assert ids == [(t, r) for t in range(4) for r in range(2)]
    _, ecp, ew = mtc.eval_table(em)
    assert ew == [int(w) for w in ws]
    for a, b in zip(ecp, cps):
        assert np.array_equal(a, b)
    # the recorded start orders are the seed's stream of np.random.shuffle([0, 1]) calls
    st = np.random.RandomState(int(em["seed"]))
    want = []
    for _ in em["orders"]:
        o = [0, 1]
        st.shuffle(o)
        want.append(o[0])
    assert want == list(em["orders"])


@pytest.mark.parametrize("build", ["glibc", "device_libm"])
def test_eval_bookkeeping_reproduces_the_recorded_dictionaries(em, oracle, oracle_dev, build):
    """eval_multi_agent restated over the oracle's replay; which car is reported, placement
    (None when max_steps ends the loop) and steps exact, floats at test_eval_golden_gpu.py's
    tolerances.  The same replay as a [N, 2, RX_EVAL_W] record through _record_summary."""
    from rx import _lib
    from rx.evaluate import _record_summary
    orc = oracle if build == "glibc" else oracle_dev
    (reset, rows, off), (reset_s, rows_s, off_s) = _eval_replays(orc, em)
    fin = em["finished_cars"].astype(bool)
    # the set holds both branches of the car choice, a crash ending and a truncation
    assert [True, False] in fin[:8].tolist() and [False, True] in fin[:8].tolist()
    none = ~fin[:8].any(axis=1)
    assert (none & (em["steps"][:8] < 3000)).any() and (none & (em["steps"][:8] == 3000)).any()
    worst = 0.0
    rec = np.zeros((8, 2, _lib.RX_EVAL_W))
    for i in range(8):
        a, b = int(off[i]), int(off[i + 1])
        got = mtc.multi_metrics(None, rows, a, b)
        assert got["chosen"] == int(fin[i, 1] and not fin[i, 0]), i
        worst = max(worst, mtc.assert_metrics(got, mtc.eval_record(em, i), i))
        d = np.sqrt(np.diff(rows["x"][a:b], axis=0) ** 2 + np.diff(rows["y"][a:b], axis=0) ** 2).sum(axis=0)
        for q in range(2):
            rec[i, q, :7] = (rows["reward"][a:b, q].sum(), d[q], b - a, rows["info_progress"][b - 1, q],
                             rows["info_speed"][b - 1, q], rows["placement"][b - 1, q], rows["flags"][b - 1, q])
    got = mtc.multi_metrics(None, rows_s, 0, int(off_s[1]))
    ref = mtc.eval_record(em, 8)
    assert ref["placement"] is None and ref["steps"] == 40
    worst = max(worst, mtc.assert_metrics(got, ref, 8))
    print(f"\n{build} oracle: worst evaluation metric deviation {worst:.3g}")
    if build == "glibc":
        assert worst <= 1e-9  # the same arithmetic on the same numbers; sums in another order
    eps = _record_summary(rec)["all_episodes"]
    for i in range(8):
        mtc.assert_metrics(eps[i], mtc.eval_record(em, i), ("record", i))
