"""Shared helpers for the two-car episode fixtures (tests/golden/traj_multi.npz and
eval_multi.npz, written by tests/golden/gen_golden.py from the reference):

* ``census`` / ``check_census``: what the trajectory set must contain (the generator
  asserts it when it writes the file, tests/test_multi_traj_cpu.py again from the file);
* ``replay``: every episode from ``multi_reset(order)`` through ``oracle.multi_step``,
  all episodes stepped side by side, in the fixture's own columns;
* ``eval_table`` / ``eval_replay`` / ``multi_metrics``: the evaluation pool's tracks, the
  oracle's replay of the recorded evaluation actions, and utils/metrics.py:80-150's
  bookkeeping restated in NumPy over such a replay.

Nothing here reads the reference or needs a GPU.
"""
import numpy as np

from oracle.orc import (F_CP25, F_CP50, F_CP75, F_CRASHED, F_FINISHED, F_HAS_CRASHED, TrackTable, multi_state,
                        sensor_angles)

REL2 = sensor_angles(11, np.pi / 2)
F64_COLS = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering")
EVAL_KEYS = ("total_reward", "progress", "finished", "crashed", "speed", "placement", "steps", "total_distance",
             "distance_per_step")


def flags_of(tm, sl=slice(None)):
    """The oracle / device flag byte of both cars from the fixture's boolean columns."""
    cp = tm["cp"][sl]
    return (tm["crashed"][sl].astype(np.uint8) * F_CRASHED + tm["finished"][sl].astype(np.uint8) * F_FINISHED
            + (cp[..., 0] != 0) * F_CP25 + (cp[..., 1] != 0) * F_CP50 + (cp[..., 2] != 0) * F_CP75
            + tm["has_crashed"][sl].astype(np.uint8) * F_HAS_CRASHED).astype(np.uint8)


def _runs(mask):
    """Length of the longest run of True in a 1-d mask."""
    best = cur = 0
    for m in mask:
        cur = cur + 1 if m else 0
        best = max(best, cur)
    return best


def census(tm):
    """What traj_multi.npz holds, per episode and in all (ISSUE census; plain Python values)."""
    off = tm["off"]
    eps = []
    for e in range(len(off) - 1):
        a, b = int(off[e]), int(off[e + 1])
        last = b - 1
        fin, crashed = tm["finished"][last], tm["crashed"][last]
        place = tm["placement"][last]
        rew = tm["reward"][a:b]
        hc = tm["has_crashed"][a:b]
        first_crash = [int(np.argmax(hc[:, q])) if hc[:, q].any() else -1 for q in range(2)]
        # the step a car's checkpoints were set at, and whether they came in order
        cp = tm["cp"][a:b].astype(bool)
        cp_order = []
        for q in range(2):
            at = [int(np.argmax(cp[:, q, k])) if cp[:, q, k].any() else -1 for k in range(3)]
            cp_order.append(all(t >= 0 for t in at) and at[0] < at[1] < at[2])
        # a frozen car: state constant from its crash on, -160 on exactly one step
        frozen = []
        for q in range(2):
            c = first_crash[q]
            if c < 0:
                frozen.append(False)
                continue
            const = all((tm[k][a + c:b, q] == tm[k][a + c, q]).all() for k in ("x", "y", "angle", "vx", "vy",
                                                                                 "progress"))
            # the crash step's reward holds the -160 (progress, contact and speed terms are far smaller)
            paid = int((rew[:, q] < -100).sum())
            frozen.append(bool(const and paid == 1 and rew[c, q] < -100))
        # the +250 (multi_racing_env.py:256-257): without it a step's reward stays below 50 unless the
        # car finishes, and a finisher is placed first; with it, it is at least 250 - 160 - 5
        big = np.argwhere(rew > 60.0)
        eps.append(dict(
            slot=int(tm["slot"][e]), order=int(tm["order"][e]), steps=b - a,
            finished=(bool(fin[0]), bool(fin[1])), crashed=(bool(crashed[0]), bool(crashed[1])),
            placement=(int(place[0]), int(place[1])), truncated=bool(tm["truncated"][last]),
            done=bool(tm["done"][last]), done_all=bool(tm["done_all"][last]),
            ended_only_at_last=bool(not tm["done_all"][a:last].any()),
            first_crash=tuple(first_crash), frozen=tuple(frozen), cp_in_order=tuple(cp_order),
            final_progress=(float(tm["progress"][last, 0]), float(tm["progress"][last, 1])),
            bonus_at=[(int(t), int(q)) for t, q in big],
            contact=int(tm["contact"][a:b].sum()), contact_run=_runs(tm["contact"][a:b]),
            car_ray_steps=int((tm["car_rays"][a:b] > 0).sum())))
    return dict(episodes=eps, contact=sum(e["contact"] for e in eps),
                contact_run=max(e["contact_run"] for e in eps),
                car_ray_steps=sum(e["car_ray_steps"] for e in eps),
                slots=sorted({e["slot"] for e in eps}), orders=sorted({e["order"] for e in eps}))


def check_census(c, widths):
    """The conditions the trajectory set was built to meet (ISSUE): asserts each."""
    eps = c["episodes"]
    assert len(c["slots"]) >= 3 and 16 in c["slots"], c["slots"]
    assert len({widths[s] for s in c["slots"]}) >= 2
    assert c["orders"] == [0, 1]
    for e in eps:  # every episode runs to dones['__all__'] and no further
        assert e["done_all"] and e["ended_only_at_last"], e
        assert sorted(e["placement"]) == [1, 2], e
        assert e["bonus_at"] == [(e["steps"] - 1, e["placement"].index(1))], e  # the +250: once, to the first
    assert any(e["finished"] == (True, False) for e in eps), "no episode where car 0 finishes first"
    assert any(e["finished"] == (False, True) for e in eps), "no episode where only car 1 finishes"
    both = [e for e in eps if e["crashed"] == (True, True) and not any(e["finished"])]
    assert both, "no all_crashed episode"
    for e in both:  # placement by progress (multi_racing_env.py:198-211: crashed and unfinished alike)
        p = e["final_progress"]
        assert p[0] != p[1] and e["placement"][int(p[1] > p[0])] == 1, e
    lone = [e for e in eps for q in range(2)
            if e["first_crash"][q] >= 0 and e["finished"][1 - q] and e["steps"] - 1 - e["first_crash"][q] >= 200
            and e["frozen"][q]]
    assert lone, "no episode where one car crashes and the other finishes >= 200 steps later"
    trunc = [e for e in eps if e["truncated"] and not any(e["finished"])]
    assert trunc and all(e["steps"] == 3000 and not e["done"] for e in trunc), "no episode truncated at 3000 steps"
    assert c["contact"] >= 50 and c["contact_run"] >= 10, (c["contact"], c["contact_run"])
    assert c["car_ray_steps"] >= 200, c["car_ray_steps"]
    for e in eps:
        if any(e["finished"]):
            assert any(e["cp_in_order"]), e


def check_placement_column(tm):
    """placement is 0 on every step but an episode's last, where it is a permutation of (1, 2)."""
    off = tm["off"]
    for e in range(len(off) - 1):
        a, b = int(off[e]), int(off[e + 1])
        assert (tm["placement"][a:b - 1] == 0).all(), e
        assert sorted(tm["placement"][b - 1]) == [1, 2], e


def replay(orc, table, slots, orders, actions, off, max_steps=None):
    """Every episode from multi_reset(order) through orc.multi_step, side by side (one env
    per episode, an ended episode fed zeros and ignored).  ``actions`` [S, 2, 2] with
    ``off`` [E + 1]; returns (reset, rows): reset = dict(obs, x, y, angle) [E, ...], rows =
    the per-step columns concatenated in the fixture's order [S, ...]."""
    E = len(slots)
    L = np.diff(off).astype(np.int64)
    if max_steps is not None:
        L = np.minimum(L, max_steps)
    st = multi_state(E)
    st["track"][:] = np.asarray(slots, dtype=np.int32)
    obs0 = orc.multi_reset(table, st, np.asarray(orders, dtype=np.uint8), REL2)
    reset = dict(obs=obs0.copy(), x=st["x"].copy(), y=st["y"].copy(), angle=st["angle"].copy())
    S = int(L.sum())
    out_off = np.concatenate([[0], np.cumsum(L)])
    rows = dict(obs=np.zeros((S, 2, obs0.shape[2]), np.float32), reward=np.zeros((S, 2)),
                done=np.zeros(S, bool), done_all=np.zeros(S, bool), truncated=np.zeros(S, bool),
                placement=np.zeros((S, 2), np.int32), info_speed=np.zeros((S, 2)), info_progress=np.zeros((S, 2)),
                finished_step=np.zeros((S, 2), np.int32), flags=np.zeros((S, 2), np.uint8),
                steps=np.zeros(S, np.int32))
    for k in F64_COLS:
        rows[k] = np.zeros((S, 2))
    act = np.zeros((E, 2, 2), np.float32)
    for t in range(int(L.max())):
        live = np.nonzero(t < L)[0]
        act[:] = 0.0
        act[live] = actions[off[live] + t]
        obs, rew, done, done_all, trunc, place, info = orc.multi_step(table, st, act, REL2)
        j = out_off[live] + t
        rows["obs"][j], rows["reward"][j] = obs[live], rew[live]
        rows["done"][j], rows["done_all"][j], rows["truncated"][j] = done[live], done_all[live], trunc[live]
        rows["placement"][j] = place[live]
        rows["info_speed"][j], rows["info_progress"][j] = info[live, :, 0], info[live, :, 1]
        rows["finished_step"][j], rows["flags"][j], rows["steps"][j] = (st["finished_step"][live], st["flags"][live],
                                                                        st["steps"][live])
        for k in F64_COLS:
            rows[k][j] = st[k][live]
    return reset, rows, out_off


# ----------------------------------------------------------------- evaluation
def eval_table(em):
    """The 8 (track, run) slots of rx.evaluate.eval_pool(4, 2) as an oracle TrackTable, built
    from the control points the fixture recorded; also returns (cps, widths) per episode."""
    from rx.track import TrackGeometry
    cps = [em["cp"][em["cp_off"][t]:em["cp_off"][t + 1]] for t in range(len(em["cp_off"]) - 1)]
    recs, ecp, ew = [], [], []
    for t in range(len(cps)):
        for r in range(int(em["num_runs"])):
            g = TrackGeometry(cps[t], int(em["widths"][r]))
            st = g.get_start_pos()
            recs.append(dict(wp=g.waypoints, nrm=g.normals, starts=g.segment_cache["starts"],
                             v2=g.segment_cache["v2"], start=np.array([float(s) for s in st]),
                             width=float(g.track_width), maxd=float(g.max_track_distance)))
            ecp.append(cps[t])
            ew.append(int(em["widths"][r]))
    return TrackTable(recs), ecp, ew


def multi_metrics(reset_xy, rows, a, b):
    """utils/metrics.py:80-150 over steps a..b-1 of a replay (``rows`` as ``replay`` returns
    them): both cars' totals, the car choice, and the returned dictionary."""
    n = b - a
    total_reward = [0, 0]
    total_distance = [0.0, 0.0]
    prev = None
    for j in range(a, b):
        pos = [(rows["x"][j, q], rows["y"][j, q]) for q in range(2)]
        for q in range(2):
            total_reward[q] += rows["reward"][j, q]
            if prev is not None:
                total_distance[q] += np.sqrt((pos[q][0] - prev[q][0]) ** 2 + (pos[q][1] - prev[q][1]) ** 2)
        prev = pos
    last = b - 1
    fin = [(rows["flags"][last, q] & F_FINISHED) != 0 for q in range(2)]
    pick = 0 if fin[0] else (1 if fin[1] else 0)
    place = int(rows["placement"][last, pick])
    return dict(total_reward=float(total_reward[pick]), progress=float(rows["info_progress"][last, pick]),
                finished=bool(fin[pick]), crashed=bool((rows["flags"][last, pick] & F_CRASHED) != 0),
                speed=float(rows["info_speed"][last, pick]), placement=place if place > 0 else None, steps=n,
                total_distance=float(total_distance[pick]),
                distance_per_step=float(total_distance[pick] / n) if n > 1 else 0, chosen=pick)


def eval_record(em, i):
    """Episode i's recorded dictionary (placement 0 -> None)."""
    d = {k: em[k][i] for k in EVAL_KEYS}
    d = dict(total_reward=float(d["total_reward"]), progress=float(d["progress"]), finished=bool(d["finished"]),
             crashed=bool(d["crashed"]), speed=float(d["speed"]),
             placement=int(d["placement"]) if d["placement"] > 0 else None, steps=int(d["steps"]),
             total_distance=float(d["total_distance"]), distance_per_step=float(d["distance_per_step"]))
    return d


def assert_metrics(got, ref, tag):
    """test_eval_golden_gpu.py's tolerances: integers, booleans and placement exact; progress,
    speed, distance_per_step within 1e-5; the totals within 1e-5 x max(1, |ref|).  Returns the
    worst float deviation (the totals' scaled by max(1, |ref|))."""
    assert got["steps"] == ref["steps"] and got["placement"] == ref["placement"], (tag, got, ref)
    assert got["finished"] == ref["finished"] and got["crashed"] == ref["crashed"], (tag, got, ref)
    worst = 0.0
    for k in ("progress", "speed", "distance_per_step"):
        d = abs(got[k] - ref[k])
        assert d <= 1e-5, (tag, k, got[k], ref[k])
        worst = max(worst, d)
    for k in ("total_reward", "total_distance"):
        d = abs(got[k] - ref[k]) / max(1.0, abs(ref[k]))
        assert d <= 1e-5, (tag, k, got[k], ref[k])
        worst = max(worst, d)
    return worst
