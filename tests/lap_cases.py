"""Event-rich step cases built with the oracle alone (DESIGN.md §4 "Lap events under
every schedule").

The step kernels are compared bit for bit with the device-libm oracle, but under uniform
random play from a reset a car crashes near the start line: checkpoints, the finish, the
refused finish, truncation, the progress wraps, a frozen crashed car beside a racing one,
placement and contact never occur, and every car of a slot stands near waypoint 0.  The
cases here put cars all round the lap, a few waypoints before a checkpoint or the line,
with step counters a few steps before the limit, and drive them with a scripted controller
while the ORACLE steps them: the actions and the whole trace (gymnasium next-step autoreset
emulated as tests/test_env_gpu.py::test_random_rollout_bit_exact_vs_oracle_dev does) are
complete before any kernel runs.  tests/test_lap_cases_cpu.py checks that the events occur
(the census floors); tests/test_lap_events_gpu.py runs every launch form against the trace.

Placement: env e of slot s stands on waypoint i = (floor(line W) - lead) mod W, heading along
wp[i + 1] - wp[i], at speed U(12, 29) along that tangent, progress = last_progress = i / W,
holding the checkpoint flags of a car that drove there; line cycles over 0.25, 0.5, 0.75
and 1.0, lead ~ U{1 .. 39}.  steps ~ U{0 .. 1999} or 3000 - U{1 .. K - 1}, even odds.
Controller: steering = clip(2 (heading error to wp[closest + 6]) + N(0, 0.1), -1.2, 1.2),
throttle ~ U(0.2, 1), both float32; about one car in seven plays uniformly at random.
"""
import numpy as np

from oracle.orc import (F_CP25, F_CP50, F_CP75, F_CRASHED, F_FINISHED, F_HAS_CRASHED, multi_state, sensor_angles,
                        single_state)

K = 64
MAX_STEPS = 3000
LINES = (0.25, 0.5, 0.75, 1.0)
REL1 = sensor_angles(11, np.pi / 3)
REL2 = sensor_angles(11, np.pi / 2)
ALL_CP = F_CP25 | F_CP50 | F_CP75
# controller kinds
PURSUIT, WILD, COAST, FULL = 0, 1, 2, 3


def resort_steps(sort_interval, n_steps=K):
    """The steps of a call that begins right after the reset whose re-sort is due: the reset
    is dynamics launch 0, so step k is launch k + 1."""
    return [k for k in range(n_steps) if (k + 1) % sort_interval == 0]


def _cp_flags(i, W):
    p = i / W
    return (F_CP25 if p >= 0.25 else 0) | (F_CP50 if p >= 0.5 else 0) | (F_CP75 if p >= 0.75 else 0)


def _pose(tab, slot, i, speed, lateral=0.0, reverse=False):
    """(x, y, angle, vx, vy) on waypoint i of the slot, `lateral` along its normal."""
    o = int(tab.wp_off[slot])
    W = int(tab.wp_off[slot + 1]) - o
    a, b = tab.wp[o + i % W], tab.wp[o + (i + 1) % W]
    ang = np.arctan2(b[1] - a[1], b[0] - a[0]) + (np.pi if reverse else 0.0)
    ang = float(np.mod(ang, 2 * np.pi))
    n = tab.nrm[o + i % W]
    return (a[0] + n[0] * lateral, a[1] + n[1] * lateral, ang, speed * np.cos(ang), speed * np.sin(ang))


def _steps_draw(rng, n, horizon):
    late = rng.random(n) < 0.5
    return np.where(late, MAX_STEPS - rng.integers(1, horizon, n), rng.integers(0, 2000, n)).astype(np.int32)


def _widths(tab, slots):
    return (tab.wp_off[slots + 1] - tab.wp_off[slots]).astype(np.int64)


def _pursuit(tab, slots, st_x, st_y, st_angle, st_progress, rng, lateral=None):
    """clip(2 (heading error to wp[closest + 6]) + N(0, 0.1), -1.2, 1.2); closest = progress W."""
    W = _widths(tab, slots)
    c = np.rint(st_progress * W).astype(np.int64) % W
    g = tab.wp_off[slots] + (c + 6) % W
    tx, ty = tab.wp[g, 0], tab.wp[g, 1]
    if lateral is not None:
        tx, ty = tx + tab.nrm[g, 0] * lateral, ty + tab.nrm[g, 1] * lateral
    err = np.arctan2(ty - st_y, tx - st_x) - st_angle
    err = np.mod(err + np.pi, 2 * np.pi) - np.pi
    return np.clip(2.0 * err + rng.normal(0.0, 0.1, len(slots)), -1.2, 1.2)


class Case:
    """state0 (the injected state), slots, actions [T, N, (2,) 2] float32 and the oracle's trace."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return len(self.slots)


# ------------------------------------------------------------------------------ single agent
def single_state0(tab, slots, seed, horizon=K, max_lead=39, extras=True):
    """The injected state and each env's controller kind."""
    rng = np.random.default_rng(seed)
    slots = np.asarray(slots, dtype=np.int32)
    n = len(slots)
    st = single_state(n)
    st["track"][:] = slots
    st["steps"][:] = _steps_draw(rng, n, horizon)
    kind = np.where(rng.random(n) < 1.0 / 7.0, WILD, PURSUIT)
    lead = rng.integers(1, max_lead + 1, n)
    speed = rng.uniform(12.0, 29.0, n)
    group = np.full(n, -1)
    if extras:  # four groups of 8 envs spread over the slots: envs 5, 11, 17, ... in turn
        pick = 5 + 6 * np.arange(32)
        group[pick] = np.arange(32) % 4
    for e in range(n):
        s = int(slots[e])
        W = int(tab.wp_off[s + 1] - tab.wp_off[s])
        i = (int(LINES[e % 4] * W) - int(lead[e])) % W
        fl, rev, v = None, False, float(speed[e])
        if group[e] == 0:  # just past the line, heading backwards at 15: the backward wrap
            i, fl, rev, v, kind[e] = 1 + e % 3, 0, True, 15.0, COAST
        elif group[e] == 1:  # before the line with a checkpoint flag missing: the refused finish
            i, kind[e] = W - 1 - e % 5, PURSUIT
            fl = (F_CP25 | F_CP50, F_CP25, 0)[e % 3]
        elif group[e] == 2:  # 29.9 on full throttle: the speed cap
            v, kind[e] = 29.9, FULL
        x, y, ang, vx, vy = _pose(tab, s, i, v, reverse=rev)
        st["x"][e], st["y"][e], st["angle"][e], st["vx"][e], st["vy"][e] = x, y, ang, vx, vy
        st["progress"][e] = st["last_progress"][e] = i / W
        st["flags"][e] = _cp_flags(i, W) if fl is None else fl
        if group[e] == 3:  # already crashed: one frozen step, -60, terminated
            st["flags"][e] |= F_CRASHED
    return st, kind


def _single_actions(tab, st, kind, rng):
    n = len(kind)
    steer = _pursuit(tab, st["track"], st["x"], st["y"], st["angle"], st["progress"], rng)
    thr = rng.uniform(0.2, 1.0, n)
    w_steer, w_thr = rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    steer = np.where(kind == WILD, w_steer, steer)
    thr = np.where(kind == WILD, w_thr, thr)
    coast = kind == COAST
    steer = np.where(coast, np.clip(rng.normal(0.0, 0.1, n), -1.2, 1.2), steer)
    thr = np.where(coast, 0.0, np.where(kind == FULL, 1.0, thr))
    return np.stack([steer, thr], 1).astype(np.float32)


def run_single(tab, oracle, state0, n_steps, actions=None, kind=None, seed=0):
    """Step the oracle n_steps from a copy of state0 with next-step autoreset.  actions
    [T, N, 2] given: replay them; else the controller draws them from the oracle's state."""
    st = {k: v.copy() for k, v in state0.items()}
    n = len(st["x"])
    rng = np.random.default_rng(seed + 1000)
    kind = None if kind is None else kind.copy()
    T = n_steps
    out = dict(actions=np.zeros((T, n, 2), np.float32), obs=np.zeros((T, n, 15), np.float32),
               reward64=np.zeros((T, n)), terminated=np.zeros((T, n), bool), truncated=np.zeros((T, n), bool),
               info=np.zeros((T, n, 4)), reset=np.zeros((T, n), bool))
    ev = {k: np.zeros((T, n), bool) for k in ("cp25", "cp50", "cp75", "finish", "trunc", "crash", "back_wrap",
                                             "refused", "capped")}
    ep_ret, ep_len = np.zeros(n), np.zeros(n, np.int32)
    stats = [0.0, 0, 0]
    pending = np.zeros(n, bool)
    for t in range(T):
        a = actions[t] if actions is not None else _single_actions(tab, st, kind, rng)
        fl0, lp0 = st["flags"].copy(), st["last_progress"].copy()
        obs, rew, term, trunc, info = oracle.single_step(tab, st, a, REL1)
        live = ~pending
        if pending.any():  # (the oracle stepped the pending envs first; their reset overwrites that)
            r_obs = oracle.single_reset(tab, st, REL1, mask=pending)
            obs[pending] = r_obs[pending]
            rew[pending], term[pending], trunc[pending], info[pending] = 0.0, False, False, 0.0
            if kind is not None:
                kind[pending & ((kind == COAST) | (kind == FULL))] = PURSUIT
        new = st["flags"] & ~fl0
        p = st["progress"]
        ev["cp25"][t], ev["cp50"][t], ev["cp75"][t] = (live & ((new & b) != 0) for b in (F_CP25, F_CP50, F_CP75))
        ev["finish"][t] = live & ((new & F_FINISHED) != 0)
        ev["trunc"][t] = trunc
        ev["crash"][t] = term & ((st["flags"] & F_CRASHED) != 0)
        ev["back_wrap"][t] = live & (lp0 < 0.1) & (p > 0.9) & (info[:, 2] < 0)
        ev["refused"][t] = live & (lp0 > 0.9) & (p < 0.1) & (info[:, 2] > 0) & ((st["flags"] & F_FINISHED) == 0)
        ev["capped"][t] = live & (info[:, 0] == 30.0)
        ep_ret = np.where(pending, 0.0, ep_ret + rew)
        ep_len = np.where(pending, 0, ep_len + 1).astype(np.int32)
        ended = term | trunc
        stats[0] += float(ep_ret[ended].sum())
        stats[1] += int(ep_len[ended].sum())
        stats[2] += int(ended.sum())
        out["actions"][t], out["obs"][t], out["reward64"][t] = a, obs, rew
        out["terminated"][t], out["truncated"][t], out["reset"][t] = term, trunc, pending
        out["info"][t, :, :3] = info
        pending = ended
    final = dict(st, env_flags=pending.astype(np.uint8), ep_return=ep_ret, ep_length=ep_len)
    out["done"] = out["terminated"] | out["truncated"]
    return Case(slots=state0["track"].copy(), state0={k: v.copy() for k, v in state0.items()}, T=T, trace=out,
                events=ev, final=final, stats=tuple(stats), n_agents=1)


def single_case(golden, oracle, seed=7, n=200, n_slots=3, n_steps=K, extras=True):
    tab = golden.table()
    slots = np.arange(n) % n_slots
    st, kind = single_state0(tab, slots, seed, horizon=n_steps, extras=extras)
    return run_single(tab, oracle, st, n_steps, kind=kind, seed=seed)


def lane_case(golden, oracle, seed=6):
    """130 envs on all 21 golden slots (lane_tracks = 1: three blocks, the last one ragged)."""
    return single_case(golden, oracle, seed=seed, n=130, n_slots=golden.n_tracks, extras=False)


def policy_state0(golden, seed=8, n=200, n_slots=3, n_steps=16):
    """Short leads (1 .. 8 waypoints) and T = 16: the cars reach their line by inertia, whatever
    the policy decides."""
    st, _ = single_state0(golden.table(), np.arange(n) % n_slots, seed, horizon=n_steps, max_lead=8, extras=False)
    return st


def state_obs(tab, oracle, state0):
    """The observation of a state: the oracle's step of a copy marked crashed does not move the
    car, and reports its rays and velocity columns."""
    st = {k: v.copy() for k, v in state0.items()}
    st["flags"] = st["flags"] | np.uint8(F_CRASHED)
    a = np.stack([st["last_steering"], np.zeros_like(st["x"])], 1).astype(np.float32)
    return oracle.single_step(tab, st, a, REL1)[0]


def census_text(ev):
    """Per event: its count on even / on odd step indices (the two sub-steps of a paired launch)."""
    return ", ".join(f"{k} {int(v[0::2].sum())}/{int(v[1::2].sum())}" for k, v in ev.items())


def single_masks(terminated, truncated, info):
    """The census a run's own outputs give ([T, N] masks and [T, N, >= 3] info rows): per
    step the number of terminations, truncations, finishes, crashes, backward steps, capped speeds."""
    fin = terminated & (info[..., 1] == 1.0)
    m = dict(term=terminated, trunc=truncated, finish=fin, crash=terminated & ~fin, backward=info[..., 2] < 0,
             capped=info[..., 0] == 30.0)
    return {k: v.sum(1).astype(int) for k, v in m.items()}


# ------------------------------------------------------------------------------ two cars
def replay_first(rs, k):
    """agent_order[0] of the reference's next k resets: np.random.shuffle on [0, 1], env order."""
    out = np.zeros(k, np.uint8)
    for j in range(k):
        order = [0, 1]
        rs.shuffle(order)
        out[j] = order[0]
    return out


def multi_state0(tab, slots, seed, horizon=K):
    rng = np.random.default_rng(seed)
    slots = np.asarray(slots, dtype=np.int32)
    n = len(slots)
    st = multi_state(n)
    st["track"][:] = slots
    st["steps"][:] = _steps_draw(rng, n, horizon)
    wild = rng.random((n, 2)) < 1.0 / 7.0
    lead = rng.integers(1, 40, n)
    speed = rng.uniform(12.0, 29.0, (n, 2))
    gap = np.array([3.5, 3.5, 2.0, 1.0])[(np.arange(n) // 4) % 4]  # half the pairs clear of each other; 1.0: contact
    lane = np.stack([-gap / 2, gap / 2], 1)
    for e in range(n):
        s = int(slots[e])
        W = int(tab.wp_off[s + 1] - tab.wp_off[s])
        i = (int(LINES[e % 4] * W) - int(lead[e])) % W
        for q in range(2):
            x, y, ang, vx, vy = _pose(tab, s, i, float(speed[e, q]), lateral=float(lane[e, q]))
            st["x"][e, q], st["y"][e, q], st["angle"][e, q], st["vx"][e, q], st["vy"][e, q] = x, y, ang, vx, vy
            st["progress"][e, q] = st["last_progress"][e, q] = i / W
            st["flags"][e, q] = _cp_flags(i, W)
    return st, wild, lane


def _multi_actions(tab, st, wild, lane, rng):
    n = len(st["steps"])
    a = np.zeros((n, 2, 2))
    for q in range(2):
        a[:, q, 0] = _pursuit(tab, st["track"], st["x"][:, q], st["y"][:, q], st["angle"][:, q], st["progress"][:, q],
                              rng, lateral=lane[:, q])
        a[:, q, 1] = rng.uniform(-0.6, 1.0, n)
    w = rng.uniform(-1.0, 1.0, (n, 2, 2))
    return np.where(wild[:, :, None], w, a).astype(np.float32)


def _corners(x, y, ang):
    L = np.array([[2.0, 1.0], [2.0, -1.0], [-2.0, -1.0], [-2.0, 1.0]])
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    return np.stack([c * L[:, 0] - s * L[:, 1] + x[:, None], s * L[:, 0] + c * L[:, 1] + y[:, None]], 2)  # [n, 4, 2]


def touching(st):
    """Census hook: do the two cars' rectangles overlap (separating axes, as multi_car.py)?"""
    A = _corners(st["x"][:, 0], st["y"][:, 0], st["angle"][:, 0])
    B = _corners(st["x"][:, 1], st["y"][:, 1], st["angle"][:, 1])
    hit = np.ones(len(A), bool)
    for R in (A, B):
        for i in range(2):
            ax = np.stack([-(R[:, i + 1, 1] - R[:, i, 1]), R[:, i + 1, 0] - R[:, i, 0]], 1)
            pa, pb = (A * ax[:, None, :]).sum(2), (B * ax[:, None, :]).sum(2)
            hit &= ~((pa.max(1) < pb.min(1)) | (pb.max(1) < pa.min(1)))
    return hit


def run_multi(tab, oracle, state0, n_steps, draw_seed, actions=None, wild=None, lane=None, seed=0):
    """As run_single for two cars.  The start side of every reset comes from the reference's own
    stream: np.random.RandomState(draw_seed) after the N draws of the reset that precedes the
    injection, one shuffle per resetting env in env order (tests/test_start_draws_gpu.py)."""
    st = {k: v.copy() for k, v in state0.items()}
    n = len(st["steps"])
    rng = np.random.default_rng(seed + 1000)
    rs = np.random.RandomState(draw_seed)
    replay_first(rs, n)
    T = n_steps
    out = dict(actions=np.zeros((T, n, 2, 2), np.float32), obs=np.zeros((T, n, 2, 19), np.float32),
               reward64=np.zeros((T, n, 2)), terminated=np.zeros((T, n), bool), truncated=np.zeros((T, n), bool),
               info=np.zeros((T, n, 2, 4)), reset=np.zeros((T, n), bool), frozen_car=np.zeros((T, n, 2), bool))
    ev = {k: np.zeros((T, n), bool) for k in ("checkpoint", "finish", "trunc", "trunc_unfinished", "both_crashed",
                                             "lone_crash", "frozen", "contact", "placed_by_progress",
                                             "placed_by_finish")}
    ep_ret, ep_len = np.zeros(n), np.zeros(n, np.int32)
    stats = [0.0, 0, 0]
    pending = np.zeros(n, bool)
    for t in range(T):
        a = actions[t] if actions is not None else _multi_actions(tab, st, wild, lane, rng)
        fl0 = st["flags"].copy()
        obs, rew, term, _, trunc, place, info = oracle.multi_step(tab, st, a, REL2)
        touch = touching(st)
        live = ~pending
        if pending.any():
            first = np.zeros(n, np.uint8)
            first[pending] = replay_first(rs, int(pending.sum()))
            r_obs = oracle.multi_reset(tab, st, first, REL2, mask=pending)
            obs[pending] = r_obs[pending]
            rew[pending], term[pending], trunc[pending], place[pending], info[pending] = 0.0, False, False, 0, 0.0
        fl = st["flags"]
        new = fl & ~fl0
        fin = ((fl & F_FINISHED) != 0).any(1)
        crashed0, crashed = (fl0 & F_CRASHED) != 0, (fl & F_CRASHED) != 0
        ended = term | trunc
        ev["checkpoint"][t] = live & ((new & ALL_CP) != 0).any(1)
        ev["finish"][t] = live & ((new & F_FINISHED) != 0).any(1)
        ev["trunc"][t] = trunc
        ev["trunc_unfinished"][t] = trunc & ~fin
        ev["both_crashed"][t] = term & ~fin
        first_crash = (new & F_HAS_CRASHED) != 0
        ev["lone_crash"][t] = live & ~ended & ((first_crash[:, 0] & ~crashed[:, 1]) | (first_crash[:, 1] & ~crashed[:, 0]))
        ev["frozen"][t] = live & crashed0.any(1)
        out["frozen_car"][t] = live[:, None] & crashed0
        ev["contact"][t] = live & touch
        ev["placed_by_finish"][t] = ended & fin
        ev["placed_by_progress"][t] = ended & ~fin
        ep_ret = np.where(pending, 0.0, ep_ret + rew[:, 0])
        ep_len = np.where(pending, 0, ep_len + 1).astype(np.int32)
        stats[0] += float(ep_ret[ended].sum())
        stats[1] += int(ep_len[ended].sum())
        stats[2] += int(ended.sum())
        out["actions"][t], out["obs"][t], out["reward64"][t] = a, obs, rew
        out["terminated"][t], out["truncated"][t], out["reset"][t] = term, trunc, pending
        out["info"][t, :, :, :2] = info
        out["info"][t, :, :, 3] = place
        pending = ended
    final = dict(st, env_flags=pending.astype(np.uint8), ep_return=ep_ret, ep_length=ep_len)
    out["done"] = out["terminated"] | out["truncated"]
    return Case(slots=state0["track"].copy(), state0={k: v.copy() for k, v in state0.items()}, T=T, trace=out,
                events=ev, final=final, stats=tuple(stats), n_agents=2, draw_seed=draw_seed)


def multi_case(golden, oracle, seed=9, n=130, n_slots=4, n_steps=K, draw_seed=77):
    tab = golden.table()
    st, wild, lane = multi_state0(tab, np.arange(n) % n_slots, seed, horizon=n_steps)
    return run_multi(tab, oracle, st, n_steps, draw_seed, wild=wild, lane=lane, seed=seed)


def multi_masks(terminated, truncated, info):
    """The census a two-car run's own outputs give: info rows [T, N, 2, 4] = speed, progress, 0, placement."""
    fin = (info[..., 1] == 1.0).any(2) & terminated
    m = dict(term=terminated, trunc=truncated, finish=fin, both_crashed=terminated & ~fin,
             placed=(info[..., 3] > 0).any(2), car1_first=info[..., 1, 3] == 1.0)
    return {k: v.sum(1).astype(int) for k, v in m.items()}


# ------------------------------------------------------------------------------ one build per session
_BUILDERS = {"single": single_case, "lane": lane_case, "multi": multi_case}
_CACHE = {}


def get(name, golden, oracle):
    """The named case on the device-libm oracle, built once and shared (read only)."""
    assert oracle.device_libm
    if name not in _CACHE:
        _CACHE[name] = _BUILDERS[name](golden, oracle)
    return _CACHE[name]
