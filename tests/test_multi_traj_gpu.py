"""Two-car episodes, the two-car evaluation and SelfPlayWrapper on the device, against the
reference (tests/golden/traj_multi.npz, eval_multi.npz; gen_golden.py) and against the
device-libm oracle.

Episodes.  One env per recorded episode, reset through numpy start draws after seeding
np.random so that the recorded start orders come out, then the recorded actions replayed open
loop (an ended env is fed zeros, as test_single_trajectories_vs_golden does).  Every live step
is compared with the reference -- terminated, truncated, every flag (crashed, finished,
has_crashed, the three checkpoints), progress, finished_step and placement exact, obs and
reward64 within 1e-5, the reset observations bit for bit -- and with the oracle's replay
(tests/multi_traj_cases.replay, computed once per module) bit for bit: obs, reward64,
terminated, truncated, info and the whole f64 state, at every step.  Launch forms: the
one-kernel step, the split step, the automatic choice at this N (split, 4 lanes per ray, a
REWARD lane per car), one lane per ray and env, 2 lanes per ray, lane_cars=1 (the wide
kernels and wide_n are single-agent: resolve_schedule takes them for A == 1 only), and
steps_device in calls of 7 and 24 steps (a two-car handle runs rx_steps as K single steps --
the paired and deep schedules are single-agent -- so these check its [K, ...] row strides: obs,
float32 reward and done row by row, the env's own rows and the state after every call).
Every form accepts autoreset="disabled".  Once more with every episode replicated 420 times
(2,100 envs: culled ray waves of many envs per slot with the spatial re-sort; start positions
injected, since 2,100 orders cannot be seeded): replicas equal one another bit for bit at
every step, replica 0 compared as above.

Evaluation.  MultiEvaluator.run_actions (fused) on eval_multi.npz's actions, numpy start
draws seeded with the fixture's seed: steps, finished, crashed, placement exact, progress /
speed / distance_per_step within 1e-5, total_reward / total_distance within 1e-5 x max(1,
|ref|); the eager loop on the same actions returns the same dictionaries exactly; the
max_steps=40 call gives placement None.

Wrapper.  rx.envs.SelfPlayWrapper(MultiRacingEnv, agent_idx) for agent_idx 0 and 1 over the
recorded wrapper rows, the opponent a module replaying the other car's actions; the start
order comes from numpy start draws switched on on the env's private vector env (the
single-env classes do not expose the draws).

Measured on an MI355X (printed by the tests): worst |obs/reward - reference| over the 4,536
trajectory steps 1.42e-14; worst evaluation metric deviation 3.55e-15.
"""
import numpy as np
import pytest
import torch

from tests import multi_traj_cases as mtc
from tests.golden_util import load

pytestmark = pytest.mark.gpu

OBS_TOL = 1e-5
STATE = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering")
REPS = 420


@pytest.fixture(scope="module")
def tm():
    if not torch.cuda.is_available():
        pytest.fail("gpu test without a HIP device")
    return load("traj_multi.npz")


@pytest.fixture(scope="module")
def em():
    return load("eval_multi.npz")


@pytest.fixture(scope="module")
def ref_dev(tm, golden, oracle_dev):
    """The device-libm oracle's replay of every episode: (reset, rows, off), shared and read-only."""
    out = mtc.replay(oracle_dev, golden.table(), tm["slot"], tm["order"], tm["actions"], tm["off"])
    for d in out[:2]:
        for a in d.values():
            a.setflags(write=False)
    return out


def _seed_for(orders):
    """A seed whose stream of np.random.shuffle([0, 1]) calls starts with ``orders``."""
    for s in range(1 << 16):
        st = np.random.RandomState(s)
        got = []
        for _ in orders:
            o = [0, 1]
            st.shuffle(o)
            got.append(o[0])
        if got == [int(x) for x in orders]:
            return s
    raise AssertionError("no seed found")


def _venv(golden, slots, **kw):
    from rx.track import DEFAULT_CONTROL_POINTS
    from rx.vector_env import RacingVectorEnv
    cps = [DEFAULT_CONTROL_POINTS if golden.tracks[k]["label"] == "default" else golden.tracks[k]["cp"] for k in slots]
    ws = [golden.tracks[k]["width"] for k in slots]
    return RacingVectorEnv(cps, ws, n_agents=2, device="cuda", autoreset="disabled", **kw)


def _padded_actions(actions, off, n=None):
    """[T, E, 2, 2]: episode e's actions in column e, zeros after its end."""
    L = np.diff(off)
    n = len(L) if n is None else n
    a = np.zeros((int(L.max()), n, 2, 2), np.float32)
    for e in range(len(L)):
        a[:L[e], e] = actions[off[e]:off[e + 1]]
    return a


def _play(v, tm, reps=1, K=1):
    """Replay the fixture's actions on ``v`` (E x reps envs, env r * E + e = replica r of episode
    e); returns replica 0's rows [T, E, ...] as numpy arrays, ``full`` [T] (the steps whose
    reward64 / masks / info / state rows were read: all of them for K = 1, the last of every
    steps_device call otherwise) and, for reps > 1, whether all replicas stayed equal."""
    E = len(tm["slot"])
    N = E * reps
    assert v.num_envs == N
    dev = v.device
    A = torch.from_numpy(_padded_actions(tm["actions"], tm["off"])).to(dev)
    T = A.shape[0]
    D = v.D
    rec = dict(obs=torch.zeros((T, E, 2, D), dtype=torch.float32, device=dev),
               reward=torch.zeros((T, E, 2), dtype=torch.float32, device=dev),
               done=torch.zeros((T, E), dtype=torch.float32, device=dev),
               reward64=torch.zeros((T, E, 2), dtype=torch.float64, device=dev),
               terminated=torch.zeros((T, E), dtype=torch.uint8, device=dev),
               truncated=torch.zeros((T, E), dtype=torch.uint8, device=dev),
               info=torch.zeros((T, E, 2, 4), dtype=torch.float64, device=dev),
               flags=torch.zeros((T, E, 2), dtype=torch.uint8, device=dev),
               finished_step=torch.zeros((T, E, 2), dtype=torch.int32, device=dev),
               steps=torch.zeros((T, E), dtype=torch.int32, device=dev))
    for k in STATE:
        rec[k] = torch.zeros((T, E, 2), dtype=torch.float64, device=dev)
    full = np.zeros(T, bool)
    same = torch.ones((), dtype=torch.bool, device=dev)

    def read_full(t):
        nonlocal same
        b, st = v.buf, v.state
        rows = dict(reward64=b["reward64"], terminated=b["terminated"], truncated=b["truncated"], info=b["info"],
                    flags=st["flags"].view(N, 2), finished_step=st["finished_step"].view(N, 2), steps=st["steps"])
        for k in STATE:
            rows[k] = st[k].view(N, 2)
        for k, r in rows.items():
            rec[k][t].copy_(r[:E])
            if reps > 1:
                same = same & (r.view(reps, -1) == r[:E].reshape(1, -1)).all()
        full[t] = True

    if K == 1:
        for t in range(T):
            a = A[t] if reps == 1 else A[t].repeat(reps, 1, 1)
            obs, rew, done = v.step_device(a, full_info=True)
            rec["obs"][t].copy_(obs[:E])
            rec["reward"][t].copy_(rew[:E])
            rec["done"][t].copy_(done[:E])
            if reps > 1:
                same = same & (obs.view(reps, -1) == obs[:E].reshape(1, -1)).all()
            read_full(t)
    else:
        ob = torch.zeros((K, N, 2, D), dtype=torch.float32, device=dev)
        rw = torch.zeros((K, N, 2), dtype=torch.float32, device=dev)
        dn = torch.zeros((K, N), dtype=torch.float32, device=dev)
        for t0 in range(0, T, K):
            k = min(K, T - t0)
            v.steps_device(A[t0:t0 + k].contiguous(), obs_out=ob[:k], reward_out=rw[:k], done_out=dn[:k],
                           full_info=True)
            rec["obs"][t0:t0 + k].copy_(ob[:k])
            rec["reward"][t0:t0 + k].copy_(rw[:k])
            rec["done"][t0:t0 + k].copy_(dn[:k])
            read_full(t0 + k - 1)
    out = {k: r.cpu().numpy() for k, r in rec.items()}
    return out, full, bool(same.item())


def _compare(rec, full, tm, ref_dev, tag):
    """Every live step against the reference and against the oracle's replay; returns the
    worst |obs / reward - reference|."""
    _, rows, off = ref_dev
    worst = 0.0
    flags = mtc.flags_of(tm)
    for e in range(len(tm["slot"])):
        a, b = int(off[e]), int(off[e + 1])
        n = b - a
        g = {k: r[:n, e] for k, r in rec.items()}
        f = full[:n]
        at = (tag, e)
        # --- the reference: masks exact, floats within tolerance
        assert np.array_equal(g["done"] != 0, tm["done_all"][a:b]), at
        assert np.array_equal(g["terminated"][f] != 0, tm["done"][a:b][f]), at
        assert np.array_equal(g["truncated"][f] != 0, tm["truncated"][a:b][f]), at
        assert np.array_equal(g["flags"][f], flags[a:b][f]), at
        assert np.array_equal(g["progress"][f], tm["progress"][a:b][f]), at
        assert np.array_equal(g["finished_step"][f], tm["finished_step"][a:b][f]), at
        assert np.array_equal(g["steps"][f], tm["steps"][a:b][f]), at
        assert np.array_equal(g["info"][f][..., 3].astype(np.int64), tm["placement"][a:b][f].astype(np.int64)), at
        assert np.array_equal(g["info"][f][..., 1], tm["info_progress"][a:b][f]), at
        d_obs = float(np.abs(g["obs"] - tm["obs"][a:b]).max())
        d_rew = float(np.abs(g["reward64"][f] - tm["reward"][a:b][f]).max())
        d_r32 = float(np.abs(g["reward"] - tm["reward"][a:b].astype(np.float32)).max())
        assert d_obs <= OBS_TOL and d_rew <= OBS_TOL and d_r32 <= OBS_TOL, (at, d_obs, d_rew, d_r32)
        worst = max(worst, d_obs, d_rew)
        # --- the device-libm oracle: bit for bit
        assert np.array_equal(g["obs"], rows["obs"][a:b]), at
        assert np.array_equal(g["reward"], rows["reward"][a:b].astype(np.float32)), at
        assert np.array_equal(g["reward64"][f], rows["reward"][a:b][f]), at
        assert np.array_equal(g["terminated"][f] != 0, rows["done"][a:b][f]), at
        assert np.array_equal(g["truncated"][f] != 0, rows["truncated"][a:b][f]), at
        assert np.array_equal(g["info"][f][..., 0], rows["info_speed"][a:b][f]), at
        assert np.array_equal(g["info"][f][..., 1], rows["info_progress"][a:b][f]), at
        assert np.array_equal(g["info"][f][..., 3].astype(np.int32), rows["placement"][a:b][f]), at
        for k in STATE + ("flags", "finished_step", "steps"):
            assert np.array_equal(g[k][f], rows[k][a:b][f]), (at, k)
        assert full[n - 1] or tag.startswith("steps"), at
    return worst


FORMS = {
    "one_kernel": dict(sched=dict(split=-1)),
    "split": dict(sched=dict(split=1)),
    "auto": dict(),
    "one_lane": dict(sched=dict(ray_lpr=1, reward_lpe=1, wide_n=-1)),
    "two_lanes_per_ray": dict(sched=dict(ray_lpr=2, reward_lpe=2)),
    "lane_cars": dict(lane_cars=1),
    "steps7": dict(K=7),
    "steps24": dict(K=24),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_two_car_episodes_vs_reference_and_oracle(tm, golden, ref_dev, form):
    kw = dict(FORMS[form])
    K = kw.pop("K", 1)
    v = _venv(golden, tm["slot"], **kw)
    s = v.schedule()
    assert s["wide"] == 0, s  # the wide kernels are single-agent (resolve_schedule: A == 1)
    if form in ("one_kernel", "split"):
        assert s["split"] == int(form == "split"), s
    elif form == "auto":  # what a small two-car env runs unasked: split, 4 lanes per ray, a lane per car
        assert (s["split"], s["ray_lpr"], s["reward_lpe"]) == (1, 4, 2), s
    elif form == "one_lane":
        assert (s["ray_lpr"], s["reward_lpe"]) == (1, 1), s
    elif form == "two_lanes_per_ray":
        assert (s["ray_lpr"], s["reward_lpe"]) == (2, 2), s
    elif form == "lane_cars":
        assert s["lane_tracks"] == 1, s
    v.use_numpy_start_draws()
    np.random.seed(_seed_for(tm["order"]))
    obs0 = v.reset_device().cpu().numpy()
    v.use_numpy_start_draws(False)  # autoreset is off: no further reset, and no per-step draw session
    assert np.array_equal(obs0, tm["reset_obs"])  # reset observations: bit for bit
    assert np.array_equal(obs0, ref_dev[0]["obs"])
    g = v.get_state()
    for k in ("x", "y", "angle"):
        assert np.array_equal(g[k].reshape(-1, 2), tm["reset_" + k]), k
    rec, full, _ = _play(v, tm, K=K)
    worst = _compare(rec, full, tm, ref_dev, form)
    print(f"\n{form}: max |obs/reward - reference| over {len(tm['steps'])} two-car trajectory steps: {worst:.3g}")
    assert worst <= OBS_TOL
    v.close()


def test_two_car_episodes_replicated_on_the_culled_sorted_path(tm, golden, ref_dev):
    E = len(tm["slot"])
    N = E * REPS
    assert N >= 2100
    v = _venv(golden, list(tm["slot"]) * REPS, seed=3)
    s = v.schedule()  # the schedule of a large two-car env: one lane per ray, the spatial re-sort on
    assert s["split"] == 1 and s["lane_tracks"] == 0 and v.sort_interval > 0 and v.env_order()[1] > 0, s
    v.reset_device()
    # the start order of 2,100 envs cannot be seeded: every replica takes the recorded reset positions
    v.set_state(x=np.tile(tm["reset_x"], (REPS, 1)), y=np.tile(tm["reset_y"], (REPS, 1)))
    rec, full, same = _play(v, tm, reps=REPS)
    assert same, "replicas of one episode differ"
    worst = _compare(rec, full, tm, ref_dev, "replicated")
    print(f"\nreplicated x{REPS}: max |obs/reward - reference|: {worst:.3g}")
    v.close()


# ----------------------------------------------------------------- evaluation
class _Replay(torch.nn.Module):
    """Both cars' recorded actions, step by step: MultiEvaluator.run's agent ([2N, D] -> [2N, 2])."""

    def __init__(self, actions):
        super().__init__()
        self.a, self.t = actions, 0

    def get_action_and_value(self, obs):
        a = self.a[min(self.t, len(self.a) - 1)].reshape(-1, 2)
        self.t += 1
        return a.clone(), None, None, None


def test_multi_evaluator_vs_reference(em):
    from rx.evaluate import MultiEvaluator
    S = int(em["seed"])
    A = torch.from_numpy(_padded_actions(em["actions"], em["off"][:9])).cuda()
    ev = MultiEvaluator(num_tracks=4, num_runs=2, device="cuda", backend="fused")
    assert [tuple(i) for i in ev.ids] == [(t, r) for t in range(4) for r in range(2)]
    ev.venv.use_numpy_start_draws()
    np.random.seed(S)
    eps = ev.run_actions(A)["all_episodes"]
    worst = 0.0
    for i in range(8):
        worst = max(worst, mtc.assert_metrics(eps[i], mtc.eval_record(em, i), i))
    # the ninth recorded call: the first episode again, max_steps=40, on the seed's ninth draw --
    # which this second reset hands to env 0
    A40 = torch.zeros((40, 8, 2, 2), dtype=torch.float32, device="cuda")
    A40[:, 0] = torch.from_numpy(em["actions"][em["off"][8]:em["off"][9]]).cuda()
    short = ev.run_actions(A40, max_steps=40)["all_episodes"]
    ref = mtc.eval_record(em, 8)
    assert short[0]["placement"] is None and ref["placement"] is None and short[0]["steps"] == 40
    worst = max(worst, mtc.assert_metrics(short[0], ref, 8))
    print(f"\nworst evaluation metric deviation from the reference: {worst:.3g}")
    ev.close()
    # the eager loop on the same actions and start orders: the same dictionaries exactly
    eg = MultiEvaluator(num_tracks=4, num_runs=2, device="cuda", backend="eager")
    eg.venv.use_numpy_start_draws()
    np.random.seed(S)
    eager = eg.run(_Replay(A))["all_episodes"]
    assert eager == eps
    with pytest.raises(ValueError):
        eg.run_actions(A)  # open-loop replay is the fused backend's
    eg.close()


# ----------------------------------------------------------------- wrapper
class _Opponent(torch.nn.Module):
    """Replays the other car's recorded actions; SelfPlayWrapper asks it for parameters()."""

    def __init__(self, rows):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.rows, self.t = torch.from_numpy(np.ascontiguousarray(rows)), 0

    def get_action_and_value(self, obs):
        a = self.rows[self.t][None].clone()
        self.t += 1
        return a, None, None, None


@pytest.mark.parametrize("agent_idx", [0, 1])
def test_selfplay_wrapper_vs_reference(tm, golden, agent_idx):
    from rx.envs import MultiRacingEnv, SelfPlayWrapper
    worst = 0.0
    for e, n in zip(tm["wrap_episode"], tm["wrap_len"]):
        e, n = int(e), int(n)
        a = int(tm["off"][e])
        tr = golden.tracks[int(tm["slot"][e])]
        env = MultiRacingEnv(num_agents=2, num_sensors=11) if tr["label"] == "default" else \
            MultiRacingEnv(num_agents=2, num_sensors=11, track_pool=[tr["cp"]], track_id=0, track_width=[tr["width"]])
        w = SelfPlayWrapper(env, agent_idx=agent_idx)
        w.set_opponent(_Opponent(tm["actions"][a:a + n, 1 - agent_idx]))
        env._vec().use_numpy_start_draws()
        np.random.seed(_seed_for([tm["order"][e]]))
        obs, _ = w.reset()
        assert np.array_equal(obs, tm["reset_obs"][e][agent_idx])
        for t in range(n):
            obs, rew, done, trunc, info = w.step(tm["actions"][a + t, agent_idx])
            assert bool(done) == bool(tm["done_all"][a + t]) and bool(trunc) == bool(tm["truncated"][a + t]), (e, t)
            d = max(float(np.abs(obs - tm["obs"][a + t, agent_idx]).max()), abs(rew - tm["reward"][a + t, agent_idx]))
            assert d <= OBS_TOL, (e, t, d)
            worst = max(worst, d)
        if n == tm["off"][e + 1] - a:  # a whole episode: the wrapper's info carries the placement
            assert info["placement"] == int(tm["placement"][a + n - 1, agent_idx])
        w.env.close()
    print(f"\nwrapper agent_idx {agent_idx}: max |obs/reward - reference| {worst:.3g}")
