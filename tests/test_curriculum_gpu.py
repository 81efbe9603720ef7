"""The track curriculum on the GPU: each kernel (csrc/rx_curriculum.hip) against its
host twin bit for bit, rx_track_rollout_steps against rx_rollout_steps and the
per-step eager path, and CurriculumPPO's resampling.

Every device output buffer carries a guard element past its end.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.test_curriculum_cpu import make_tally, py_tally, tally_case, track_io

pytestmark = pytest.mark.gpu

GUARD = -77
NAMES = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- 1. kernels == host twins
@pytest.mark.parametrize("mode", ["one_slot", "distinct", "none", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_tally_kernel_equals_host_twin(L, n, mode):
    """one_slot: every env ended on ONE slot (full contention: the sums must be exact); distinct: every
    lane of a wave on a different slot (67 slots); none: no env ended, the tally stays untouched;
    random: out-of-range slots, finishes, crashes and timeouts mixed."""
    from rx import _lib
    n_tracks = 67
    track, done, terminated, info = tally_case(n, n_tracks, 100 + n, mode)
    start = np.random.RandomState(n).randint(0, 1000, size=(n_tracks + 1, 4)).astype(np.int64)
    want = start.copy()
    q = _lib.ptr
    tc = track_io(_lib, n_tracks, track=track, tally=want)
    assert L.rx_track_tally_host(ctypes.byref(tc), n, q(done), q(terminated), q(info), None) == 0
    if n <= 65:  # the twin itself against the restatement at the small sizes
        ref = start.copy()
        py_tally(ref[:n_tracks], track, done, terminated, info)
        assert np.array_equal(want, ref)
    d = {k: _dev(v) for k, v in dict(track=track, tally=start, done=done, terminated=terminated, info=info).items()}
    tcd = track_io(_lib, n_tracks, track=d["track"], tally=d["tally"])
    _lib.check(L.rx_track_tally(ctypes.byref(tcd), n, q(d["done"]), q(d["terminated"]), q(d["info"]),
                                _lib.stream_ptr()), "rx_track_tally")
    got = d["tally"].cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[n_tracks], start[n_tracks]), "guard row"
    if mode == "none":
        assert np.array_equal(got, start)
    if mode == "one_slot":
        k = n_tracks // 2
        assert got[k, 0] - start[k, 0] == n and np.array_equal(np.delete(got, k, 0), np.delete(start, k, 0))
        assert got[k, 1] - start[k, 1] == int((info[:, 1] == 1.0).sum())


def _chunk():
    from rx import _lib
    return _lib.RX_TRACK_SCORES_CHUNK


SCORE_SIZES = [1, 2, 63, 64, 65, "C-1", "C", "C+1", 70001]
RULES = [(0, 0), (0, 1), (0, 4), (1, 1), (1, 4)]  # (score, power)


@pytest.mark.parametrize("size", SCORE_SIZES)
def test_scores_and_draw_kernels_equal_host_twins(L, size):
    """k_track_scores at one lane, around a wave, around the chunk C and over several chunks plus a
    remainder, both score modes, powers 0, 1 and 4, on random tallies with zero-weight slots and on a
    table that is all zero weights (F == 0); then k_track_draw on every one of those tables at 65 and
    4,097 envs, mix 0 and 0.1."""
    from rx import _lib
    C = _chunk()
    n = {"C-1": C - 1, "C": C, "C+1": C + 1}.get(size, size)
    q = _lib.ptr
    seed = 0xC0FFEE1234567
    for kind, rules in (("mixed", RULES), ("mastered", [(0, 4), (1, 1)]), ("fresh", [(0, 1)])):
        tally = make_tally(kind, n, seed=n)
        if kind == "mixed" and n > 200:  # a run of zero-weight slots across a wave boundary
            tally[60:70] = (1000, 1000, 0, 0)
        tally_d = _dev(tally)
        for score, power in rules:
            cdf, p = np.zeros(n, dtype=np.int64), np.zeros(n)
            tc = track_io(_lib, n, score=score, tally=tally, cdf=cdf, p=p)
            assert L.rx_track_scores_host(ctypes.byref(tc), power, 1.0, None) == 0
            cdf_d = torch.full((n + 1,), GUARD, dtype=torch.int64, device="cuda")
            p_d = torch.full((n + 1,), float(GUARD), dtype=torch.float64, device="cuda")
            tcd = track_io(_lib, n, score=score, tally=tally_d, cdf=cdf_d, p=p_d)
            _lib.check(L.rx_track_scores(ctypes.byref(tcd), power, 1.0, _lib.stream_ptr()), "rx_track_scores")
            got_cdf, got_p = cdf_d.cpu().numpy(), p_d.cpu().numpy()
            assert np.array_equal(got_cdf[:n], cdf), (kind, score, power)
            assert np.array_equal(got_p[:n], p), (kind, score, power)
            assert got_cdf[n] == GUARD and got_p[n] == GUARD
            if kind == "mastered" and score == 0:
                assert cdf[-1] == 0
            for n_envs in (65, 4097):
                for mix in (0.0, 0.1):
                    want = np.zeros(n_envs, dtype=np.int32)
                    th = track_io(_lib, n, cdf=cdf, track_of_env=want, seed=seed)
                    assert L.rx_track_draw_host(ctypes.byref(th), n_envs, 3, mix, None) == 0
                    out = torch.full((n_envs + 1,), GUARD, dtype=torch.int32, device="cuda")
                    td = track_io(_lib, n, cdf=cdf_d, track_of_env=out, seed=seed)
                    _lib.check(L.rx_track_draw(ctypes.byref(td), n_envs, 3, mix, _lib.stream_ptr()), "rx_track_draw")
                    got = out.cpu().numpy()
                    assert np.array_equal(got[:n_envs], want), (kind, score, power, n_envs, mix)
                    assert got[n_envs] == GUARD and want.min() >= 0 and want.max() < n


# ---------------------------------------------------------------- 2. rx_track_rollout_steps
def _pool(n_tracks, seed):
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    return gen_tracks(n_tracks, seed=None, rng=rng), [int(rng.randint(6, 10)) for _ in range(n_tracks)]


def _agent():
    from rx.agent import Agent
    from rx.optim import FlatAdam
    from rx.spaces import Box
    torch.manual_seed(9)
    ag = Agent(Box(-1, 1, (15,)), Box(-1, 1, (2,))).cuda()
    with torch.no_grad():
        ag.log_std.fill_(-0.3)
    return ag, FlatAdam(ag, torch.optim.Adam(ag.parameters(), lr=1e-3, eps=1e-5), 0.5)


@pytest.mark.parametrize("n_tracks,sched,lane_tracks", [(8, None, 0), (64, dict(wide_n=-1, dyn_lpe=1), 1)])
def test_track_rollout_steps_equals_rollout_steps_and_the_eager_tally(L, n_tracks, sched, lane_tracks):
    """64 envs x 32 steps with max_steps = 12: every env ends at least two episodes by truncation.
    From the same state with the same noise: rx_track_rollout_steps' outputs are rx_rollout_steps' bit
    for bit; its tally is the per-step eager path's (rx_policy_act, step_device with the info rows,
    tally_step) and a host count of the downloaded done / terminated / info rows.  Once on 8 tracks
    (slot-uniform waves) and once on 64 distinct tracks with the lane-varying schedule."""
    from rx import _lib
    from rx.curriculum import CurriculumStepRollout, TrackCurriculum
    from rx.ppo_fused import StepRollout
    from rx.vector_env import RacingVectorEnv
    N, T = 64, 32
    pool, widths = _pool(n_tracks, 5)
    cps, ws = [pool[i % n_tracks] for i in range(N)], [widths[i % n_tracks] for i in range(N)]
    ag, fl = _agent()
    g = torch.Generator(device="cuda").manual_seed(6)
    eps = torch.randn((T, N, 2), device="cuda", generator=g) * 1.5
    outs, tallies = [], []
    host = np.zeros((n_tracks, 4), dtype=np.int64)
    for path in ("track", "plain", "eager"):
        venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=12, sched=sched)
        assert venv.schedule()["lane_tracks"] == lane_tracks and len(venv.tracks) == n_tracks
        cur = TrackCurriculum(venv, seed=3)
        obs = torch.zeros((T, N, 15), device="cuda")
        actions = torch.zeros((T, N, 2), device="cuda")
        logprobs, dones, rewards, values = (torch.zeros((T, N), device="cuda") for _ in range(4))
        nobs = venv.reset_device().clone()
        nd = torch.zeros(N, device="cuda")
        obs[0].copy_(nobs)
        dones[0].copy_(nd)
        bufs = (obs, actions, logprobs, dones, rewards, values, nobs, nd)
        if path == "track":
            CurriculumStepRollout(ag, fl, venv, T, cur)(*bufs, eps=eps)
        elif path == "plain":
            StepRollout(ag, fl, venv, T)(*bufs, eps=eps)
        else:
            track = venv.track_of_env.copy()
            for s in range(T):
                io = _lib.RxPolicyIO(15, N, _lib.ptr(obs[s]), _lib.ptr(eps[s]), _lib.ptr(fl.flat_param),
                                     _lib.ptr(ag.log_std), _lib.ptr(actions[s]), _lib.ptr(logprobs[s]),
                                     _lib.ptr(values[s]), 0, 0)
                _lib.check(L.rx_policy_act(io, _lib.stream_ptr()), "rx_policy_act")
                last = s + 1 == T
                _, _, d = venv.step_device(actions[s], obs_out=nobs if last else obs[s + 1], reward_out=rewards[s],
                                           done_out=nd if last else dones[s + 1], full_info=True)
                cur.tally_step(d)
                py_tally(host, track, d.cpu().numpy(), venv.buf["terminated"].cpu().numpy(),
                         venv.buf["info"].cpu().numpy().reshape(N, 4))
        torch.cuda.synchronize()
        outs.append([x.clone() for x in bufs])
        tallies.append(cur.tally.cpu().numpy())
        assert np.array_equal(venv._st["track"].cpu().numpy(), venv.track_of_env)
        venv.close()
    for k, a, b, c in zip(NAMES, *outs):
        assert torch.equal(a, b), k
        assert torch.equal(a, c), k
    t_track, t_plain, t_eager = tallies
    assert not t_plain.any()  # rx_rollout_steps tallies nothing
    assert np.array_equal(t_track, t_eager) and np.array_equal(t_track, host)
    assert t_track[:, 0].sum() >= 2 * N and (t_track[:, 0] > 0).all()
    assert t_track[:, 0].sum() == int(outs[0][3].sum().item() + outs[0][7].sum().item())  # one per done flag
    assert (t_track[:, 1] == 0).all() and (t_track[:, 2] <= t_track[:, 0]).all() and (t_track[:, 3] >= 0).all()


# ---------------------------------------------------------------- 3. CurriculumPPO
def _train(updates=3, **over):
    """tests/test_cull_tables_gpu.py's _train on CurriculumPPO: 64 envs x 16 steps on a pool of 8
    tracks, max_steps = 12 -> (trainer, np.random state after, per-rollout obs buffers, what every
    resample left: (generation, tally, bound track array, retired slots, the control points before))."""
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.ppo import build_vector_env

    class ShortEpisodes(CurriculumPPO):
        def _make_envs(self, env_fn):
            c = self.config
            return build_vector_env(env_fn, c["num_envs"], c["seed"], self.device, max_steps=12)

    config = base_config(num_envs=64, num_steps=16, kl_target=1e9, **over)
    config["total_timesteps"] = updates * config["batch_size"]
    random.seed(config["seed"])
    np.random.seed(config["seed"])
    torch.manual_seed(config["seed"])
    pool, widths = _pool(8, 21)
    t = ShortEpisodes(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 8, track_width=widths[i % 8]),
                      config, device="cuda")
    rollouts, swaps, collect, resample = [], [], t.collect_rollout, t.resample_tracks

    def recording(*a):
        out = collect(*a)
        rollouts.append(out[0].clone())
        return out

    def swapping(*a):
        before = list(t._cps)
        out = resample(*a)
        swaps.append((t.envs.track_generation, t.curriculum.tally.cpu().numpy(), t.envs._st["track"].cpu().numpy(),
                      list(t.retired[-1]), before))
        return out

    t.collect_rollout, t.resample_tracks = recording, swapping
    done = [u for u, _, _, _ in t.train_iter()]
    assert done == list(range(updates))
    return t, np.random.get_state(), rollouts, swaps


@pytest.fixture(scope="module")
def trained():
    return _train(track_resample_every=1, curriculum_mastery=0.0, curriculum_min_episodes=1)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_curriculum_ppo_redraws_from_the_tallies(L, trained):
    from rx import _lib
    t, _, rollouts, swaps = trained
    cur = t.curriculum
    assert t.envs.track_generation == 2 and len(swaps) == 2 and cur.n_tracks == 8 and len(t.envs._table) == 8
    assert len(rollouts) == 3 and all(torch.isfinite(r).all() for r in rollouts)
    for p in t.agent.parameters():
        assert torch.isfinite(p).all()
    for i, (g, tally, bound, retired, before) in enumerate(swaps):
        assert g == i + 1
        # the assignment is the host twin's draw from the tally the resample left
        cdf, p = np.zeros(8, dtype=np.int64), np.zeros(8)
        want = np.zeros(64, dtype=np.int32)
        tc = track_io(_lib, 8, score=0, tally=tally, cdf=cdf, p=p, track_of_env=want, seed=t.config["seed"])
        assert L.rx_track_scores_host(ctypes.byref(tc), 1, 1.0, None) == 0
        assert L.rx_track_draw_host(ctypes.byref(tc), 64, g, 0.1, None) == 0
        assert np.array_equal(bound, want)
        # mastery 0.0, one episode enough: exactly floor(0.25 * 8) slots retired, zeroed, on new tracks
        assert len(retired) == 2 and len(set(retired)) == 2
        assert not tally[retired].any() and tally[:, 0].sum() > 0
        for k in range(8):
            now = t._cps[k] if i == 1 else swaps[1][4][k]  # the control points right after swap i
            assert (k in retired) != np.array_equal(np.asarray(before[k]), np.asarray(now)), k
    assert not np.array_equal(swaps[0][2], swaps[1][2]), "a new generation must give a new assignment"
    tab = t.track_table()
    assert tab["episodes"].sum() >= 64 and abs(tab["prob"].sum() - 1.0) < 1e-12
    assert np.array_equal(tab["episodes"], cur.tally[:, 0].cpu().numpy())


def test_curriculum_ppo_leaves_np_random_alone_and_is_deterministic(trained):
    t, state, rollouts, _ = trained
    t0, state0, _, swaps0 = _train(track_resample_every=0)
    assert t0.envs.track_generation == 0 and not swaps0
    assert t0.curriculum.tally[:, 0].sum().item() >= 3 * 64, "with no resampling the trainer still tallies"
    assert _same_state(state, state0), "a curriculum resample moved the global numpy stream"
    t2, state2, rollouts2, _ = _train(track_resample_every=1, curriculum_mastery=0.0, curriculum_min_episodes=1)
    assert _same_state(state, state2)
    for a, b in zip(t.agent.parameters(), t2.agent.parameters()):
        assert torch.equal(a, b)
    assert torch.equal(t.curriculum.tally, t2.curriculum.tally)
    assert all(torch.equal(a, b) for a, b in zip(rollouts, rollouts2))


def test_curriculum_ppo_graph_rollout_equals_eager(trained):
    t, _, eager, swaps = trained
    tg, _, graph, swaps_g = _train(track_resample_every=1, curriculum_mastery=0.0, curriculum_min_episodes=1,
                                   graph_rollout=True)
    assert tg.envs.track_generation == 2
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    for a, b in zip(swaps, swaps_g):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert torch.equal(t.curriculum.tally, tg.curriculum.tally)
