"""The track curriculum for self-play on the device: k_track_tally2 and the duel scores
against their host twins, rx_track_duel_rollout_steps against rx_selfplay_rollout_steps and
rx_league_rollout_steps (outputs bit for bit) and against a step-by-step composition that
records every terminal row (tallies), track swaps on two-car envs, and the two trainers.

No tolerance anywhere: every comparison is exact.  Every device output buffer of the kernel
tests carries a guard row / element past its end."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_curriculum_cpu import track_io
from tests.test_track_selfplay_cpu import (C, MODES, duel_io, make_duel_tally, py_tally2, start_tables, tally2_case)

pytestmark = pytest.mark.gpu

DEV = "cuda"
T, N, SLOTS = 32, 64, 8
NAMES = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---- 1. k_track_tally2 == rx_track_tally2_host ----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_tally2_device_equals_host(n, mode):
    from rx import _lib
    L = _lib.load()
    n_tracks = 67
    track, done, terminated, info = tally2_case(n, n_tracks, 31 + n, mode)
    d_track, d_done, d_term, d_info = _dev(track), _dev(done), _dev(terminated), _dev(info)
    q = _lib.ptr
    for agent in (0, 1):
        t0, d0 = start_tables(n_tracks, seed=3 + agent)  # non-zero starting tallies; the last row is the guard
        h_t, h_d = t0.copy(), d0.copy()
        tc, td = track_io(_lib, n_tracks, track=track, tally=h_t), duel_io(_lib, agent, h_d)
        _lib.check(L.rx_track_tally2_host(ctypes.byref(tc), ctypes.byref(td), n, q(done), q(terminated), q(info), None),
                   "host")
        g_t, g_d = _dev(t0), _dev(d0)
        dtc, dtd = track_io(_lib, n_tracks, track=d_track, tally=g_t), duel_io(_lib, agent, g_d)
        for call in range(2):  # the second call adds the same again: integer sums
            _lib.check(L.rx_track_tally2(ctypes.byref(dtc), ctypes.byref(dtd), n, q(d_done), q(d_term), q(d_info),
                                         _lib.stream_ptr(None)), "device")
            torch.cuda.synchronize()
            want_t, want_d = t0 + (call + 1) * (h_t - t0), d0 + (call + 1) * (h_d - d0)
            assert np.array_equal(g_t.cpu().numpy(), want_t), (agent, call)
            assert np.array_equal(g_d.cpu().numpy(), want_d), (agent, call)
        assert np.array_equal(g_t[-1].cpu().numpy(), t0[-1]) and np.array_equal(g_d[-1].cpu().numpy(), d0[-1])
        if mode == "none":
            assert np.array_equal(g_t.cpu().numpy(), t0) and np.array_equal(g_d.cpu().numpy(), d0)
        else:
            assert not np.array_equal(h_t, t0)


# ---- 2. rx_track_duel_scores == its host twin; rx_track_draw on those tables ----------------------
@pytest.mark.parametrize("n_tracks", [1, 63, 64, 65, C - 1, C, C + 1, 70001])
def test_duel_scores_and_draw_device_equal_host(n_tracks):
    from rx import _lib
    L = _lib.load()
    n_envs, seed, mix = 777, 0x0123456789ABCDEF ^ n_tracks, 0.1
    tally, duel = make_duel_tally("mixed", n_tracks, seed=9 + n_tracks)
    d_tally, d_duel = _dev(tally), _dev(duel)
    d_cdf = torch.empty(n_tracks + 1, dtype=torch.int64, device=DEV)
    d_p = torch.empty(n_tracks + 1, dtype=torch.float64, device=DEV)
    d_toe = torch.empty(n_envs + 1, dtype=torch.int32, device=DEV)
    for score, power in ((0, 1), (1, 1), (2, 0), (2, 1), (2, 4), (3, 1), (3, 4)):
        cdf, p, toe = np.zeros(n_tracks, np.int64), np.zeros(n_tracks), np.zeros(n_envs, np.int32)
        htc = track_io(_lib, n_tracks, score=score, tally=tally, cdf=cdf, p=p, track_of_env=toe, seed=seed)
        htd = duel_io(_lib, 0, duel)
        _lib.check(L.rx_track_duel_scores_host(ctypes.byref(htc), ctypes.byref(htd), power, 1.0, None), "host")
        _lib.check(L.rx_track_draw_host(ctypes.byref(htc), n_envs, 3, mix, None), "host draw")
        d_cdf.fill_(-7)
        d_p.fill_(-7.0)
        d_toe.fill_(-7)
        dtc = track_io(_lib, n_tracks, score=score, tally=d_tally, cdf=d_cdf, p=d_p, track_of_env=d_toe, seed=seed)
        dtd = duel_io(_lib, 0, d_duel)
        _lib.check(L.rx_track_duel_scores(ctypes.byref(dtc), ctypes.byref(dtd), power, 1.0, _lib.stream_ptr(None)),
                   "device")
        _lib.check(L.rx_track_draw(ctypes.byref(dtc), n_envs, 3, mix, _lib.stream_ptr(None)), "device draw")
        torch.cuda.synchronize()
        g_cdf, g_p, g_toe = d_cdf.cpu().numpy(), d_p.cpu().numpy(), d_toe.cpu().numpy()
        assert g_cdf[-1] == -7 and g_p[-1] == -7.0 and g_toe[-1] == -7, "a guard element was written"
        assert np.array_equal(g_cdf[:-1], cdf), (score, power)
        assert np.array_equal(g_p[:-1].view(np.uint64), p.view(np.uint64)), (score, power)
        assert np.array_equal(g_toe[:-1], toe), (score, power)
        assert cdf[-1] > 0 and toe.min() >= 0 and toe.max() < n_tracks
    assert torch.equal(d_tally.cpu(), torch.from_numpy(tally)) and torch.equal(d_duel.cpu(), torch.from_numpy(duel))


# ---- shared: two-car envs on 8 slots, agents, buffers, noise ---------------------------------------
def _pool(n, seed):
    import random
    from rx.track import gen_tracks
    state = np.random.get_state()
    random.seed(seed)
    np.random.seed(seed)
    cps = gen_tracks(num_tracks=n, seed=None)
    np.random.set_state(state)
    return cps, [float(6 + k % 4) for k in range(n)]


def _venv(n_envs, slots, seed=9, max_steps=12, pool_seed=51):
    from rx.vector_env import RacingVectorEnv
    cps, widths = _pool(slots, pool_seed)
    return RacingVectorEnv([cps[i % slots] for i in range(n_envs)], [widths[i % slots] for i in range(n_envs)],
                           n_agents=2, device=DEV, seed=seed, max_steps=max_steps)


def _agents(seeds, D=19):
    from rx.agent import Agent
    from rx.spaces import Box
    out = []
    for k, seed in enumerate(seeds):
        torch.manual_seed(seed)
        a = Agent(Box(-1.0, 1.0, shape=(D,), dtype=np.float32), Box(-1.0, 1.0, shape=(2,), dtype=np.float32)).to(DEV)
        with torch.no_grad():
            a.actor_mu[4].weight.mul_(40.0)  # the mean actions depend on the observation
            a.log_std.copy_(torch.tensor([-0.3 - 0.2 * k, -0.5 + 0.15 * k]))
        out.append(a)
    return out


def _bufs():
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    return [z(T, N, 19), z(T, N, 2), z(T, N), z(T, N), z(T, N), z(T, N)]  # obs actions logprobs dones rewards values


def _noise(seed=8):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((T, N, 2), device=DEV, generator=g), torch.randn((T, N, 2), device=DEV, generator=g))


def _start(env, bufs):
    o = env.reset_device()
    bufs[0][0].copy_(o)
    bufs[3][0].zero_()
    return torch.full((N, 19), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)


def _same(a, b, names=NAMES):
    for name, x, y in zip(names, a, b):
        assert not (x.is_floating_point() and torch.isnan(x).any()), name
        assert torch.equal(x, y), name


class _Recorder:
    """The per-step eager path's rows: the device tally after every step, and the same rows downloaded
    for the Python restatement."""

    def __init__(self, cur):
        self.cur = cur
        self.tally = np.zeros((cur.n_tracks, 4), np.int64)
        self.duel = np.zeros((cur.n_tracks, 4), np.int64)
        self.dones = 0

    def step(self, done):
        v = self.cur.venv
        self.cur.tally_step(done)
        h_done = done.cpu().numpy()
        py_tally2(self.tally, self.duel, self.cur.agent_idx, v._st["track"].cpu().numpy(), h_done,
                  v.buf["terminated"].cpu().numpy(), v.buf["info"].cpu().numpy())
        self.dones += int((h_done != 0).sum())


# ---- 3. the self-play rollout ---------------------------------------------------------------------
@pytest.mark.parametrize("agent_idx", [0, 1])
def test_selfplay_rollout_with_the_tally(agent_idx):
    from rx import _lib
    from rx.optim import FlatParams
    from rx.ppo_fused import PolicyAct, SelfPlayStepRollout
    from rx.selfplay import SelfPlayVectorEnv
    from rx.track_selfplay import DuelSelfPlayStepRollout, DuelTrackCurriculum
    P = _lib.RX_PREC_FP32
    learner, opp = _agents((29, 21))
    flat, oflat = FlatParams(learner), FlatParams(opp)
    eps, oeps = _noise()

    def env():
        sp = SelfPlayVectorEnv(_venv(N, SLOTS), agent_idx)
        sp.set_opponent(opp, oflat, P)
        return sp, DuelTrackCurriculum(sp.venv, agent_idx, seed=5)
    # A: the new call
    spa, cura = env()
    assert cura.n_tracks == SLOTS
    ba = _bufs()
    na, da = _start(spa, ba)
    DuelSelfPlayStepRollout(learner, flat, spa, T, cura, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    # B: rx_selfplay_rollout_steps from the same state (same env seed) and noise
    spb, _ = env()
    bb = _bufs()
    nb, db = _start(spb, bb)
    SelfPlayStepRollout(learner, flat, spb, T, P)(*bb, nb, db, eps=eps, opp_eps=oeps)
    torch.cuda.synchronize()
    _same(ba + [na, da], bb + [nb, db])
    assert torch.equal(spa.venv.buf["obs"], spb.venv.buf["obs"])
    # C: step by step with the existing entry points, rx_track_tally2 after every step, every row recorded
    spc, curc = env()
    bc = _bufs()
    nc, dc = _start(spc, bc)
    obs, actions, logprobs, dones, rewards, values = bc
    v = spc.venv
    pa, po = PolicyAct(learner, flat, N, 19, P), PolicyAct(opp, oflat, N, 19, P)
    act = torch.zeros((N, 2, 2), device=DEV)
    rec = _Recorder(curc)
    for t in range(T):
        last = t + 1 == T
        pa(obs[t], actions[t], logprobs[t], values[t], eps=eps[t])
        po(v.buf["obs"][:, 1 - agent_idx], act[:, 1 - agent_idx], eps=oeps[t])
        act[:, agent_idx].copy_(actions[t])
        done = dc if last else dones[t + 1]
        o, r, _ = v.step_device(act, done_out=done, full_info=True)
        (nc if last else obs[t + 1]).copy_(o[:, agent_idx])
        rewards[t].copy_(r[:, agent_idx])
        rec.step(done)
    torch.cuda.synchronize()
    _same(ba + [na, da], bc + [nc, dc])
    ta, du = cura.tally.cpu().numpy(), cura.duel.cpu().numpy()
    assert np.array_equal(ta, curc.tally.cpu().numpy()) and np.array_equal(du, curc.duel.cpu().numpy())
    assert np.array_equal(ta, rec.tally) and np.array_equal(du, rec.duel)
    ended = int((ba[3][1:] != 0).sum()) + int((da != 0).sum())
    assert ta[:, 0].sum() == ended == rec.dones and ended >= 2 * N  # max_steps = 12: every env ended twice
    assert (ta[:, 0] > 0).all() and (du[:, 0] <= ta[:, 0]).all() and 0 < du[:, 0].sum() < ended
    assert du[:, 3].sum() > 0  # timeouts
    tab = cura.table()
    assert np.array_equal(tab["wins"], du[:, 0]) and np.array_equal(tab["episodes"], ta[:, 0])
    assert np.allclose(tab["win_rate"], du[:, 0] / ta[:, 0]) and abs(tab["prob"].sum() - 1.0) < 1e-12
    # the handle's and the agents' refusals need a live handle
    wrong = DuelTrackCurriculum(spa.venv, 1 - agent_idx, seed=5)
    with pytest.raises(_lib.RxError, match="agent"):
        DuelSelfPlayStepRollout(learner, flat, spa, T, wrong, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    from rx.vector_env import RacingVectorEnv
    cps, widths = _pool(2, 3)
    single = RacingVectorEnv(cps, widths, device=DEV)
    r = L_rollout_args(_lib, spa, cura, single)
    assert r == _lib.RX_EINVAL and b"two-car" in _lib.load().rx_last_error()
    for e in (spa, spb, spc, single):
        e.close()


def L_rollout_args(_lib, sp, cur, single):
    """rx_track_duel_rollout_steps on a single-agent handle: refused before any launch."""
    L = _lib.load()
    io, r, s = _lib.RxIO(), _lib.RxRolloutIO(), _lib.RxSelfplayIO()
    return L.rx_track_duel_rollout_steps(single._h, ctypes.byref(io), ctypes.byref(r), ctypes.byref(s), None,
                                         ctypes.byref(cur.tc), ctypes.byref(cur.td), 0, None)


# ---- 4. the league rollout ------------------------------------------------------------------------
def _league_case(bank):
    from rx import _lib
    from rx.league_train import LeagueVectorEnv
    from rx.track_selfplay import DuelTrackCurriculum
    lenv = LeagueVectorEnv(_venv(N, SLOTS), 0, seed=77, pool_size=3, prec=_lib.RX_PREC_FP32)
    for k, a in enumerate(bank):
        lenv.set_slot(k, a)
    lenv.tally[:2].copy_(torch.tensor([[40, 30, 5], [25, 5, 15]]))
    lenv.weights(2, power=2, mix=0.1, prior=1.0)  # two live bank slots
    lenv.draw_all()
    return lenv, DuelTrackCurriculum(lenv.venv, 0, seed=5)


def test_league_rollout_with_the_tally():
    from rx import _lib
    from rx.league_train import LeagueStepRollout
    from rx.optim import FlatParams
    from rx.ppo_fused import PolicyAct
    from rx.track_selfplay import DuelLeagueStepRollout
    L = _lib.load()
    P = _lib.RX_PREC_FP32
    bank = _agents((31, 32))
    learner = _agents((39,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(18)
    la, cura = _league_case(bank)
    assert len(np.unique(la.opp_id.cpu().numpy())) == 2
    ba = _bufs()
    na, da = _start(la, ba)
    DuelLeagueStepRollout(learner, flat, la, T, cura, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    lb, _ = _league_case(bank)
    bb = _bufs()
    nb, db = _start(lb, bb)
    LeagueStepRollout(learner, flat, lb, T, P)(*bb, nb, db, eps=eps, opp_eps=oeps)
    torch.cuda.synchronize()
    league = lambda e: [e.opp_id, e.draw_count, e.tally, e.venv.buf["obs"]]  # noqa: E731
    _same(ba + [na, da] + league(la), bb + [nb, db] + league(lb), NAMES + ("opp_id", "draw_count", "tally", "env_obs"))
    # step by step: the learner, the bank forward, the step, rx_league_draw, rx_track_tally2
    lc, curc = _league_case(bank)
    bc = _bufs()
    nc, dc = _start(lc, bc)
    obs, actions, logprobs, dones, rewards, values = bc
    v = lc.venv
    pa = PolicyAct(learner, flat, N, 19, P)
    act = torch.zeros((N, 2, 2), device=DEV)
    sink = torch.empty((2, N), device=DEV)
    ob1, a1 = v.buf["obs"][:, 1], act[:, 1]
    rec = _Recorder(curc)
    for t in range(T):
        last = t + 1 == T
        pa(obs[t], actions[t], logprobs[t], values[t], eps=eps[t])
        io = _lib.RxPolicyIO(19, N, _lib.view_ptr(ob1), _lib.ptr(oeps[t]), _lib.ptr(lc.params), _lib.ptr(lc.log_std),
                             _lib.view_ptr(a1), _lib.ptr(sink[0]), _lib.ptr(sink[1]), ob1.stride(0), a1.stride(0), P,
                             None, 0)
        b = _lib.RxPolicyBankIO(io, 3, 1, lc.stride, _lib.ptr(lc.opp_id))
        _lib.check(L.rx_policy_act_bank(ctypes.byref(b), _lib.stream_ptr(None)), "rx_policy_act_bank")
        act[:, 0].copy_(actions[t])
        done = dc if last else dones[t + 1]
        o, r, _ = v.step_device(act, done_out=done, full_info=True)
        (nc if last else obs[t + 1]).copy_(o[:, 0])
        rewards[t].copy_(r[:, 0])
        rec.step(done)
        _lib.check(L.rx_league_draw(ctypes.byref(lc.lg), N, _lib.ptr(done), _lib.ptr(v.buf["info"]),
                                    _lib.stream_ptr(None)), "rx_league_draw")
    torch.cuda.synchronize()
    _same(ba + [na, da] + league(la), bc + [nc, dc] + league(lc), NAMES + ("opp_id", "draw_count", "tally", "env_obs"))
    ta, du = cura.tally.cpu().numpy(), cura.duel.cpu().numpy()
    assert np.array_equal(ta, curc.tally.cpu().numpy()) and np.array_equal(du, curc.duel.cpu().numpy())
    assert np.array_equal(ta, rec.tally) and np.array_equal(du, rec.duel)
    ended = int((ba[3][1:] != 0).sum()) + int((da != 0).sum())
    assert ta[:, 0].sum() == ended == rec.dones and ended >= 2 * N
    assert int(la.tally[:, 0].sum()) - 65 == ended  # the league's own tally counted the same episodes
    # the league io's agent must be the track duel io's
    la.lg.agent = 1
    with pytest.raises(_lib.RxError, match="agent"):
        DuelLeagueStepRollout(learner, flat, la, T, cura, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    for e in (la, lb, lc):
        e.close()


def test_league_rollout_graph_replays_tally_like_eager_calls():
    """A captured graph of the call replayed twice leaves what two eager calls leave, bit for bit, and
    both tallied the episodes of both rollouts: twice one call's launches, nothing lost in the capture."""
    from rx import _lib
    from rx.optim import FlatParams
    from rx.track_selfplay import DuelLeagueStepRollout
    bank = _agents((31, 32))
    learner = _agents((49,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(28)
    res = []
    for graphed in (False, True):
        lenv, cur = _league_case(bank)
        bufs = _bufs()
        nobs, nd = _start(lenv, bufs)
        nobs.copy_(bufs[0][0])
        nd.zero_()
        sr = DuelLeagueStepRollout(learner, flat, lenv, T, cur, _lib.RX_PREC_FP32)
        ended = []

        def body():
            bufs[0][0].copy_(nobs)
            bufs[3][0].copy_(nd)
            sr(*bufs, nobs, nd, eps=eps, opp_eps=oeps)
        torch.cuda.synchronize()
        if graphed:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):  # records only: nothing runs
                body()
            assert not cur.tally.any()
            for _ in range(2):
                g.replay()
                torch.cuda.synchronize()
                ended.append(int((bufs[3][1:] != 0).sum()) + int((nd != 0).sum()))
            lenv._launched()
        else:
            for _ in range(2):
                body()
                torch.cuda.synchronize()
                ended.append(int((bufs[3][1:] != 0).sum()) + int((nd != 0).sum()))
        assert int(cur.tally[:, 0].sum()) == sum(ended) and min(ended) >= N
        res.append([x.clone() for x in bufs + [nobs, nd]] + [lenv.opp_id.clone(), lenv.draw_count.clone(),
                                                             lenv.tally.clone(), cur.tally.clone(), cur.duel.clone()])
        lenv.close()
    _same(*res, NAMES + ("opp_id", "draw_count", "league_tally", "tally", "duel"))


# ---- 5. track swaps on two-car envs ---------------------------------------------------------------
def _actions(g, n):
    a = torch.rand((n, 2, 2), device=DEV, generator=g) * 2 - 1
    a[..., 1].abs_()
    return a


def _same_steps(va, vb, n, steps, seed):
    """Obs, rewards, masks and info of both cars, bit for bit, episode ends included."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ends = 0
    for t in range(steps):
        a = _actions(g, n)
        state = np.random.get_state()  # numpy start draws: both envs take the same outputs of np.random
        oa, ra, da = va.step_device(a, full_info=True)
        after = np.random.get_state()
        np.random.set_state(state)
        ob, rb, db = vb.step_device(a, full_info=True)
        assert np.array_equal(after[1], np.random.get_state()[1]) and after[2] == np.random.get_state()[2], t
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        for k in ("terminated", "truncated", "info", "reward64"):
            assert torch.equal(va.buf[k], vb.buf[k]), (t, k)
        ends += int(da.sum())
    return ends


@pytest.mark.parametrize("draws", ["hash", "numpy"])
def test_two_car_track_swaps_equal_a_fresh_env(draws):
    """Env A is built on pool X, stepped, and moved with set_tracks to pool Y under a non-trivial
    assignment; env B is built on Y with that assignment.  The reset count that keys the device
    start-slot draw restarts at rx_assign, so after A's swap (whose reset is its first on the new
    assignment) and ONE reset_device of B both are at the same count; with numpy start draws both take
    their start sides from np.random seeded alike just before.  Then reassign_tracks on A against a
    second fresh env."""
    from rx.track import TrackSet
    from rx.track_device import DeviceTrackTable
    from rx.vector_env import RacingVectorEnv
    n, slots = 96, 5
    kw = dict(n_agents=2, device=DEV, seed=9, max_steps=25)
    xs, xw = _pool(slots, 61)
    ys, yw = _pool(slots, 62)
    rs = np.random.RandomState(4)
    toe = rs.randint(0, slots, size=n).astype(np.int32)
    toe[:slots] = np.arange(slots)[::-1]  # every slot used, not i % n
    assert not np.array_equal(toe, np.arange(n) % slots)
    ts_y = TrackSet.build(ys, yw, backend="native")
    assert len(ts_y) == slots

    def fresh(assign):
        v = RacingVectorEnv([ys[k] for k in assign], [yw[k] for k in assign], track_set=ts_y, **kw)
        if draws == "numpy":
            v.use_numpy_start_draws()
        return v
    va = RacingVectorEnv([xs[i % slots] for i in range(n)], [xw[i % slots] for i in range(n)], **kw)
    if draws == "numpy":
        va.use_numpy_start_draws()
    va.reset_device()
    g = torch.Generator(device=DEV).manual_seed(70)
    for _ in range(30):  # episodes in flight, resets behind it, the re-sort has run
        va.step_device(_actions(g, n))
    vb = fresh(toe)
    assert np.array_equal(vb.track_of_env, toe)
    np.random.seed(123)
    obs_a = va.set_tracks(DeviceTrackTable.from_arrays(ts_y.arrays(), DEV), toe)
    np.random.seed(123)
    obs_b = vb.reset_device()
    assert va.track_generation == 1
    assert torch.equal(obs_a, obs_b) and torch.equal(va.state["track"], vb.state["track"])
    assert _same_steps(va, vb, n, 40, 71) >= n  # max_steps = 25: every env ended
    sa, sb = va.get_state(), vb.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    # reassign_tracks: the same table, another assignment
    toe2 = np.roll(toe, 7)
    vc = fresh(toe2)
    np.random.seed(321)
    obs_a = va.reassign_tracks(toe2)
    np.random.seed(321)
    obs_c = vc.reset_device()
    assert va.track_generation == 2 and np.array_equal(va.track_of_env, toe2)
    assert torch.equal(obs_a, obs_c)
    assert _same_steps(va, vc, n, 40, 72) >= n
    for e in (va, vb, vc):
        e.close()


# ---- 6. the trainers ------------------------------------------------------------------------------
TN, TT, TSLOTS = 128, 16, 6


def _trainers():
    from rx.league_train import LeagueSelfPlayPPO
    from rx.selfplay import SelfPlayPPO, SelfPlayVectorEnv
    from rx.track_selfplay import LeagueCurriculumPPO, SelfPlayCurriculumPPO

    def venv(self):
        v = _venv(self.config["num_envs"], TSLOTS, seed=self.config["seed"], max_steps=6, pool_seed=81)
        v.reset_device()
        return v

    def sp_envs(self, env_fn):
        return SelfPlayVectorEnv(venv(self), 0, seed=self.config["seed"])

    def lg_venv(self, env_fn):
        return venv(self)
    return {"selfplay": (type("SP", (SelfPlayPPO,), {"_make_envs": sp_envs}),
                         type("SPC", (SelfPlayCurriculumPPO,), {"_make_envs": sp_envs})),
            "league": (type("LG", (LeagueSelfPlayPPO,), {"_make_venv": lg_venv}),
                       type("LGC", (LeagueCurriculumPPO,), {"_make_venv": lg_venv}))}


def _cfg(n_upd=3, **over):
    from rx.configs import self_play_config
    cfg = self_play_config(num_envs=TN, num_steps=TT, snapshot_freq=1, pool_size=3, checkpoint=False,
                           num_minibatches=4, **over)
    cfg["total_timesteps"] = n_upd * cfg["batch_size"]
    return cfg


def _run(cls, cfg, stop_after=None):
    torch.manual_seed(1)
    np.random.seed(1)
    t = cls(None, cfg, device=DEV)
    for update, _, gstep, _, info in t.train_iter():
        if stop_after is not None and update == stop_after:
            break
    torch.cuda.synchronize()
    return t, update, gstep, info


def _params(t):
    return torch.cat([p.detach().reshape(-1) for p in t.agent.parameters()]).clone()


@pytest.mark.parametrize("kind", ["selfplay", "league"])
def test_tally_only_run_equals_the_parent(kind):
    parent, child = _trainers()[kind]
    tp, *_ = _run(parent, _cfg())
    tc, *_ = _run(child, _cfg(track_resample_every=0))
    assert torch.equal(_params(tp), _params(tc)), "the tally changed the training run"
    tab = tc.track_table()
    assert tab["episodes"].sum() >= 3 * 2 * TN and (tab["episodes"] > 0).all()  # max_steps = 6, 16 steps, 3 updates
    # six-step episodes mostly time out level (a tie places car 1 first): wins are checked in the rollout tests
    assert (tab["wins"] <= tab["episodes"]).all() and tab["timeouts"].sum() > 0
    assert tc.envs.venv.track_generation == 0 and tc.retired == []
    from rx.track_selfplay import format_track_table
    text = format_track_table(tab)
    assert "win rate" in text and len(text.splitlines()) == TSLOTS + 1
    if kind == "league":
        assert torch.equal(tp.envs.tally, tc.envs.tally) and torch.equal(tp.envs.opp_id, tc.envs.opp_id)
    tp.envs.close()
    tc.envs.close()


@pytest.mark.parametrize("kind", ["selfplay", "league"])
def test_resample_draws_from_the_table_and_graphs_agree(kind):
    from rx import _lib
    L = _lib.load()
    _, child = _trainers()[kind]
    over = dict(track_resample_every=1, curriculum_refresh=0.0, curriculum_score="contested")
    t, update, *_ = _run(child, _cfg(**over), stop_after=1)
    assert update == 1
    cur, venv = t.curriculum, t.envs.venv
    assert venv.track_generation == 1 and t.retired == [[]]
    cdf = cur.cdf.cpu().numpy()  # the table the resample before update 1 drew from
    want = np.full(TN, -1, np.int32)
    tc = track_io(_lib, cur.n_tracks, cdf=cdf, track_of_env=want, seed=cur.seed)
    _lib.check(L.rx_track_draw_host(ctypes.byref(tc), TN, 1, cur.mix, None), "host draw")
    assert np.array_equal(venv.track_of_env, want) and np.array_equal(venv._st["track"].cpu().numpy(), want)
    assert not np.array_equal(want, np.arange(TN) % TSLOTS) and len(np.unique(want)) == TSLOTS
    assert t._graphs_by_kind == {} or all(not g for g in t._graphs_by_kind.values())
    t.envs.close()
    # the same run to its end, eager and with captured rollout graphs
    te, *_ = _run(child, _cfg(**over))
    tg, *_ = _run(child, _cfg(graph_rollout=True, **over))
    assert te.envs.venv.track_generation == tg.envs.venv.track_generation == 2
    assert torch.equal(_params(te), _params(tg)), "graph_rollout changed the run"
    assert torch.equal(te.curriculum.tally, tg.curriculum.tally) and torch.equal(te.curriculum.duel, tg.curriculum.duel)
    te.envs.close()
    tg.envs.close()


def test_retirement_and_checkpoint_round_trip(tmp_path):
    _, child = _trainers()["league"]
    over = dict(track_resample_every=1, curriculum_refresh=0.5, curriculum_mastery=0.0, curriculum_min_episodes=1)
    t, update, gstep, info = _run(child, _cfg(**over), stop_after=0)
    cur, venv = t.curriculum, t.envs.venv
    before_t, before_d = cur.tally.cpu().numpy().copy(), cur.duel.cpu().numpy().copy()
    before_cp = [cp.copy() for cp in t._cps]
    assert (before_t[:, 0] > 0).all()
    state = np.random.get_state()
    t.resample_tracks()
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]  # np.random stays
    retired = t.retired[-1]
    assert len(retired) == 3 and venv.track_generation == 1  # floor(0.5 * 6), every slot qualifies at mastery 0
    p_sorted = np.argsort(-((before_d[:, 0] + 1.0) / (before_t[:, 0] + 2.0)), kind="stable")[:3]
    assert sorted(retired) == sorted(p_sorted.tolist())  # the highest p of the chosen score ("lose": the win rate)
    now_t, now_d = cur.tally.cpu().numpy(), cur.duel.cpu().numpy()
    for k in range(TSLOTS):
        if k in retired:
            assert not now_t[k].any() and not now_d[k].any()
            assert t._cps[k].shape != before_cp[k].shape or not np.array_equal(t._cps[k], before_cp[k])
        else:
            assert np.array_equal(now_t[k], before_t[k]) and np.array_equal(now_d[k], before_d[k])
            assert np.array_equal(t._cps[k], before_cp[k])
    geoms = venv.tracks.geoms  # the env runs the new pool
    assert len(geoms) == TSLOTS
    for k in range(TSLOTS):
        assert np.array_equal(np.asarray(geoms[k].control_points, dtype=np.float64), t._cps[k]), k
    # one more rollout's worth of tallies, then the round trip
    cur.tally[0, 0] += 5
    path = t.save_checkpoint(0, gstep, info, path=str(tmp_path / "duel.pth"))
    torch.manual_seed(1)
    np.random.seed(1)
    t2 = child(None, _cfg(**over), device=DEV)
    start, _, _ = t2.load_checkpoint(path)
    assert start == 0
    assert torch.equal(t2.curriculum.tally, cur.tally) and torch.equal(t2.curriculum.duel, cur.duel)
    assert np.array_equal(t2.envs.venv.track_of_env, venv.track_of_env)
    assert t2.envs.venv.track_generation == venv.track_generation
    assert all(np.array_equal(a, b) for a, b in zip(t2._cps, t._cps)) and t2._widths == t._widths
    for a, b in zip(t2.envs.venv.tracks.geoms, venv.tracks.geoms):
        assert np.array_equal(a.waypoints, b.waypoints) and a.track_width == b.track_width
    # a checkpoint without the key: a fresh curriculum on the built pool
    ck = torch.load(path, map_location=DEV, weights_only=True)
    del ck["track_state"]
    torch.save(ck, str(tmp_path / "plain.pth"))
    t3 = child(None, _cfg(**over), device=DEV)
    t3.load_checkpoint(str(tmp_path / "plain.pth"))
    assert not t3.curriculum.tally.any() and t3.envs.venv.track_generation == 0
    assert all(np.array_equal(a, b) for a, b in zip(t3._cps, before_cp))
    for e in (t, t2, t3):
        e.envs.close()
