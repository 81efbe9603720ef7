"""League play on the device: rx_policy_act_bank against rx_policy_act row by
row (torch.equal: a batch row is one MFMA column, so which tile a row shares
with which other policies' rows must not change a bit of it), rx_match_steps
against rx_eval_steps where the seats cannot matter and against an open-loop
replay where they do, and rx.league.League end to end.

Shapes: 53 rows = three full 16-row tiles and a ragged one of 5; 37 two-car
envs = per car two full tiles and a ragged one, with the seat swap at env 20
inside the second tile.  No tolerance anywhere: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _agents(D, seeds):
    """tests/test_eval_fused_gpu.py::_agent without an env: the output layer widened
    x40 so the mean actions depend on the observation; seeds and log-stds differ."""
    from rx.agent import Agent
    from rx.spaces import Box
    out = []
    for k, seed in enumerate(seeds):
        torch.manual_seed(seed)
        a = Agent(Box(-1.0, 1.0, shape=(D,), dtype=np.float32), Box(-1.0, 1.0, shape=(2,), dtype=np.float32)).to(DEV)
        with torch.no_grad():
            a.actor_mu[4].weight.mul_(40.0)
            a.log_std.copy_(torch.tensor([-0.3 - 0.2 * k, -0.5 + 0.15 * k]))
        out.append(a)
    return out


def _flat(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()]).contiguous()


def _single(L, D, prec, agent, obs, eps, n, obs_stride=0, act_out=None, act_stride=0):
    """One rx_policy_act launch with ``agent`` alone: (actions, logprobs, values)."""
    from rx import _lib
    flat = _flat(agent)
    act = torch.full((n, 2), float("nan"), device=DEV) if act_out is None else act_out
    lp = torch.full((n,), float("nan"), device=DEV)
    val = torch.full((n,), float("nan"), device=DEV)
    io = _lib.RxPolicyIO(D, n, _lib.view_ptr(obs), _lib.ptr(eps), _lib.ptr(flat), _lib.ptr(agent.log_std),
                         _lib.view_ptr(act), _lib.ptr(lp), _lib.ptr(val), obs_stride, act_stride,
                         _lib.PRECISION[prec], None, 0)
    _lib.check(L.rx_policy_act(ctypes.byref(io), _lib.stream_ptr(None)), "rx_policy_act")
    torch.cuda.synchronize()
    return act, lp, val


def _banked(L, bank, prec, obs, eps, ids, n, tile_cars=1, actions2=False):
    from rx import _lib
    act = torch.full((n, 2), float("nan"), device=DEV)
    act2 = torch.full((n, 2), float("nan"), device=DEV) if actions2 else None
    lp = torch.full((n,), float("nan"), device=DEV)
    val = torch.full((n,), float("nan"), device=DEV)
    assert 0 <= int(ids.min()) and int(ids.max()) < bank.n_policies  # the kernel cannot check device memory
    idt = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(DEV)
    io = _lib.RxPolicyIO(bank.obs_dim, n, _lib.ptr(obs), _lib.ptr(eps), _lib.ptr(bank.params), _lib.ptr(bank.log_std),
                         _lib.ptr(act), _lib.ptr(lp), _lib.ptr(val), 0, 0, _lib.PRECISION[prec], _lib.ptr(act2), 0)
    b = _lib.RxPolicyBankIO(io, bank.n_policies, tile_cars, bank.stride, _lib.ptr(idt))
    _lib.check(L.rx_policy_act_bank(ctypes.byref(b), _lib.stream_ptr(None)), "rx_policy_act_bank")
    torch.cuda.synchronize()
    return act, lp, val, act2


# ---- 1. bank == single, contiguous rows -------------------------------------------------------
N_ROWS = 53
ASSIGN = {
    "all0": np.zeros(N_ROWS, np.int32), "all1": np.ones(N_ROWS, np.int32), "all2": np.full(N_ROWS, 2, np.int32),
    "tile_uniform": np.repeat([0, 1, 2, 0], 16)[:N_ROWS].astype(np.int32),
    "mod3": (np.arange(N_ROWS) % 3).astype(np.int32),
    "one_odd_row": np.where(np.arange(N_ROWS) == 21, 2, 1).astype(np.int32),
    "ragged_mixed": np.concatenate([np.zeros(48, np.int32), np.array([0, 1, 2, 1, 0], np.int32)]),
}


@pytest.fixture(scope="module")
def rows_case():
    """Per (D, prec): the bank, the inputs and every policy's rx_policy_act outputs, computed once."""
    from rx import _lib
    from rx.league import PolicyBank
    L = _lib.load()
    cache = {}

    def get(D, prec):
        if (D, prec) not in cache:
            agents = _agents(D, (11, 12, 13))
            bank = PolicyBank(agents, device=DEV)
            g = torch.Generator(device=DEV).manual_seed(100 + D)
            obs = torch.rand((N_ROWS, D), device=DEV, generator=g) * 2.0 - 1.0
            eps = torch.empty((N_ROWS, 2), device=DEV).normal_(generator=g)
            ref = [_single(L, D, prec, a, obs, eps, N_ROWS) for a in agents]
            for r in ref:
                assert not any(torch.isnan(t).any() for t in r)
            # the policies really differ: otherwise a wrong row choice would go unseen
            assert not torch.equal(ref[0][0], ref[1][0]) and not torch.equal(ref[1][2], ref[2][2])
            cache[(D, prec)] = (L, bank, obs, eps, ref)
        return cache[(D, prec)]
    return get


@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("D", [15, 19])
def test_bank_equals_single(rows_case, D, prec, assign):
    L, bank, obs, eps, ref = rows_case(D, prec)
    ids = ASSIGN[assign]
    act, lp, val, act2 = _banked(L, bank, prec, obs, eps, ids, N_ROWS, actions2=(assign == "mod3"))
    pick = torch.from_numpy(ids.astype(np.int64)).to(DEV)
    ar = torch.arange(N_ROWS, device=DEV)
    for k, got in enumerate((act, lp, val)):
        want = torch.stack([r[k] for r in ref])[pick, ar]
        assert not torch.isnan(got).any(), "a row was left unwritten"
        assert torch.equal(got, want), (assign, k, (got != want).nonzero()[:4].tolist())
    if act2 is not None:
        assert torch.equal(act2, act)


# ---- 2. the two-car layout, tiled by car --------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_bank_two_car_layout(prec):
    from rx import _lib
    from rx.league import PolicyBank
    L = _lib.load()
    N, D = 37, 19
    agents = _agents(D, (21, 22))
    bank = PolicyBank(agents, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    obs = torch.rand((N, 2, D), device=DEV, generator=g) * 2.0 - 1.0
    eps = torch.empty((N, 2, 2), device=DEV).normal_(generator=g)
    seat = np.where(np.arange(N)[:, None] < 20, [[0, 1]], [[1, 0]]).astype(np.int32)  # the swap falls inside a tile
    act, lp, val, _ = _banked(L, bank, prec, obs.view(2 * N, D), eps.view(2 * N, 2), seat.reshape(-1), 2 * N,
                              tile_cars=2)
    act, lp, val = act.view(N, 2, 2), lp.view(N, 2), val.view(N, 2)
    assert not any(torch.isnan(t).any() for t in (act, lp, val))
    st = torch.from_numpy(seat.astype(np.int64)).to(DEV)
    for p, a in enumerate(agents):
        for q in (0, 1):  # policy p on car q's rows: strided views of the two-car buffers
            out = torch.full((N, 2, 2), float("nan"), device=DEV)
            ra, rl, rv = _single(L, D, prec, a, obs[:, q], eps[:, q].contiguous(), N, obs_stride=2 * D,
                                 act_out=out[:, q], act_stride=4)
            m = st[:, q] == p
            assert m.any()
            assert torch.equal(act[:, q][m], out[:, q][m])
            assert torch.equal(lp[:, q][m], rl[m]) and torch.equal(val[:, q][m], rv[m])


# ---- 3. / 4. rx_match_steps ---------------------------------------------------------------------
def _venv(golden, N, n_agents, seed=9):
    from rx.vector_env import RacingVectorEnv
    ks = [k for k in range(golden.n_tracks) if golden.tracks[k]["label"] != "default"][:3]
    return RacingVectorEnv([golden.tracks[ks[i % 3]]["cp"] for i in range(N)],
                           [golden.tracks[ks[i % 3]]["width"] for i in range(N)], n_agents=n_agents, device=DEV,
                           autoreset="disabled", seed=seed)


def _env_agents(v, seeds):
    return _agents(v.D, seeds)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("n_agents", [2, 1])
def test_match_equals_eval_when_the_seats_cannot_matter(golden, n_agents, prec):
    """A bank of two copies of ONE policy: whatever the seats, rx_match_steps must
    leave exactly what rx_eval_steps' policy mode leaves, call by call."""
    from rx.evaluate import FusedEval
    from rx.league import Match, PolicyBank
    N = 37
    va, vb = _venv(golden, N, n_agents), _venv(golden, N, n_agents)
    agent = _env_agents(va, (31,))[0]
    bank = PolicyBank([agent, agent], device=DEV)
    fe, m = FusedEval(va, chunk=8), Match(vb, chunk=8)
    if n_agents == 2:
        seat = np.tile(np.array([[0, 1]], np.int32), (N, 1))
    else:
        seat = (np.arange(N)[:, None] % 2).astype(np.int32)
    m.set_seat(seat, 2)
    flat = _flat(agent)
    fe.begin()
    m.begin()
    for call in range(3):
        torch.manual_seed(40 + call)  # both draw one normal_() of the same shape per call
        left_e = fe.policy_chunk(flat, agent.log_std, 8, prec=prec)
        torch.manual_seed(40 + call)
        left_m = m.steps(bank, 8, prec=prec)
        assert torch.equal(fe.eps, m.fe.eps)
        assert left_e == left_m
        assert torch.equal(fe.actions, m.fe.actions), call
        assert np.array_equal(fe.record(), m.fe.record()), call
        assert torch.equal(fe.active, m.fe.active) and torch.equal(fe.n_active, m.fe.n_active)
    assert fe.record()[:, :, 2].max() == 24.0
    va.close()
    vb.close()


def _play(m, bank, max_steps, prec):
    """Match.run by hand, keeping the reset observations and the first step's noise."""
    m.begin()
    obs0 = m.venv.buf["obs"].clone()
    taken, t, eps0 = [], 0, None
    while t < max_steps:
        n = min(m.chunk, max_steps - t)
        left = m.steps(bank, n, prec=prec)
        if eps0 is None:
            eps0 = m.fe.eps[0].clone()
        taken.append(m.fe.actions[:n].clone())
        t += n
        if left == 0:
            break
    return m.fe.record(), torch.cat(taken), obs0, eps0


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_match_with_distinct_policies(golden, prec):
    from rx import _lib
    from rx.evaluate import FusedEval
    from rx.league import Match, PolicyBank, all_pairs, seating
    L = _lib.load()
    N, D = 37, 19
    agents = None
    for max_steps in (40, 400):
        va, vb = _venv(golden, N, 2, seed=4), _venv(golden, N, 2, seed=4)  # same seed: the same start-side draws
        if agents is None:
            agents = _env_agents(va, (41, 42, 43))
            bank = PolicyBank(agents, device=DEV)
        seat = seating(all_pairs(3), 7, 3)[:N]  # six pairings of 7 episodes, the last group ragged
        assert len(np.unique(seat, axis=0)) == 6
        m = Match(va)
        m.set_seat(seat, 3)
        torch.manual_seed(60)
        rec, acts, obs0, eps0 = _play(m, bank, max_steps, prec)
        assert acts.shape[1:] == (N, 2, 2) and not torch.isnan(acts).any()
        ended = int((m.fe.active == 0).sum())
        if max_steps == 40:
            assert rec[:, :, 2].max() == 40.0
        else:
            assert ended > 0, "no episode ended: the long run checks nothing the short one does not"
            assert (rec[m.fe.active.cpu().numpy() == 0][:, :, 5] > 0).all()  # an ended episode has placements
        # the first step's actions: every car on ITS policy
        st = torch.from_numpy(seat.astype(np.int64)).to(DEV)
        e0 = eps0.view(N, 2, 2)
        for p, a in enumerate(agents):
            for q in (0, 1):
                out = torch.full((N, 2, 2), float("nan"), device=DEV)
                _single(L, D, prec, a, obs0[:, q], e0[:, q].contiguous(), N, obs_stride=2 * D, act_out=out[:, q],
                        act_stride=4)
                sel = st[:, q] == p
                assert torch.equal(acts[0][:, q][sel], out[:, q][sel]), (p, q)
        # an open-loop replay of the recorded actions gives the same record
        want = FusedEval(vb).run_actions(acts, max_steps)
        assert np.array_equal(rec, want)
        va.close()
        vb.close()


# ---- 5. League end to end -----------------------------------------------------------------------
def test_league_end_to_end():
    from rx.league import League, PolicyBank
    lg = League(num_tracks=2, num_runs=1, max_steps=60, device=DEV)
    bank = PolicyBank(_agents(19, (51, 52, 53)), device=DEV)
    res = lg.play(bank, deterministic=True)
    P, E = 3, 2
    assert res.record.shape == (6 * E, 2, 10) and res.seat.shape == (6 * E, 2)
    games = np.zeros((P, P), np.int64)
    wins = np.zeros((P, P), np.int64)
    draws = np.zeros((P, P), np.int64)
    for e in range(6 * E):  # the reduction written out
        i, j = int(res.seat[e, 0]), int(res.seat[e, 1])
        games[i, j] += 1
        p0, p1 = res.record[e, 0, 5], res.record[e, 1, 5]
        assert not (p0 == 1 and p1 == 1)
        if p0 == 1:
            wins[i, j] += 1
        elif p1 == 1:
            wins[j, i] += 1
        else:
            draws[i, j] += 1
            draws[j, i] += 1
    assert np.array_equal(res.games, games) and np.array_equal(res.wins, wins) and np.array_equal(res.draws, draws)
    for i in range(P):
        assert res.games[i, i] == 0
        for j in range(P):
            if i != j:
                assert res.games[i, j] == E
                assert res.wins[i, j] + res.wins[j, i] + res.draws[i, j] == res.games[i, j] + res.games[j, i]
    assert res.record[:, :, 2].max() <= 60.0 and res.record[:, :, 2].min() >= 1.0
    table = res.table()
    assert len(table) == 3 and np.isfinite([d["rating"] for d in table]).all()
    # zero noise: an identically built league repeats the run (the SAME league's next play resets
    # its env again, and every reset draws the start sides anew, as the reference's shuffle does)
    lg2 = League(num_tracks=2, num_runs=1, max_steps=60, device=DEV)
    res2 = lg2.play(bank, deterministic=True)
    assert np.array_equal(res.record, res2.record) and np.array_equal(res.seat, res2.seat)
    assert np.array_equal(res.ratings(), res2.ratings())
    # the env is built once per pair count and kept
    res3 = lg.play(bank, deterministic=True)
    assert len(lg._matches) == 1 and np.array_equal(res3.seat, res.seat) and np.array_equal(res3.games, res.games)
    lg.close()
    lg2.close()


def test_selfplay_league_bank():
    import random
    from rx.configs import self_play_config
    from rx.envs import MultiRacingEnv
    from rx.evaluate import _flat_policy
    from rx.selfplay import SelfPlayPPO
    from rx.track import gen_tracks
    cfg = self_play_config(num_envs=4, num_steps=8, checkpoint=False)
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    pool = gen_tracks(num_tracks=4, seed=1)
    widths = [np.random.randint(6, 10) for _ in range(4)]
    t = SelfPlayPPO(lambda i: MultiRacingEnv(2, 11, pool, i, widths), cfg, device=DEV)
    snaps = []
    for k in range(2):
        s = t.snapshot_agent()
        with torch.no_grad():
            for p in s.parameters():
                p.add_(0.01 * (k + 1))
            s.log_std.fill_(-0.1 * (k + 1))
        snaps.append(s)
    t.opponent_pool = list(snaps)
    bank = t.league_bank()
    assert bank.n_policies == 3 and bank.obs_dim == 19
    for p, a in enumerate([t.agent] + snaps):
        assert torch.equal(bank.params[p, :bank.n_params], _flat_policy(a))
        assert torch.equal(bank.log_std[p], a.log_std)
    t.envs.close()
