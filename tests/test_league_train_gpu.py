"""League training on the device: the two small kernels against their host
twins, rx_league_rollout_steps against rx_selfplay_rollout_steps with every env
pinned to one bank member, against a step-by-step composition of the existing
entry points with mixed opponents, through a captured graph, and
rx.league_train.LeagueSelfPlayPPO end to end.

Envs: two-car envs on three golden tracks with max_steps = 20, so every env
ends at least twice in a 48-step rollout (a truncation gets a placement too).
Shapes: 37 and 200 envs, both ragged against the 16-row policy tile.  No
tolerance anywhere: every comparison is exact."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests.test_league_train_cpu import CDF5, SLOTS, _info, _tallies

pytestmark = pytest.mark.gpu

DEV = "cuda"
T = 48
NAMES = ("obs", "actions", "logprobs", "dones", "rewards", "values", "next_obs", "next_done")


def _agents(seeds, D=19):
    """tests/test_league_gpu.py::_agents: the output layer widened so the mean actions
    depend on the observation; seeds and log-stds differ."""
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


def _venv(golden, N, seed=9, max_steps=20):
    from rx.vector_env import RacingVectorEnv
    ks = [k for k in range(golden.n_tracks) if golden.tracks[k]["label"] != "default"][:3]
    return RacingVectorEnv([golden.tracks[ks[i % 3]]["cp"] for i in range(N)],
                           [golden.tracks[ks[i % 3]]["width"] for i in range(N)], n_agents=2, device=DEV,
                           seed=seed, max_steps=max_steps)


def _bufs(N):
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    return [z(T, N, 19), z(T, N, 2), z(T, N), z(T, N), z(T, N), z(T, N)]  # obs actions logprobs dones rewards values


def _noise(N, seed=8):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn((T, N, 2), device=DEV, generator=g), torch.randn((T, N, 2), device=DEV, generator=g))


def _league_env(golden, N, agent_idx, prec, bank_agents, seed=9):
    from rx import _lib
    from rx.league_train import LeagueVectorEnv
    lenv = LeagueVectorEnv(_venv(golden, N, seed), agent_idx, seed=77, pool_size=len(bank_agents),
                           prec=_lib.PRECISION[prec])
    for k, a in enumerate(bank_agents):
        lenv.set_slot(k, a)
    lenv.n_live = len(bank_agents)
    return lenv


def _start(env, bufs):
    """Reset; the rollout's first rows.  Returns (next_obs, next_done) holders."""
    o = env.reset_device()
    bufs[0][0].copy_(o)
    bufs[3][0].zero_()
    return torch.full((env.num_envs, 19), float("nan"), device=DEV), torch.full((env.num_envs,), float("nan"),
                                                                              device=DEV)


def _dev_lg(_lib, n_slots, ids, cnt, tally, cdf, seed=0, agent=0):
    p = _lib.ptr
    return _lib.RxLeagueIO(n_slots, agent, None, None, 0, p(ids), p(cnt), p(tally), p(cdf), seed, 0)


# ---- 1. the kernels == their host twins -------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["zero", "random", "all_won", "all_won_big", "played_unplayed"])
def test_weights_device_equals_host(pattern):
    from rx import _lib
    L = _lib.load()
    for n_slots, n_live in SLOTS:
        tally = _tallies(n_slots, pattern)
        d_tally = torch.from_numpy(tally).to(DEV)
        d_cdf = torch.full((n_slots,), -7.0, dtype=torch.float64, device=DEV)
        dlg = _dev_lg(_lib, n_slots, None, None, d_tally, d_cdf)
        for power, mix, prior in itertools.product(range(5), (0.0, 0.1, 1.0), (0.5, 1.0)):
            cdf = np.full(n_slots, -7.0)
            hlg = _dev_lg(_lib, n_slots, None, None, tally, cdf)
            _lib.check(L.rx_league_weights_host(ctypes.byref(hlg), n_live, power, mix, prior, None), "host")
            d_cdf.fill_(-7.0)
            _lib.check(L.rx_league_weights(ctypes.byref(dlg), n_live, power, mix, prior, _lib.stream_ptr(None)), "dev")
            got = d_cdf.cpu().numpy()
            assert np.array_equal(got.view(np.uint64), cdf.view(np.uint64)), (n_slots, n_live, power, mix, prior)
        assert torch.equal(d_tally.cpu(), torch.from_numpy(tally))


@pytest.mark.parametrize("agent", [0, 1])
@pytest.mark.parametrize("mask", ["none", "all", "third", "null"])
@pytest.mark.parametrize("n", [200, 4096])
def test_draw_device_equals_host(n, mask, agent):
    from rx import _lib
    L = _lib.load()
    rng = np.random.RandomState(n + 13 * agent)
    seed = 0x0123456789ABCDEF ^ n
    ids = rng.randint(0, 4, n).astype(np.int32)
    cnt = rng.randint(0, 50, n).astype(np.int32)
    tally = rng.randint(0, 9, (5, 3)).astype(np.int64)
    info = _info(n, rng)
    done = {"none": np.zeros(n, np.float32), "all": np.ones(n, np.float32),
            "third": (np.arange(n) % 3 == 0).astype(np.float32), "null": None}[mask]
    host = [ids.copy(), cnt.copy(), tally.copy(), CDF5.copy()]
    dev = [torch.from_numpy(x).to(DEV) for x in (ids, cnt, tally, CDF5)]
    d_done = None if done is None else torch.from_numpy(done).to(DEV)
    d_info = torch.from_numpy(info).to(DEV)
    hlg, dlg = _dev_lg(_lib, 5, *host, seed, agent), _dev_lg(_lib, 5, *dev, seed, agent)
    for call in range(2):
        _lib.check(L.rx_league_draw_host(ctypes.byref(hlg), n, _lib.ptr(done), _lib.ptr(info), None), "host")
        _lib.check(L.rx_league_draw(ctypes.byref(dlg), n, _lib.ptr(d_done), _lib.ptr(d_info), _lib.stream_ptr(None)),
                   "dev")
        for h, d, name in zip(host, dev, ("opp_id", "draw_count", "tally", "cdf")):
            assert np.array_equal(d.cpu().numpy(), h), (name, call)
    if done is not None and mask != "none":
        assert not np.array_equal(host[2], tally)


# ---- 2. every env pinned to bank member k == rx_selfplay_rollout_steps with that opponent -------------
@pytest.mark.parametrize("agent_idx", [0, 1])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("N", [37, 200])
def test_pinned_opponent_equals_selfplay_rollout(golden, N, prec, agent_idx):
    from rx import _lib
    from rx.league_train import LeagueStepRollout
    from rx.optim import FlatParams
    from rx.ppo_fused import SelfPlayStepRollout
    from rx.selfplay import SelfPlayVectorEnv
    k = 1
    bank = _agents((21, 22, 23))
    learner = _agents((29,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(N)
    P = _lib.PRECISION[prec]
    # league: the table is 0 below k and 1 from k on, every id = k
    lenv = _league_env(golden, N, agent_idx, prec, bank)
    lenv.cdf.copy_(torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64))
    lenv.opp_id.fill_(k)
    ba = _bufs(N)
    na, da = _start(lenv, ba)
    LeagueStepRollout(learner, flat, lenv, T, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    # self-play: bank member k as the frozen opponent, the same start (same env seed) and noise
    sp = SelfPlayVectorEnv(_venv(golden, N), agent_idx)
    sp.set_opponent(bank[k], FlatParams(bank[k]), P)
    bb = _bufs(N)
    nb, db = _start(sp, bb)
    sr = SelfPlayStepRollout(learner, flat, sp, T, P)
    assert SelfPlayStepRollout.supported(sp, learner, {})
    sr(*bb, nb, db, eps=eps, opp_eps=oeps)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, ba + [na, da], bb + [nb, db]):
        assert not torch.isnan(x).any(), name
        assert torch.equal(x, y), name
    assert torch.equal(lenv.venv.buf["obs"], sp.venv.buf["obs"])
    ended = int((ba[3][1:] != 0).sum()) + int((da != 0).sum())
    assert ended >= 2 * N  # max_steps = 20: every env ended at least twice
    tally = lenv.tally.cpu().numpy()
    assert tally[k, 0] == ended and not tally[[0, 2]].any()
    assert tally[k, 1] + tally[k, 2] <= ended and tally[k, 1] + tally[k, 2] > 0
    assert (lenv.opp_id == k).all() and int(lenv.draw_count.sum()) == ended
    lenv.close()
    sp.close()


# ---- 3. mixed opponents == the step-by-step composition of existing entry points ---------------------
def _mixed_case(golden, N, prec, seed_env=9):
    """A league env with 3 distinct policies and a non-trivial table, reset, ids drawn."""
    bank = _agents((31, 32, 33))
    lenv = _league_env(golden, N, 0, prec, bank, seed=seed_env)
    lenv.tally.copy_(torch.tensor([[40, 30, 5], [25, 5, 15], [0, 0, 0]]))
    lenv.weights(3, power=2, mix=0.1, prior=1.0)
    lenv.draw_all()
    return lenv


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixed_opponents_equal_step_by_step_composition(golden, prec):
    from rx import _lib
    from rx.league_train import LeagueStepRollout
    from rx.optim import FlatParams
    from rx.ppo_fused import PolicyAct
    L = _lib.load()
    N = 200
    P = _lib.PRECISION[prec]
    learner = _agents((39,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(N, seed=18)
    lenv = _mixed_case(golden, N, prec)
    cdf = lenv.cdf.cpu().numpy().copy()
    assert 0.0 < cdf[0] < cdf[1] < 1.0 and cdf[2] == 1.0
    start = [lenv.opp_id.cpu().numpy().copy(), lenv.draw_count.cpu().numpy().copy(), lenv.tally.cpu().numpy().copy()]
    assert len(np.unique(start[0])) == 3
    ba = _bufs(N)
    na, da = _start(lenv, ba)
    LeagueStepRollout(learner, flat, lenv, T, P)(*ba, na, da, eps=eps, opp_eps=oeps)
    torch.cuda.synchronize()

    # the reference: rx_policy_act, rx_policy_act_bank, rx_step, rx_league_draw_host, step by step
    ref = _league_env(golden, N, 0, prec, _agents((31, 32, 33)))  # the same bank and env seed; its own draws unused
    v = ref.venv
    ids, cnt, tally = (x.copy() for x in start)
    hlg = _dev_lg(_lib, 3, ids, cnt, tally, cdf, ref.seed, 0)
    d_ids = torch.from_numpy(ids).to(DEV)
    bb = _bufs(N)
    nb, db = _start(ref, bb)
    obs, actions, logprobs, dones, rewards, values = bb
    pa = PolicyAct(learner, flat, N, 19, P)
    act = torch.zeros((N, 2, 2), device=DEV)
    sink = torch.empty((2, N), device=DEV)
    ob1, a1 = v.buf["obs"][:, 1], act[:, 1]
    mixed_tiles = 0
    wins = start[2].copy()  # [slot] games, episodes car 0 placed first in, episodes car 1 did
    for t in range(T):
        last = t + 1 == T
        pa(obs[t], actions[t], logprobs[t], values[t], eps=eps[t])
        io = _lib.RxPolicyIO(19, N, _lib.view_ptr(ob1), _lib.ptr(oeps[t]), _lib.ptr(ref.params), _lib.ptr(ref.log_std),
                             _lib.view_ptr(a1), _lib.ptr(sink[0]), _lib.ptr(sink[1]), ob1.stride(0), a1.stride(0), P,
                             None, 0)
        b = _lib.RxPolicyBankIO(io, 3, 1, ref.stride, _lib.ptr(d_ids))
        _lib.check(L.rx_policy_act_bank(ctypes.byref(b), _lib.stream_ptr(None)), "rx_policy_act_bank")
        mixed_tiles += sum(len(np.unique(ids[i:i + 16])) > 1 for i in range(0, N, 16))
        act[:, 0].copy_(actions[t])
        done = db if last else dones[t + 1]
        o, r, _ = v.step_device(act, done_out=done, full_info=True)
        (nb if last else obs[t + 1]).copy_(o[:, 0])
        rewards[t].copy_(r[:, 0])
        h_done, h_info = done.cpu().numpy(), v.buf["info"].cpu().numpy()
        # who won, read here from the step's info rows and not through rx_league.h: the learner drives car 0
        place = h_info.reshape(N, 2, -1)[:, :, _lib.RX_INFO_PLACEMENT]
        for e in np.nonzero(h_done)[0]:
            wins[ids[e]] += (1, place[e, 0] == 1.0, place[e, 1] == 1.0)
        _lib.check(L.rx_league_draw_host(ctypes.byref(hlg), N, _lib.ptr(h_done), _lib.ptr(h_info), None), "draw_host")
        d_ids.copy_(torch.from_numpy(ids))
    torch.cuda.synchronize()
    assert mixed_tiles > 0, "no 16-env tile ever held two opponents: the bank loop was not exercised"
    for name, x, y in zip(NAMES, ba + [na, da], bb + [nb, db]):
        assert not torch.isnan(x).any(), name
        assert torch.equal(x, y), name
    assert torch.equal(lenv.venv.buf["obs"], v.buf["obs"])
    assert np.array_equal(lenv.opp_id.cpu().numpy(), ids)
    assert np.array_equal(lenv.draw_count.cpu().numpy(), cnt)
    assert np.array_equal(lenv.tally.cpu().numpy(), tally)
    assert np.array_equal(tally, wins) and wins[:, 1:].sum() > start[2][:, 1:].sum()  # some episode had a winner
    assert tally[:, 0].sum() - start[2][:, 0].sum() == int((ba[3][1:] != 0).sum()) + int((da != 0).sum())
    assert ids.max() < 3 and (tally[:, 0] > start[2][:, 0]).all()  # every member played
    lenv.close()
    ref.close()


# ---- 4. a captured graph of the rollout, replayed twice == two eager calls ---------------------------
def test_rollout_graph_replays_equal_eager_calls(golden):
    from rx import _lib
    from rx.league_train import LeagueStepRollout
    from rx.optim import FlatParams
    N = 200
    learner = _agents((49,))[0]
    flat = FlatParams(learner)
    eps, oeps = _noise(N, seed=28)
    res = []
    for graphed in (False, True):
        lenv = _mixed_case(golden, N, "fp32")
        bufs = _bufs(N)
        nobs, nd = _start(lenv, bufs)
        nobs.copy_(bufs[0][0])
        nd.zero_()
        sr = LeagueStepRollout(learner, flat, lenv, T, _lib.RX_PREC_FP32)

        def body():
            bufs[0][0].copy_(nobs)
            bufs[3][0].copy_(nd)
            sr(*bufs, nobs, nd, eps=eps, opp_eps=oeps)
        torch.cuda.synchronize()
        if graphed:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):  # records only: nothing runs
                body()
            for _ in range(2):
                g.replay()
            lenv._launched()
        else:
            for _ in range(2):
                body()
        torch.cuda.synchronize()
        res.append([x.clone() for x in bufs + [nobs, nd]] + [lenv.venv.buf["obs"].clone(), lenv.opp_id.clone(),
                                                              lenv.draw_count.clone(), lenv.tally.clone()])
        lenv.close()
    for name, x, y in zip(NAMES + ("env_obs", "opp_id", "draw_count", "tally"), *res):
        assert not (x.is_floating_point() and torch.isnan(x).any()), name
        assert torch.equal(x, y), name
    assert int(res[0][-2].sum()) > N  # draws happened beyond the first draw_all


# ---- 5. LeagueSelfPlayPPO end to end --------------------------------------------------------------
@pytest.mark.parametrize("rollout_steps", ["auto", False])
def test_league_selfplay_ppo_end_to_end(golden, tmp_path, rollout_steps):
    from rx.configs import self_play_config
    from rx.league import PolicyBank
    from rx.league_train import LeagueSelfPlayPPO, LeagueStepRollout

    class Trainer(LeagueSelfPlayPPO):
        def _make_venv(self, env_fn):
            # max_steps = 6: the envs are rebuilt every update, so in a 16-step rollout only a short
            # episode limit makes every env end (at least twice) and the tally check mean something
            v = _venv(golden, self.config["num_envs"], seed=self.config["seed"], max_steps=6)
            v.reset_device()
            return v

    n_upd = 6
    cfg = self_play_config(num_envs=32, num_steps=16, snapshot_freq=1, pool_size=3, checkpoint=False,
                           num_minibatches=4, rollout_steps=rollout_steps)
    cfg["total_timesteps"] = n_upd * cfg["batch_size"]
    torch.manual_seed(1)
    np.random.seed(1)
    t = Trainer(None, cfg, device=DEV)
    seen = []
    orig = t.collect_rollout

    def spy(*bufs):
        before = int(t.envs.tally[:, 0].sum())
        out = orig(*bufs)
        ended = int((out[3][1:] != 0).sum()) + int((out[7] != 0).sum())
        seen.append((before, int(t.envs.tally[:, 0].sum()), ended))
        return out
    t.collect_rollout = spy
    total = 0
    for update, num_updates, gstep, ep, info in t.train_iter():
        assert num_updates == n_upd
        n_live = min(update, 3)
        assert len(t.opponent_pool) == n_live == t.envs.n_live == t._slots.n_live
        assert t._slots.member_slots() == [s % 3 for s in range(max(0, update - 3), update)]
        before, after, ended = seen[-1]
        if n_live:
            assert int(t.envs.opp_id.max()) < n_live and int(t.envs.opp_id.min()) >= 0
            assert after - before == ended and ended >= 2 * 32, update
            total += ended
        else:
            assert after == before == 0 and t.envs.opponent_policy is None  # the random opponent, nothing tallied
        # the bank row of every pool member is that member
        for slot, o in zip(t._slots.member_slots(), t.opponent_pool):
            flat = torch.cat([p.reshape(-1) for p in o.parameters()])
            assert torch.equal(t.envs.params[slot, :flat.numel()], flat) and torch.equal(t.envs.log_std[slot], o.log_std)
    assert update == n_upd - 1 and t._slots.member_slots() == [2, 0, 1]  # the slots wrapped
    assert isinstance(t.__dict__.get("_lg_steps_rollout"), LeagueStepRollout) == (rollout_steps == "auto")
    raw = t.envs.tally.cpu().numpy()
    h2h = t.head_to_head()
    assert [r["slot"] for r in h2h] == [2, 0, 1] and [r["snapshot"] for r in h2h] == [2, 3, 4]
    for r in h2h:
        g, w, l = (int(x) for x in raw[r["slot"]])
        assert (r["games"], r["wins"], r["losses"], r["draws"]) == (g, w, l, g - w - l)
        assert r["win_rate"] == ((w + 0.5 * (g - w - l)) / g if g else None)
    assert 0 < raw[:, 0].sum() <= total  # reused slots started again
    # save, load into a fresh trainer, and the plain bank loader
    path = t.save_checkpoint(5, gstep, info, path=str(tmp_path / "league.pth"))
    t2 = Trainer(None, cfg, device=DEV)
    start, _, _ = t2.load_checkpoint(path)
    assert start == 5 and len(t2.opponent_pool) == 3 and t2._slots.n_snapshots == t._slots.n_snapshots == 5
    assert torch.equal(t2.envs.tally, t.envs.tally) and torch.equal(t2.envs.draw_count, t.envs.draw_count)
    assert torch.equal(t2.envs.params, t.envs.params) and torch.equal(t2.envs.log_std, t.envs.log_std)
    assert t2.head_to_head() == h2h
    bank = PolicyBank.from_checkpoint(path, device=DEV)
    assert bank.n_policies == 4
    for member, slot in enumerate(t._slots.member_slots()):
        assert torch.equal(bank.params[1 + member], t.envs.params[slot])
    t.envs.close()
    t2.envs.close()
