"""League training without a GPU: the host twins rx_league_weights_host and
rx_league_draw_host against a NumPy restatement of csrc/rx_league.h written here
(bit for bit: every step of the rules is one separately rounded IEEE operation
in a fixed order), one distribution check of the draw, every argument check
that runs before a HIP call, and the host-side pool bookkeeping of
rx.league_train."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---- the NumPy restatement ----------------------------------------------------------------------
def np_weights(tally, n_slots, n_live, power, mix, prior):
    f8 = np.float64
    mix, prior = f8(mix), f8(prior)
    f = np.zeros(n_live, dtype=f8)
    for k in range(n_live):
        g, w, l = (f8(int(v)) for v in tally[k])
        num = (w + f8(0.5) * ((g - w) - l)) + prior
        den = g + f8(2.0) * prior
        q = f8(1.0) - num / den
        fk = f8(1.0)
        for _ in range(power):
            fk = fk * q
        f[k] = fk
    F = f8(0.0)
    for k in range(n_live):
        F = F + f[k]
    nl = f8(n_live)
    cdf = np.ones(n_slots, dtype=f8)
    c = f8(0.0)
    for k in range(n_live - 1):
        prob = f8(1.0) / nl if F == 0.0 else (f8(1.0) - mix) * (f[k] / F) + mix / nl
        c = c + prob
        cdf[k] = c
    return cdf, F


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def np_uniform(seed, count, e):
    h = splitmix64(seed ^ splitmix64((((count & 0xFFFFFFFF) << 32) ^ e) & M64))
    return float(h >> 11) * 2.0 ** -53


def np_draw(cdf, opp_id, draw_count, tally, seed, agent, done, info):
    """In place, env by env; done None = every env, nothing tallied."""
    n_slots = len(cdf)
    for e in range(len(opp_id)):
        if done is not None:
            if done[e] == 0:
                continue
            k = int(opp_id[e])
            tally[k, 0] += 1
            tally[k, 1] += int(info[e, agent, 3] == 1.0)
            tally[k, 2] += int(info[e, 1 - agent, 3] == 1.0)
        u = np_uniform(seed, int(draw_count[e]), e)
        k = 0
        while k < n_slots - 1 and not u < cdf[k]:
            k += 1
        opp_id[e] = k
        draw_count[e] += 1


def _lg(_lib, n_slots, opp_id=None, draw_count=None, tally=None, cdf=None, seed=0, agent=0):
    p = _lib.ptr
    return _lib.RxLeagueIO(n_slots, agent, None, None, 0, p(opp_id), p(draw_count), p(tally), p(cdf), seed, 0)


# ---- rx_league_weights_host ---------------------------------------------------------------------
SLOTS = [(1, 1), (5, 3), (5, 5), (64, 64), (64, 1)]
BIG = 1 << 60  # (g + prior) / (g + 2 prior) rounds to 1.0: the priority is exactly 0


def _tallies(n_slots, pattern):
    t = np.zeros((n_slots, 3), dtype=np.int64)
    rng = np.random.RandomState(n_slots * 7 + len(pattern))
    if pattern == "random":
        t[:, 0] = rng.randint(0, 5000, n_slots)
        t[:, 1] = (t[:, 0] * rng.rand(n_slots)).astype(np.int64)
        t[:, 2] = ((t[:, 0] - t[:, 1]) * rng.rand(n_slots)).astype(np.int64)
    elif pattern == "all_won":  # w == g everywhere, small counts: every priority small but > 0
        t[:, 0] = t[:, 1] = rng.randint(1, 200, n_slots)
    elif pattern == "all_won_big":  # w == g everywhere and 1 - p == 0.0: F == 0, the uniform fallback
        t[:, 0] = t[:, 1] = BIG
    elif pattern == "played_unplayed":
        t[0] = (40, 30, 5)
    else:
        assert pattern == "zero"
    return t


@pytest.mark.parametrize("pattern", ["zero", "random", "all_won", "all_won_big", "played_unplayed"])
@pytest.mark.parametrize("n_slots,n_live", SLOTS)
def test_weights_host_equals_numpy_bits(L, n_slots, n_live, pattern):
    from rx import _lib
    tally = _tallies(n_slots, pattern)
    for power, mix, prior in itertools.product(range(5), (0.0, 0.1, 1.0), (0.5, 1.0)):
        cdf = np.full(n_slots, -7.0)
        lg = _lg(_lib, n_slots, tally=tally, cdf=cdf)
        _lib.check(L.rx_league_weights_host(ctypes.byref(lg), n_live, power, mix, prior, None), "weights_host")
        want, F = np_weights(tally, n_slots, n_live, power, mix, prior)
        assert np.array_equal(cdf.view(np.uint64), want.view(np.uint64)), (power, mix, prior, cdf, want)
        assert np.all(np.diff(cdf) >= 0.0) and np.all(cdf[n_live - 1:] == 1.0) and np.all(cdf > 0.0)
        if pattern == "all_won_big" and power > 0:
            assert F == 0.0  # the fallback really ran: a uniform table
            assert np.array_equal(cdf[:n_live - 1], np.cumsum(np.full(n_live, 1.0 / n_live))[:n_live - 1])
        if pattern == "played_unplayed" and n_live > 1 and power > 0 and mix < 1.0:
            assert cdf[0] < 1.0 / n_live  # the slot the learner beats is drawn less often than an unplayed one


# ---- rx_league_draw_host ------------------------------------------------------------------------
CDF5 = np.array([0.125, 0.5, 0.5625, 1.0, 1.0])  # n_live = 4 of 5 slots; slot 2 is rare, slot 4 dead
PROB5 = np.array([0.125, 0.375, 0.0625, 0.4375, 0.0])


def _info(n, rng):
    info = np.zeros((n, 2, 4), dtype=np.float64)
    place = rng.randint(0, 3, n)  # 0: nobody placed (a draw), 1: car 0 first, 2: car 1 first
    info[place == 1, 0, 3], info[place == 1, 1, 3] = 1.0, 2.0
    info[place == 2, 0, 3], info[place == 2, 1, 3] = 2.0, 1.0
    info[:, :, 0] = rng.rand(n, 2)
    return info


@pytest.mark.parametrize("agent", [0, 1])
@pytest.mark.parametrize("mask", ["none", "all", "third", "null"])
@pytest.mark.parametrize("n", [1, 17, 200, 4096])
def test_draw_host_equals_numpy(L, n, mask, agent):
    from rx import _lib
    rng = np.random.RandomState(n + 13 * agent)
    seed = 0x0123456789ABCDEF ^ n
    ids = rng.randint(0, 4, n).astype(np.int32)
    cnt = rng.randint(0, 50, n).astype(np.int32)
    tally = rng.randint(0, 9, (5, 3)).astype(np.int64)
    info = _info(n, rng)
    done = {"none": np.zeros(n, np.float32), "all": np.ones(n, np.float32),
            "third": (np.arange(n) % 3 == 0).astype(np.float32), "null": None}[mask]
    got = [ids.copy(), cnt.copy(), tally.copy()]
    want = [ids.copy(), cnt.copy(), tally.copy()]
    cdf = CDF5.copy()
    lg = _lg(_lib, 5, got[0], got[1], got[2], cdf, seed, agent)
    for call in range(2):  # the second call continues from the first call's counters
        _lib.check(L.rx_league_draw_host(ctypes.byref(lg), n, _lib.ptr(done), _lib.ptr(info), None), "draw_host")
        np_draw(CDF5, want[0], want[1], want[2], seed, agent, done, info)
        for g, w, name in zip(got, want, ("opp_id", "draw_count", "tally")):
            assert np.array_equal(g, w), (name, call)
        touched = np.ones(n, bool) if done is None else done != 0
        assert np.array_equal(got[0][~touched], ids[~touched]) and np.array_equal(got[1][~touched], cnt[~touched])
        assert np.array_equal(got[1][touched], cnt[touched] + call + 1)
        assert got[0].min() >= 0 and got[0].max() < 4  # every id is a live slot
        if done is None:
            assert np.array_equal(got[2], tally)
        else:
            assert got[2][:, 0].sum() - tally[:, 0].sum() == (call + 1) * int(touched.sum())
    assert np.array_equal(cdf, CDF5)


def test_draw_distribution(L):
    """65,536 envs drawn once against a fixed 5-slot table: slot k's count is
    Binomial(N, prob_k) if the hash is uniform, so it lies within 6 standard
    deviations sqrt(N prob_k (1 - prob_k)) of N prob_k (a 2e-9 event per slot
    otherwise); the dead slot gets nothing."""
    from rx import _lib
    n = 65536
    ids = np.full(n, -1, np.int32)
    cnt = np.zeros(n, np.int32)
    tally = np.zeros((5, 3), np.int64)
    cdf = CDF5.copy()
    lg = _lg(_lib, 5, ids, cnt, tally, cdf, seed=20240607)
    _lib.check(L.rx_league_draw_host(ctypes.byref(lg), n, None, None, None), "draw_host")
    counts = np.bincount(ids, minlength=5)
    for k in range(5):
        sd = np.sqrt(n * PROB5[k] * (1.0 - PROB5[k]))
        print(f"slot {k}: {counts[k]} drawn, expected {n * PROB5[k]:.0f} +- {6 * sd:.1f}")
        assert abs(counts[k] - n * PROB5[k]) <= 6.0 * sd, (k, counts)
    assert counts.sum() == n and not tally.any()


# ---- the C ABI ----------------------------------------------------------------------------------
LEAGUE_EXPORTS = ("rx_league_weights", "rx_league_weights_host", "rx_league_draw", "rx_league_draw_host",
                  "rx_league_rollout_steps")


def test_symbols_version_and_struct(L):
    from rx import _lib
    for name in LEAGUE_EXPORTS:
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert _lib.ABI_VERSION == 25 == L.rx_abi_version()
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert re.search(r"#define\s+RX_ABI_VERSION\s+25\b", src)
    body = re.search(r"typedef struct rx_league_io \{(.*?)\} rx_league_io;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    S = _lib.RxLeagueIO
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in S._fields_]
    # two int32, two pointers, an int64, four pointers, a uint64, an int32 + padding (LP64)
    assert (S.params.offset, S.params_stride.offset, S.opp_id.offset, S.seed.offset) == (8, 24, 32, 64)
    assert S.opp_precision.offset == 72 and ctypes.sizeof(S) == 80


def test_league_entry_points_refuse_by_name(L):
    """Every RX_EINVAL path returns before a HIP call: this runs without a device."""
    from rx import _lib
    buf = ctypes.create_string_buffer(1024)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def lg(**over):
        s = _lib.RxLeagueIO(5, 0, p, p, 11136, p, p, p, p, 1, _lib.RX_PREC_FP32)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def refused(rc, word):
        assert rc == _lib.RX_EINVAL, word
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())

    for sfx in ("", "_host"):
        W, Dr = getattr(L, "rx_league_weights" + sfx), getattr(L, "rx_league_draw" + sfx)
        refused(W(None, 3, 1, 0.1, 1.0, None), "null")
        refused(Dr(None, 8, None, None, None), "null")
        for ns in (0, -1, 65):
            refused(W(ctypes.byref(lg(n_slots=ns)), 1, 1, 0.1, 1.0, None), "n_slots")
            refused(Dr(ctypes.byref(lg(n_slots=ns)), 8, None, None, None), "n_slots")
        for k in ("tally", "cdf"):
            refused(W(ctypes.byref(lg(**{k: None})), 3, 1, 0.1, 1.0, None), k)
        for k in ("tally", "cdf", "opp_id", "draw_count"):
            refused(Dr(ctypes.byref(lg(**{k: None})), 8, None, None, None), k)
        for nl in (0, -2, 6):
            refused(W(ctypes.byref(lg()), nl, 1, 0.1, 1.0, None), "n_live")
        for pw in (-1, 5):
            refused(W(ctypes.byref(lg()), 3, pw, 0.1, 1.0, None), "power")
        for mix in (-0.01, 1.01, float("nan")):
            refused(W(ctypes.byref(lg()), 3, 1, mix, 1.0, None), "mix")
        for prior in (0.0, -1.0, float("nan")):
            refused(W(ctypes.byref(lg()), 3, 1, 0.1, prior, None), "prior")
        for ag in (-1, 2):
            refused(Dr(ctypes.byref(lg(agent=ag)), 8, None, None, None), "agent")
        for n in (0, -3):
            refused(Dr(ctypes.byref(lg()), n, None, None, None), "n=")
        refused(Dr(ctypes.byref(lg()), 8, p, None, None), "info")

    R = L.rx_league_rollout_steps
    io, r, sp = _lib.RxIO(), _lib.RxRolloutIO(), _lib.RxSelfplayIO()
    args = (ctypes.byref(io), ctypes.byref(r), ctypes.byref(sp))
    assert R(None, None, None, None, None, 0, None) == _lib.RX_EINVAL
    refused(R(None, *args, None, 0, None), "null league io")
    refused(R(None, *args, ctypes.byref(lg()), 0, None), "null handle")
    refused(R(None, *args, ctypes.byref(lg(n_slots=65)), 0, None), "n_slots")
    refused(R(None, *args, ctypes.byref(lg(agent=2)), 0, None), "agent")
    for k in ("params", "log_std", "opp_id", "draw_count", "tally", "cdf"):
        refused(R(None, *args, ctypes.byref(lg(**{k: None})), 0, None), k)
    refused(R(None, *args, ctypes.byref(lg(params_stride=L.rx_ppo_n_params(19) - 1)), 0, None), "params_stride")
    refused(R(None, *args, ctypes.byref(lg(opp_precision=3)), 0, None), "opp_precision")
    refused(R(None, *args, ctypes.byref(lg()), 7, None), "precision=7")


# ---- rx.league_train: the host-side bookkeeping ----------------------------------------------------
def test_pool_slots():
    from rx.league_train import PoolSlots
    s = PoolSlots(3)
    assert s.n_live == 0 and s.members() == [] and s.member_slots() == []
    got = [s.push() for _ in range(8)]
    assert [g[0] for g in got] == list(range(8))
    assert [g[1] for g in got] == [0, 1, 2, 0, 1, 2, 0, 1] == [s.slot_of(k) for k in range(8)]
    assert [g[2] for g in got] == [False] * 3 + [True] * 5  # from snapshot 3 on a slot is reused
    assert s.n_live == 3 and s.members() == [5, 6, 7] and s.member_slots() == [2, 0, 1]  # oldest first
    t = PoolSlots(5, n_snapshots=2)
    assert t.n_live == 2 and t.members() == [0, 1] and t.member_slots() == [0, 1]
    for bad in (0, 65, 1000):
        with pytest.raises(ValueError, match="pool_size"):
            PoolSlots(bad)
    assert PoolSlots(64).pool_size == 64


class _FakeVenv:
    """What SelfPlayVectorEnv / LeagueVectorEnv read of a two-car vector env, on CPU tensors."""
    n_agents, D = 2, 19

    def __init__(self, n):
        self.num_envs, self.device = n, torch.device("cpu")
        self.single_observation_space = self.single_action_space = None
        self.envs = []
        self.buf = {"obs": torch.zeros((n, 2, 19)), "info": torch.zeros((n, 2, 4), dtype=torch.float64)}


def _agent(seed):
    from rx.agent import Agent
    from rx.spaces import Box
    torch.manual_seed(seed)
    a = Agent(Box(-1.0, 1.0, shape=(19,), dtype=np.float32), Box(-1.0, 1.0, shape=(2,), dtype=np.float32))
    with torch.no_grad():
        a.log_std.copy_(torch.tensor([-0.1 * seed, -0.2 * seed]))
    return a


def test_set_slot_fills_the_bank_row_and_restarts_a_reused_slots_tally():
    from rx.league import PolicyBank
    from rx.league_train import LeagueVectorEnv, PoolSlots
    env = LeagueVectorEnv(_FakeVenv(8), 0, seed=3, pool_size=3)
    slots = PoolSlots(3)
    agents = [_agent(k + 1) for k in range(4)]
    for a in agents[:3]:
        env.set_slot(slots.push()[1], a)
    bank = PolicyBank(agents[:3])  # the layout rx_policy_act_bank reads
    assert env.stride == bank.stride and torch.equal(env.params, bank.params) and torch.equal(env.log_std, bank.log_std)
    env.tally.copy_(torch.arange(9).view(3, 3))
    s, slot, reused = slots.push()  # snapshot 3 overwrites slot 0
    assert (s, slot, reused) == (3, 0, True)
    env.set_slot(slot, agents[3])
    assert env.tally.tolist() == [[0, 0, 0], [3, 4, 5], [6, 7, 8]]
    assert torch.equal(env.params[0], PolicyBank([agents[3]]).params[0]) and torch.equal(env.params[1:], bank.params[1:])
    env.set_slot(1, agents[0], reset_tally=False)  # a checkpoint restore keeps the counts
    assert env.tally[1].tolist() == [3, 4, 5]
    with pytest.raises(ValueError, match="slot"):
        env.set_slot(3, agents[0])
    with pytest.raises(ValueError, match="pool_size"):
        LeagueVectorEnv(_FakeVenv(8), 0, pool_size=65)


def test_trainer_refuses_before_it_touches_a_device(monkeypatch):
    from rx import dist as rdist
    from rx.configs import self_play_config
    from rx.league_train import LeagueSelfPlayPPO

    def env_fn(i):
        raise AssertionError("no env may be built")
    with pytest.raises(ValueError, match="pool_size"):
        LeagueSelfPlayPPO(env_fn, self_play_config(pool_size=65))
    monkeypatch.setattr(rdist, "world", lambda: 2)
    with pytest.raises(ValueError, match="world size"):
        LeagueSelfPlayPPO(env_fn, self_play_config())
    monkeypatch.setattr(rdist, "world", lambda: 1)
    for key, bad in (("pfsp_power", 5), ("pfsp_mix", 1.5), ("pfsp_prior", 0.0)):
        with pytest.raises(ValueError, match=key):
            LeagueSelfPlayPPO(env_fn, self_play_config(**{key: bad}))
