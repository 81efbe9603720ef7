"""League play (rx_policy_act_bank, rx_match_steps, rx.league) without a GPU:
the symbols, the struct layouts, every argument check that runs before a HIP
call, the PolicyBank on CPU tensors, the seat table, the LeagueResult reductions
from hand-written records and the Bradley-Terry ratings against closed forms."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _agent(D, seed, dtype=torch.float32):
    from rx.agent import Agent
    from rx.spaces import Box
    torch.manual_seed(seed)
    a = Agent(Box(-1.0, 1.0, shape=(D,), dtype=np.float32), Box(-1.0, 1.0, shape=(2,), dtype=np.float32))
    with torch.no_grad():
        a.log_std.copy_(torch.tensor([-0.1 * seed, -0.2 * seed]))
    return a.to(dtype)


# ---- the C ABI ----------------------------------------------------------------------------------
def test_symbols_and_version(L):
    from rx import _lib
    for name in ("rx_policy_act_bank", "rx_match_steps"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name)
    assert _lib.ABI_VERSION == 25 == L.rx_abi_version()
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    assert re.search(r"#define\s+RX_ABI_VERSION\s+25\b", src)


@pytest.mark.parametrize("cname,cls", [("rx_policy_bank_io", "RxPolicyBankIO"), ("rx_match_io", "RxMatchIO")])
def test_structs_match_the_header_layout(cname, cls):
    from rx import _lib
    S = getattr(_lib, cls)
    src = open(os.path.join(ROOT, "include", "rx.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in S._fields_]
    if cls == "RxPolicyBankIO":  # the rx_policy_io (112 bytes on LP64), two int32, an int64, a pointer
        assert ctypes.sizeof(_lib.RxPolicyIO) == 112 and S.n_policies.offset == 112
        assert S.params_stride.offset == 120 and ctypes.sizeof(S) == 136
    else:  # rx_eval_io's 80 bytes, two int32, an int64, a pointer
        assert S.n_active.offset == 72 and S.n_policies.offset == 80 and S.seat.offset == 96
        assert ctypes.sizeof(S) == 104


def _bank_io(_lib, p, D=19, n=32):
    io = _lib.RxPolicyIO(D, n, p, p, p, p, p, p, p, 0, 0, _lib.RX_PREC_FP32, None, 0)
    return _lib.RxPolicyBankIO(io, 3, 1, 11136, p)


def test_policy_act_bank_refuses_by_name(L):
    """Every RX_EINVAL path returns before a HIP call: this runs without a device."""
    from rx import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(b, word):
        assert L.rx_policy_act_bank(ctypes.byref(b) if b is not None else None, None) == _lib.RX_EINVAL, word
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())
    refused(None, "null")
    b = _bank_io(_lib, p)
    b.io.obs_dim = 7
    refused(b, "obs_dim")
    for n in (0, -5):
        b = _bank_io(_lib, p)
        b.io.n = n
        refused(b, "n=")
    b = _bank_io(_lib, p)
    b.n_policies = 0
    refused(b, "n_policies")
    for D in (15, 19):
        b = _bank_io(_lib, p, D)
        b.params_stride = L.rx_ppo_n_params(D) - 1
        refused(b, "params_stride")
    b = _bank_io(_lib, p)
    b.io.precision = 4
    refused(b, "precision")
    for tc, n in ((0, 32), (3, 32), (2, 33)):
        b = _bank_io(_lib, p, n=n)
        b.tile_cars = tc
        refused(b, "tile_cars")
    for field, v in (("obs_stride", 18), ("act_stride", 1), ("act2_stride", 1)):
        b = _bank_io(_lib, p)
        setattr(b.io, field, v)
        refused(b, field)
    for k in ("obs", "eps", "params", "log_std", "actions", "logprobs", "values"):
        b = _bank_io(_lib, p)
        setattr(b.io, k, None)
        refused(b, k)
    b = _bank_io(_lib, p)
    b.policy_of_row = None
    refused(b, "policy_of_row")


def test_match_steps_refuses_by_name(L):
    from rx import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    h = ctypes.create_string_buffer(1 << 16)  # a stand-in: the checks below return before the handle is read
    io = _lib.RxIO()
    for k in ("obs", "reward64", "info", "done_f32"):
        setattr(io, k, p)

    def mk():
        return _lib.RxMatchIO(19, _lib.RX_PREC_FP32, p, p, p, p, p, p, p, p, p, 2, 0, 11136, p)

    def refused(m, word, hh=h, ii=io, n=1):
        rc = L.rx_match_steps(hh, ctypes.byref(ii) if ii is not None else None,
                              ctypes.byref(m) if m is not None else None, n, None)
        assert rc == _lib.RX_EINVAL, word
        assert word.encode() in L.rx_last_error(), (word, L.rx_last_error())
    refused(mk(), "null handle", hh=None)
    refused(mk(), "null io", ii=None)
    refused(None, "null match io")
    for n in (0, -2):
        refused(mk(), "n_steps", n=n)
    m = mk()
    m.obs_dim = 11
    refused(m, "obs_dim")
    m = mk()
    m.precision = 2
    refused(m, "precision")
    m = mk()
    m.n_policies = 0
    refused(m, "n_policies")
    m = mk()
    m.params_stride = L.rx_ppo_n_params(19) - 1
    refused(m, "params_stride")
    for k in ("params", "log_std", "eps", "seat", "actions", "logp_sink", "value_sink", "acc", "active", "n_active"):
        m = mk()
        setattr(m, k, None)
        refused(m, k)
    for k in ("obs", "reward64", "info", "done_f32"):
        setattr(io, k, None)
        refused(mk(), k)
        setattr(io, k, p)


# ---- PolicyBank ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [15, 19])
def test_bank_rows_equal_the_flat_policy(L, D):
    from rx.evaluate import _flat_policy
    from rx.league import PolicyBank
    agents = [_agent(D, s) for s in (1, 2, 3)]
    bank = PolicyBank(agents)
    n = L.rx_ppo_n_params(D)
    assert bank.n_policies == len(bank) == 3 and bank.obs_dim == D and bank.n_params == n
    assert bank.stride >= n and bank.stride % 64 == 0
    assert bank.params.shape == (3, bank.stride) and bank.params.dtype == torch.float32 and bank.params.is_contiguous()
    assert bank.log_std.shape == (3, 2) and bank.log_std.is_contiguous()
    for p, a in enumerate(agents):
        assert torch.equal(bank.params[p, :n], _flat_policy(a))
        assert not bank.params[p, n:].any()
        assert torch.equal(bank.log_std[p], a.log_std)
    # state dicts give the same bank
    b2 = PolicyBank([a.state_dict() for a in agents])
    assert torch.equal(b2.params, bank.params) and torch.equal(b2.log_std, bank.log_std)


def test_bank_from_checkpoint(tmp_path):
    """The dict SelfPlayPPO.save_checkpoint writes: agent_state_dict, then opponent_pool in order."""
    from rx.league import PolicyBank
    agents = [_agent(19, s) for s in (4, 5, 6)]
    ck = {"update": 10, "global_step": 1, "agent_state_dict": agents[0].state_dict(), "optimizer_state_dict": {},
          "opponent_pool": [a.state_dict() for a in agents[1:]], "config": {}, "training_info": {}}
    want = PolicyBank(agents)
    got = PolicyBank.from_checkpoint(ck)
    assert torch.equal(got.params, want.params) and torch.equal(got.log_std, want.log_std)
    path = tmp_path / "ck.pth"
    torch.save(ck, path)
    got = PolicyBank.from_checkpoint(str(path))
    assert torch.equal(got.params, want.params) and torch.equal(got.log_std, want.log_std)
    with pytest.raises(ValueError, match="agent_state_dict"):
        PolicyBank.from_checkpoint({"opponent_pool": []})


def test_bank_refusals():
    from rx.league import PolicyBank
    with pytest.raises(ValueError, match="at least one"):
        PolicyBank([])
    with pytest.raises(ValueError, match="mixed observation widths"):
        PolicyBank([_agent(15, 1), _agent(19, 2)])
    with pytest.raises(ValueError, match="float32"):
        PolicyBank([_agent(19, 1), _agent(19, 2, torch.float64)])
    with pytest.raises(ValueError, match="float32"):
        PolicyBank([_agent(19, 2, torch.float64).state_dict()])
    with pytest.raises(ValueError, match="layout"):  # 5 sensors: 9 columns, no policy kernel
        PolicyBank([_agent(9, 1)])
    with pytest.raises(ValueError, match="layout"):
        PolicyBank([_agent(9, 1).state_dict()])
    wide = _agent(19, 3)
    wide.critic[4] = torch.nn.Linear(64, 2)  # another head: policy_supported counts the parameters
    with pytest.raises(ValueError, match="layout"):
        PolicyBank([wide])
    sd = _agent(19, 1).state_dict()
    del sd["critic.2.bias"]
    with pytest.raises(ValueError, match="critic.2.bias"):
        PolicyBank([sd])


# ---- seating ------------------------------------------------------------------------------------
def test_seating_layout_and_refusals():
    from rx.league import all_pairs, seating
    pairs = all_pairs(3)
    assert pairs == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    s = seating(pairs, 4, 3)
    assert s.dtype == np.int32 and s.shape == (24, 2) and s.flags["C_CONTIGUOUS"]
    for k, pr in enumerate(pairs):  # every pairing's episodes are contiguous
        assert (s[4 * k:4 * k + 4] == np.array(pr)).all()
    assert np.array_equal(seating([(1, 1)], 2), [[1, 1], [1, 1]])
    for bad in ([(0, 3)], [(-1, 0)]):
        with pytest.raises(ValueError, match="indices"):
            seating(bad, 2, 3)
    with pytest.raises(ValueError, match="indices"):
        seating([(-1, 0)], 2)
    with pytest.raises(ValueError):
        seating([], 2, 3)
    with pytest.raises(ValueError, match="episodes"):
        seating(pairs, 0, 3)


def test_league_refuses_bad_pairs_before_any_library_call(monkeypatch):
    """An index beyond the bank raises ValueError before an env is built or the library loaded."""
    from rx import _lib, league

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    bank = league.PolicyBank([_agent(19, 1), _agent(19, 2)])
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(league.League, "_match", boom)
    lg = league.League(num_tracks=1, num_runs=1)
    for bad in ([(0, 2)], [(-1, 1)]):
        with pytest.raises(ValueError, match="indices"):
            lg.play(bank, pairs=bad)
    with pytest.raises(ValueError, match="prec"):
        lg.play(bank, prec="fp16")


# ---- LeagueResult -------------------------------------------------------------------------------
def _record(rows):
    """rows: per episode ((placement, flags, reward) of car 0, the same of car 1)."""
    rec = np.zeros((len(rows), 2, 10))
    for e, cars in enumerate(rows):
        for q, (place, flags, rew) in enumerate(cars):
            rec[e, q, 5], rec[e, q, 6], rec[e, q, 0], rec[e, q, 2] = place, flags, rew, 7
    return rec


def test_result_reductions():
    from rx.league import LeagueResult
    FIN, CRASH = 2, 1
    seat = np.array([[0, 1], [0, 1], [1, 0], [1, 0], [0, 2], [2, 0], [0, 2]], np.int32)
    rec = _record([((1, FIN, 10.0), (2, CRASH, -4.0)),   # 0 beats 1 from car 0
                   ((2, 0, 1.0), (1, FIN, 9.0)),          # car 1 wins: 1 beats 0
                   ((2, CRASH, -2.0), (1, FIN, 8.0)),     # seats swapped, car 1 wins: 0 beats 1
                   ((0, 0, 3.0), (0, 0, 5.0)),            # cut by the step limit: no placement, a draw
                   ((1, 0, 2.0), (2, CRASH | 32, 0.0)),   # 0 beats 2
                   ((1, FIN, 6.0), (2, 0, 0.0)),          # 2 beats 0
                   ((1, 0, 0.0), (2, 0, 0.0))])           # 0 beats 2 again
    r = LeagueResult(rec, seat, 3)
    assert np.array_equal(r.games, [[0, 2, 2], [2, 0, 0], [1, 0, 0]])
    assert np.array_equal(r.wins, [[0, 2, 2], [1, 0, 0], [1, 0, 0]])
    assert np.array_equal(r.draws, [[0, 1, 0], [1, 0, 0], [0, 0, 0]])
    g = r.games + r.games.T
    assert np.array_equal(r.wins + r.wins.T + r.draws, g)
    assert np.allclose(r.finish_rate, [2 / 7, 1 / 4, 1 / 3]) and np.allclose(r.crash_rate, [0, 2 / 4, 1 / 3])
    assert np.allclose(r.mean_reward, [(10 + 1 + 8 + 5 + 2 + 0 + 0) / 7, (-4 + 9 - 2 + 3) / 4, 2.0])
    t = r.table()
    assert [d["policy"] for d in t] == list(np.argsort(-r.ratings(), kind="stable"))
    assert t[0]["policy"] == 0 and t[0]["wins"] == 4 and t[0]["losses"] == 2 and t[0]["draws"] == 1 and t[0]["games"] == 7
    assert set(t[0]) >= {"rating", "finish_rate", "crash_rate", "mean_reward", "name"}
    assert abs(sum(d["rating"] for d in t)) < 1e-9
    assert len(r.format().splitlines()) == 4 and r.to_json()["episodes"] == 7
    with pytest.raises(ValueError, match="indices"):
        LeagueResult(rec, seat, 2)
    with pytest.raises(ValueError):
        LeagueResult(rec[:, :1], seat, 3)


# ---- Bradley-Terry ------------------------------------------------------------------------------
@pytest.mark.parametrize("w01,w10", [(30, 10), (7, 13), (5, 5)])
def test_bradley_terry_two_players(w01, w10):
    from rx.league import bradley_terry
    r = bradley_terry([[0, w01], [w10, 0]])
    assert abs((r[0] - r[1]) - 400.0 * np.log10(w01 / w10)) < 1e-9 and abs(r.sum()) < 1e-9
    # a draw is half a win to each side
    r2 = bradley_terry([[0, w01 - 1], [w10 - 1, 0]], [[0, 2], [2, 0]])
    assert np.allclose(r, r2, atol=1e-9)


def test_bradley_terry_recovers_known_strengths():
    """Exact expected counts n_ij s_i / (s_i + s_j) from known strengths: the MM
    fixed point is those strengths, so the gaps must come back to 1e-6 Elo."""
    from rx.league import bradley_terry
    elo = np.array([0.0, 100.0, 250.0])
    s = 10.0 ** (elo / 400.0)
    n = np.array([[0, 400, 600], [400, 0, 200], [600, 200, 0]], np.float64)
    w = n * s[:, None] / (s[:, None] + s[None, :])
    r = bradley_terry(w)
    assert np.abs((r - r[0]) - elo).max() < 1e-6
    assert abs(r.mean()) < 1e-9


def test_bradley_terry_clamp():
    """The documented clamp: a winless policy is granted half a win (its unbeaten
    opponent then has half a loss), and no rating leaves +-1200 around the mean."""
    from rx.league import ELO_CLAMP, bradley_terry
    r = bradley_terry([[0, 10], [0, 0]])
    assert np.isfinite(r).all() and abs((r[0] - r[1]) - 400.0 * np.log10(10 / 0.5)) < 1e-6
    r = bradley_terry([[0, 10 ** 6], [0, 0]])
    assert ELO_CLAMP == 1200.0 and np.array_equal(r, [1200.0, -1200.0])
    r = bradley_terry([[0, 5, 5], [0, 0, 5], [0, 0, 0]])
    assert np.isfinite(r).all() and r[0] > r[1] > r[2] and np.abs(r).max() <= ELO_CLAMP
    r = bradley_terry([[0, 3, 0], [1, 0, 0], [0, 0, 0]])  # a policy without games: the others' mean
    assert np.isfinite(r).all() and abs(r[2] - (r[0] + r[1]) / 2) < 1e-9
