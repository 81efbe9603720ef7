"""The fused evaluation (rx_eval_steps, ABI v25; rx.evaluate.FusedEval and
backend="fused") against the eager per-step loop and the reference.

Everything the fused path computes from given actions is compared EXACTLY
(``==`` on the per-episode dicts, array_equal on the record): k_eval_acc runs
the eager loop's float64 operations in its order.  The fused policy forward
differs from torch's by float rounding, so policy-mode runs record the actions
they took and the eager evaluator replays them.  The only tolerance here is the
north-star 1e-5 against the reference's golden metrics, copied from
tests/test_eval_golden_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Replay:
    """Stands in for an Agent in the EAGER evaluators: step t returns the recorded
    actions[t] ([T, rows, 2]; the last row again once they run out)."""

    def __init__(self, actions):
        self.a = actions.reshape(actions.shape[0], -1, 2)
        self.t = 0

    def _next(self):
        a = self.a[min(self.t, len(self.a) - 1)]
        self.t += 1
        return a.clone()

    def get_action_and_value(self, obs):
        return self._next(), None, None, None

    def actor_mu(self, obs):  # deterministic=True: the eager loop clamps this (a no-op on recorded actions)
        return self._next()


def _same(a, b):
    """Exact equality of two summary dicts (NaN == NaN for the one mean that may be empty)."""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], float) and math.isnan(a[k]):
            assert isinstance(b[k], float) and math.isnan(b[k]), k
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def _golden_actions(ref, device):
    off = ref["off"]
    n = len(off) - 1
    a = np.zeros((int(np.diff(off).max()), n, 2), np.float32)
    for i in range(n):
        a[: off[i + 1] - off[i], i] = ref["actions"][off[i]:off[i + 1]]
    return torch.from_numpy(a).to(device)


def _agent(v, seed):
    from rx.agent import Agent
    torch.manual_seed(seed)
    agent = Agent(v.single_observation_space, v.single_action_space).to(v.device)
    with torch.no_grad():  # the 0.01-gain output layer gives mu ~ 0: widen it so the mean actions differ by observation
        agent.actor_mu[4].weight.mul_(40.0)
    return agent


# ---- 1. open loop vs the reference -------------------------------------------------------------
def test_open_loop_matches_reference_and_eager(golden):
    from rx.evaluate import Evaluator
    ref = golden["eval_metrics"]
    fe = Evaluator(num_tracks=4, num_runs=2, device="cuda", backend="fused")
    acts = _golden_actions(ref, fe.device)
    res = fe.run_actions(acts)
    got = res["all_episodes"]
    n = len(ref["steps"])
    assert len(got) == n == res["num_episodes"]
    assert {int(s) for s in ref["steps"]} >= {2000} and ref["crashed"].any() and ref["finished"].any()
    for i in range(n):
        g = got[i]
        assert g["steps"] == int(ref["steps"][i]), i
        assert g["finished"] == bool(ref["finished"][i]) and g["crashed"] == bool(ref["crashed"][i]), i
        for k in ("progress", "speed", "distance_per_step"):
            assert abs(g[k] - float(ref[k][i])) <= 1e-5, (i, k, g[k], float(ref[k][i]))
        for k in ("total_reward", "total_distance"):
            assert abs(g[k] - float(ref[k][i])) <= 1e-5 * max(1.0, abs(float(ref[k][i]))), (i, k)
    ee = Evaluator(num_tracks=4, num_runs=2, device="cuda")
    _same(res, ee.run(_Replay(acts)))
    fe.close()
    ee.close()


# ---- 2. policy mode, single agent --------------------------------------------------------------
@pytest.fixture(scope="module")
def single_pair():
    from rx.evaluate import Evaluator
    fe = Evaluator(num_tracks=6, num_runs=3, max_steps=300, device="cuda", backend="fused")
    ee = Evaluator(num_tracks=6, num_runs=3, max_steps=300, device="cuda")
    yield fe, ee, _agent(fe.venv, 7)
    fe.close()
    ee.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("deterministic,max_steps", [(False, 300), (True, 300), (False, 40)])
def test_policy_mode_single_agent(single_pair, prec, deterministic, max_steps):
    fe, ee, agent = single_pair
    fe.max_steps = ee.max_steps = max_steps
    torch.manual_seed(11)
    res, acts = fe.run(agent, deterministic=deterministic, record_actions=True, prec=prec)
    N = fe.venv.num_envs
    assert acts.shape[1:] == (N, 1, 2) and acts.shape[0] <= max_steps
    assert float(acts.abs().max()) <= 1.0
    if deterministic:  # zero noise: the same mean actions whatever torch's generator holds
        torch.manual_seed(12)
        res2 = fe.run(agent, deterministic=True, prec=prec)
        _same(res, res2)
    want = ee.run(_Replay(acts), deterministic=deterministic)
    assert res["all_episodes"] == want["all_episodes"]
    _same(res, want)
    eps = res["all_episodes"]
    assert all(1 <= e["steps"] <= max_steps for e in eps)
    if max_steps == 40:
        running = fe.fused.active.cpu().numpy().astype(bool)
        assert running.any(), "no episode reached the step limit: the case checks nothing"
        for e, r in zip(eps, running):
            if r:
                assert e["steps"] == 40 and e["finished"] is False
    fe.max_steps = ee.max_steps = 300


def test_policy_mode_is_close_to_the_torch_forward(single_pair):
    """The first step's fused actions against the torch forward on the same reset
    observations: float rounding only (2e-6 absolute on actions in [-1, 1], the
    bound tests/test_ppo_fused_gpu.py holds rx_policy_act's fp32 actions to)."""
    fe, _, agent = single_pair
    fe.max_steps = 1
    obs0 = fe.venv.reset_device().clone()
    _, acts = fe.run(agent, deterministic=True, record_actions=True)
    fe.max_steps = 300
    with torch.no_grad():
        mu = agent.actor_mu(obs0).clamp(-1.0, 1.0)
    assert float((acts[0, :, 0] - mu).abs().max()) <= 2e-6


def test_unsupported_policy_is_refused():
    from rx.evaluate import Evaluator
    fe = Evaluator(num_tracks=1, num_runs=1, n_sensors=5, device="cuda", backend="fused")
    with pytest.raises(ValueError, match="eager"):
        fe.run(_agent(fe.venv, 1))
    ee = Evaluator(num_tracks=1, num_runs=1, device="cuda")
    with pytest.raises(ValueError, match="fused"):
        ee.run(_agent(ee.venv, 1), record_actions=True)
    fe.close()
    ee.close()


# ---- 3. two cars -------------------------------------------------------------------------------
def test_two_cars():
    from rx.evaluate import MultiEvaluator
    fe = MultiEvaluator(num_tracks=3, num_runs=2, max_steps=200, device="cuda", backend="fused")
    ee = MultiEvaluator(num_tracks=3, num_runs=2, max_steps=200, device="cuda")
    agent = _agent(fe.venv, 5)
    N = fe.venv.num_envs
    for prec in ("fp32", "bf16"):
        torch.manual_seed(3)
        res, acts = fe.run(agent, record_actions=True, prec=prec)
        assert acts.shape[1:] == (N, 2, 2)
        rep = _Replay(acts)
        assert rep.a.shape[1:] == (2 * N, 2)
        want = ee.run(rep)
        assert res["all_episodes"] == want["all_episodes"]
        assert [e["placement"] for e in res["all_episodes"]] == [e["placement"] for e in want["all_episodes"]]
        _same(res, want)
    fe.close()
    ee.close()


# ---- 4. working-state order under re-sorts, non-wide kernels -------------------------------------
def _eager_record(v, actions):
    """The record of rx_eval_io.acc accumulated by the eager loop's torch expressions
    (rx.evaluate.Evaluator.run / MultiEvaluator.run) over ``actions`` [T, N, A, 2]."""
    N, A, dev = v.num_envs, v.n_agents, v.device
    v.reset_device()
    active = torch.ones(N, dtype=torch.bool, device=dev)
    total_reward = torch.zeros((N, A), dtype=torch.float64, device=dev)
    total_dist = torch.zeros((N, A), dtype=torch.float64, device=dev)
    steps = torch.zeros(N, dtype=torch.int64, device=dev)
    info_last = torch.zeros((N, A, 4), dtype=torch.float64, device=dev)
    flags_last = torch.zeros((N, A), dtype=torch.uint8, device=dev)
    x, y = v.state["x"].view(N, A), v.state["y"].view(N, A)
    px, py = x.clone(), y.clone()
    for t in range(actions.shape[0]):
        _, _, done = v.step_device(actions[t], full_info=True)
        st = v.state
        act2 = active.unsqueeze(1)
        r64 = v.buf["reward64"].view(N, A)
        total_reward += torch.where(act2, r64, torch.zeros_like(r64))
        if t > 0:
            d = torch.sqrt((x - px) ** 2 + (y - py) ** 2)
            total_dist += torch.where(act2, d, torch.zeros_like(d))
        # the eager loop copies every position; an ended env's is never used again, the record keeps its last one
        px = torch.where(act2, x, px)
        py = torch.where(act2, y, py)
        steps += active.long()
        info_last = torch.where(act2.unsqueeze(2), v.buf["info"], info_last)
        flags_last = torch.where(act2, st["flags"].view(N, A), flags_last)
        active &= ~done.bool()
    rec = torch.zeros((N, A, 10), dtype=torch.float64, device=dev)
    rec[:, :, 0], rec[:, :, 1] = total_reward, total_dist
    rec[:, :, 2] = steps.double().unsqueeze(1)
    rec[:, :, 3], rec[:, :, 4], rec[:, :, 5] = info_last[:, :, 1], info_last[:, :, 0], info_last[:, :, 3]
    rec[:, :, 6] = flags_last.double()
    rec[:, :, 7], rec[:, :, 8] = px, py
    return rec.cpu().numpy(), active.cpu().numpy()


@pytest.mark.parametrize("n_agents,N", [(1, 4100), (2, 2100)])
def test_working_state_order_under_resorts(golden, n_agents, N):
    from rx.evaluate import FusedEval
    from rx.vector_env import RacingVectorEnv
    ks = [k for k in range(golden.n_tracks) if golden.tracks[k]["label"] != "default"][:8]
    assert len(ks) == 8
    cps = [golden.tracks[ks[i % 8]]["cp"] for i in range(N)]
    ws = [golden.tracks[ks[i % 8]]["width"] for i in range(N)]
    mk = lambda: RacingVectorEnv(cps, ws, n_agents=n_agents, device="cuda", autoreset="disabled",  # noqa: E731
                                 sort_interval=4, seed=9)
    va, vb = mk(), mk()
    assert va.schedule()["wide"] == 0 and va.env_order()[1] > 0  # non-wide kernels, the re-sort is on
    g = torch.Generator(device="cuda").manual_seed(17)
    acts = torch.rand((64, N, n_agents, 2), device="cuda", generator=g)
    acts[..., 0].mul_(2.0).sub_(1.0)  # steering in [-1, 1), throttle in [0, 1)
    fe = FusedEval(va)
    fe.begin()
    orders = [va.env_order()[0].copy()]
    for t0, n in ((0, 50), (50, 14)):  # a whole chunk and a partial one
        left = fe.actions_chunk(acts[t0:t0 + n])
        orders.append(va.env_order()[0].copy())
        assert left == int(fe.active.sum())
    for p in orders:
        assert np.array_equal(np.sort(p), np.arange(N))
    assert not np.array_equal(orders[0], orders[1]), \
        "the wave order never changed: the test proves nothing about the permutation"
    got = fe.record()
    want, active = _eager_record(vb, acts)
    assert np.array_equal(fe.active.cpu().numpy().astype(bool), active)
    assert 0 < active.sum() < N, "wanted ended and running episodes side by side"
    assert np.array_equal(got, want)
    assert got[:, :, 9].max() == 0.0 and got[:, :, 2].max() == 64.0
    va.close()
    vb.close()


# ---- 5. early-out and the active count -----------------------------------------------------------
def test_ended_evaluation_is_left_alone(golden):
    """Every env truncates at 30 steps, so a 64-step run ends every episode; a further
    chunk must not touch the record."""
    from rx.evaluate import FusedEval
    from rx.vector_env import RacingVectorEnv
    ks = [k for k in range(golden.n_tracks) if golden.tracks[k]["label"] != "default"][:2]
    N = 70  # a partial second wave
    v = RacingVectorEnv([golden.tracks[ks[i % 2]]["cp"] for i in range(N)],
                        [golden.tracks[ks[i % 2]]["width"] for i in range(N)], device="cuda", autoreset="disabled",
                        max_steps=30)
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = torch.rand((64, N, 1, 2), device="cuda", generator=g)
    fe = FusedEval(v)
    rec = fe.run_actions(acts, 64)
    assert int(fe.n_active.item()) == 0 and int(fe.active.sum()) == 0
    assert rec[:, 0, 2].max() == 30.0 and rec[:, 0, 2].min() >= 1.0
    before = fe.acc.clone()
    assert fe.actions_chunk(acts[:50]) == 0
    torch.cuda.synchronize()
    assert before.cpu().numpy().tobytes() == fe.acc.cpu().numpy().tobytes()
    assert int(fe.n_active.item()) == 0 and int(fe.active.sum()) == 0
    v.close()


def test_active_count_tracks_the_flags(single_pair):
    """active.sum() == n_active after every chunk of a policy-mode run (case 2's envs)."""
    from rx.evaluate import _flat_policy
    fe, _, agent = single_pair
    f = fe.fused
    flat = _flat_policy(agent)
    torch.manual_seed(21)
    f.begin()
    assert int(f.active.sum()) == int(f.n_active.item()) == fe.venv.num_envs
    seen = []
    for _ in range(6):
        left = f.policy_chunk(flat, agent.log_std, 50)
        assert left == int(f.n_active.item()) == int(f.active.sum())
        seen.append(left)
    assert seen == sorted(seen, reverse=True) and seen[-1] < fe.venv.num_envs


def test_eval_steps_refuses_a_foreign_width(single_pair):
    """obs_dim must be the handle's D (checked on a live handle; the null / n_steps checks run without a GPU)."""
    from rx import _lib
    fe, _, _ = single_pair
    f, v = fe.fused, fe.venv
    ev = f._ev(f.actions)
    ev.obs_dim = 19
    assert f.L.rx_eval_steps(v._h, v._io(full=True), ctypes.byref(ev), 1, None) == _lib.RX_EINVAL
    assert b"obs_dim" in f.L.rx_last_error()
