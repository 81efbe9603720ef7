"""Batched evaluation -- evaluate.py:12-122,173-238 and utils/metrics.py:39-142.

The reference evaluates a policy on 40 tracks (gen_tracks(40, seed=42)) x 5
runs, run r using width RandomState(42+r).randint(4, 10) (note: indexed by
RUN, evaluate.py:30), one episode at a time with a batch-1 stochastic policy
for at most 2,000 steps.  Here all 200 episodes run at once as one device
vector env with autoreset disabled; each env's metrics freeze at its first
terminal step.  ``success_rate`` = finished / episodes (evaluate.py:54) is
the quantity behind "PPO wall-clock to 90% success" (BASELINE.json metric).

Reference quirk kept: gen_tracks(seed=42) draws the FIRST track's parameters
from whatever state the global numpy RNG is in (evaluate.py never seeds it);
``eval_pool`` takes an explicit ``global_seed`` for that draw (default 0) and
restores the caller's RNG state afterwards.

Two backends.  "eager" (the default) steps the episodes from a Python loop: a
torch forward, step_device, a state export and the metric bookkeeping in torch
per step.  "fused" runs the same protocol through rx_eval_steps (include/rx.h,
ABI v25; ``FusedEval``): per step one policy launch, the step's kernels and
one metric kernel, enqueued 50 steps per library call.  Given the same
actions both backends return the same record bit for bit; the fused policy
forward is rx_policy_act's (the torch forward within float rounding) and its
noise is drawn per chunk, so a stochastic fused evaluation samples another,
equally valid stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .track import gen_tracks

BACKENDS = ("eager", "fused")


def eval_pool(num_tracks=40, num_runs=5, seed=42, global_seed=0):
    state = np.random.get_state()
    try:
        np.random.seed(global_seed)
        pool = gen_tracks(num_tracks=num_tracks, seed=seed)
    finally:
        np.random.set_state(state)
    widths = [np.random.RandomState(seed + i).randint(4, 10) for i in range(num_tracks)]
    cps, ws, ids = [], [], []
    for t in range(num_tracks):
        for r in range(num_runs):
            cps.append(pool[t])
            ws.append(widths[r])  # evaluate.py:30 indexes widths by run
            ids.append((t, r))
    return cps, ws, ids


def _flat_policy(agent):
    """The agent's parameters as ONE flat float32 tensor (rx_policy_act layout).
    A module whose parameters already lie back to back in one buffer (rx.optim's
    FlatAdam / FlatParams ran on it) is used in place; any other module is moved
    into such a buffer first (FlatParams: names and state_dict unchanged)."""
    params = list(agent.parameters())
    if not params or any(p.dtype != torch.float32 for p in params):
        raise ValueError("the fused evaluation expects float32 parameters")
    end = params[0].data_ptr()
    packed = True
    for p in params:
        packed = packed and p.is_contiguous() and p.data_ptr() == end and \
            p.untyped_storage().data_ptr() == params[0].untyped_storage().data_ptr()
        end = p.data_ptr() + 4 * p.numel()
    if not packed:
        from .optim import FlatParams
        return FlatParams(agent).flat_param
    return torch.as_strided(params[0].data, (sum(p.numel() for p in params),), (1,))


class FusedEval:
    """rx_eval_steps driver (include/rx.h, ABI v25): the evaluation loop of
    utils/metrics.py:39-78 / 80-150 over every env of ``venv`` at once, ``chunk``
    steps per library call -- per step one rx_policy_act launch (or the caller's
    actions), the step's kernels and k_eval_acc, which keeps the per-episode
    record on the device.  The host looks at one int32 (episodes still running)
    per chunk; 50 is the eager loop's own check interval.

    ``acc`` [N, A, RX_EVAL_W] float64 (columns: rx.h rx_eval_io), ``active`` [N]
    uint8 and ``n_active`` [1] int32 are the record; ``begin()`` resets the envs
    and the record, ``policy_chunk`` / ``actions_chunk`` advance the same
    episodes, ``run_policy`` / ``run_actions`` do a whole evaluation."""

    def __init__(self, venv, chunk=50):
        if chunk <= 0:
            raise ValueError("chunk must be > 0")
        self.L = _lib.load()
        self.venv, self.chunk = venv, int(chunk)
        N, A, dev = venv.num_envs, venv.n_agents, venv.device
        self.acc = torch.zeros((N, A, _lib.RX_EVAL_W), dtype=torch.float64, device=dev)
        self.active = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.n_active = torch.zeros(1, dtype=torch.int32, device=dev)
        self.eps = torch.zeros((self.chunk, N * A, 2), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((self.chunk, N, A, 2), dtype=torch.float32, device=dev)
        self._lp = torch.empty(N * A, dtype=torch.float32, device=dev)
        self._val = torch.empty(N * A, dtype=torch.float32, device=dev)
        self._eps_zero = True

    def begin(self):
        """Reset every env and the record: the state before an evaluation's first step."""
        self.venv.reset_device()
        self.acc.zero_()
        self.active.fill_(1)
        self.n_active.fill_(self.venv.num_envs)

    def _call(self, ev, n):
        v = self.venv
        _lib.check(self.L.rx_eval_steps(v._h, v._io(full=True), ctypes.byref(ev), int(n), _lib.stream_ptr(None)),
                   "rx_eval_steps")
        v._launched(None)
        return int(self.n_active.item())

    def _ev(self, actions, flat=None, log_std=None, prec=0):
        return _lib.RxEvalIO(self.venv.D, int(prec), _lib.ptr(flat), _lib.ptr(log_std),
                             _lib.ptr(self.eps) if flat is not None else None, _lib.ptr(actions),
                             _lib.ptr(self._lp), _lib.ptr(self._val), _lib.ptr(self.acc), _lib.ptr(self.active),
                             _lib.ptr(self.n_active))

    def check_n(self, n):
        if not 0 < n <= self.chunk:
            raise ValueError(f"n={n}: 1 .. {self.chunk}")

    def draw_noise(self, deterministic):
        """The next chunk's noise in ``self.eps``: one normal_() over the whole chunk,
        or zeros (= the mean action), written once and kept while they stay zeros."""
        if not deterministic:
            self.eps.normal_()
        elif not self._eps_zero:
            self.eps.zero_()
        self._eps_zero = bool(deterministic)

    def policy_chunk(self, flat, log_std, n, deterministic=False, prec="fp32"):
        """``n`` <= chunk policy-in-the-loop steps (``draw_noise``); the actions taken are
        in ``self.actions[:n]``.  Returns the number of episodes still running."""
        self.check_n(n)
        self.draw_noise(deterministic)
        return self._call(self._ev(self.actions, flat, log_std, _lib.PRECISION[prec]), n)

    def run_chunks(self, chunk, max_steps, record_actions=False):
        """Reset, then ``chunk(n)`` (n steps -> the episodes still running) until
        ``max_steps`` or until every episode has ended.  Returns the [N, A, RX_EVAL_W]
        record as a numpy array, and with ``record_actions`` also the [T, N, A, 2]
        actions of the T steps executed."""
        self.begin()
        taken, t = [], 0
        while t < max_steps:
            n = min(self.chunk, max_steps - t)
            left = chunk(n)
            if record_actions:
                taken.append(self.actions[:n].clone())
            t += n
            if left == 0:
                break
        rec = self.record()
        return (rec, torch.cat(taken)) if record_actions else rec

    def actions_chunk(self, actions):
        """Open-loop steps of ``actions`` [n, N, A, 2] (contiguous float32 on the env's
        device).  Returns the number of episodes still running."""
        N, A = self.venv.num_envs, self.venv.n_agents
        if actions.dtype != torch.float32 or not actions.is_contiguous() or actions.device != self.acc.device or \
                actions.numel() == 0 or actions.numel() % (N * A * 2):
            raise ValueError(f"actions must be a contiguous float32 device tensor of n x {N}x{A}x2 elements")
        return self._call(self._ev(actions), actions.numel() // (N * A * 2))

    def record(self):
        return self.acc.cpu().numpy()

    @torch.no_grad()
    def run_policy(self, agent, max_steps, deterministic=False, prec="fp32", record_actions=False):
        """One evaluation with ``agent`` in the loop (two-car envs: it drives both
        cars): ``run_chunks`` of ``policy_chunk``."""
        from .ppo_fused import policy_supported
        if prec not in _lib.PRECISION:
            raise ValueError(f"prec={prec!r}: 'fp32' or 'bf16'")
        if not policy_supported(agent, self.venv.D):
            raise ValueError(f"the fused evaluation needs the reference actor-critic layout with 15 or 19 "
                             f"observation columns (this env has {self.venv.D}); use backend='eager'")
        flat = _flat_policy(agent)
        if flat.device != self.acc.device:
            raise ValueError(f"the agent is on {flat.device}, the evaluation env on {self.acc.device}")
        return self.run_chunks(lambda n: self.policy_chunk(flat, agent.log_std, n, deterministic, prec), max_steps,
                               record_actions)

    @torch.no_grad()
    def run_actions(self, actions, max_steps):
        """One open-loop evaluation: step t takes ``actions[t]`` ([T, N, A, 2] or, for
        single-agent envs, [T, N, 2]); stops after min(T, max_steps) steps or when
        every episode has ended.  Returns the record."""
        N, A = self.venv.num_envs, self.venv.n_agents
        a = actions.to(self.acc.device, torch.float32).contiguous().reshape(-1, N, A, 2)
        self.begin()
        T = min(int(max_steps), a.shape[0])
        t = 0
        while t < T:
            n = min(self.chunk, T - t)
            if self.actions_chunk(a[t:t + n]) == 0:
                break
            t += n
        return self.record()


def _summary(total_reward, steps, prog, fin, crash, speed, dist, placement=None):
    """evaluate.py:37-64's summary dict from per-episode numpy arrays."""
    ok = fin
    eff = prog > 0.01
    return {
        "num_episodes": int(len(steps)),
        "num_successful": int(ok.sum()),
        "success_rate": float(ok.mean()),
        "crash_rate": float(crash.mean()),
        "avg_steps": float(steps[ok].mean()) if ok.any() else 0,
        "avg_reward": float(total_reward[ok].mean()) if ok.any() else 0,
        "avg_progress": float(prog[ok].mean()) if ok.any() else 0,
        "avg_speed": float(speed[ok].mean()) if ok.any() else 0,
        "avg_distance": float(dist[ok].mean()) if ok.any() else 0,
        "avg_steps_per_progress": float((steps[eff] / prog[eff]).mean()) if eff.any() else float("nan"),
        "all_episodes": _episodes(total_reward, steps, prog, fin, crash, speed, dist, placement),
    }


def _record_summary(rec):
    """The summary dict from a FusedEval record [N, A, RX_EVAL_W]; two cars: the
    reported car is car 0 unless only car 1 finished (utils/metrics.py:124-131)."""
    N, A = rec.shape[:2]
    flags = rec[:, :, 6].astype(np.uint8)
    fin = (flags & _lib.RX_F_FINISHED) != 0
    crash = (flags & _lib.RX_F_CRASHED) != 0
    pick = (~fin[:, 0] & fin[:, 1]).astype(np.int64) if A == 2 else np.zeros(N, np.int64)
    g = lambda a: a[np.arange(N), pick]  # noqa: E731
    steps = rec[:, 0, 2].astype(np.int64)
    return _summary(g(rec[:, :, 0]), steps, g(rec[:, :, 3]), g(fin), g(crash), g(rec[:, :, 4]), g(rec[:, :, 1]),
                    g(rec[:, :, 5]) if A == 2 else None)


def _check_backend(backend):
    if backend not in BACKENDS:
        raise ValueError(f"backend={backend!r}: one of {BACKENDS}")
    return backend


class Evaluator:
    """Reusable 200-episode evaluation env (evaluate.py protocol).  ``backend``:
    "eager" (the per-step Python loop) or "fused" (FusedEval, rx_eval_steps)."""

    def __init__(self, num_tracks=40, num_runs=5, seed=42, global_seed=0, max_steps=2000, device=None,
                 n_sensors=11, backend="eager"):
        from .vector_env import RacingVectorEnv
        self.backend = _check_backend(backend)
        cps, ws, self.ids = eval_pool(num_tracks, num_runs, seed, global_seed)
        self.max_steps = max_steps
        self.venv = RacingVectorEnv(cps, ws, n_agents=1, n_sensors=n_sensors, device=device, autoreset="disabled")
        self.device = self.venv.device
        self.fused = FusedEval(self.venv) if backend == "fused" else None

    def run_actions(self, actions):
        """Open-loop evaluation of ``actions`` [T, N, 2] (fused backend): the summary dict."""
        if self.fused is None:
            raise ValueError("run_actions needs backend='fused'")
        return _record_summary(self.fused.run_actions(actions, self.max_steps))

    @torch.no_grad()
    def run(self, agent, deterministic=False, record_actions=False, prec="fp32"):
        """utils/metrics.py:39-78 for every episode at once; returns evaluate.py's summary dict
        (fused backend: ``prec`` is the policy kernel's matrix-core precision, and with
        ``record_actions`` the [T, N, 1, 2] actions taken are returned too)."""
        if self.fused is not None:
            out = self.fused.run_policy(agent, self.max_steps, deterministic, prec, record_actions)
            return (_record_summary(out[0]), out[1]) if record_actions else _record_summary(out)
        if record_actions:
            raise ValueError("record_actions needs backend='fused'")
        v = self.venv
        N = v.num_envs
        dev = self.device
        obs = v.reset_device()
        active = torch.ones(N, dtype=torch.bool, device=dev)
        total_reward = torch.zeros(N, dtype=torch.float64, device=dev)
        total_dist = torch.zeros(N, dtype=torch.float64, device=dev)
        steps = torch.zeros(N, dtype=torch.int64, device=dev)
        fin = torch.zeros(N, dtype=torch.bool, device=dev)
        crash = torch.zeros(N, dtype=torch.bool, device=dev)
        prog = torch.zeros(N, dtype=torch.float64, device=dev)
        speed = torch.zeros(N, dtype=torch.float64, device=dev)
        x, y = v.state["x"], v.state["y"]
        px, py = x.clone(), y.clone()
        first = True
        for t in range(self.max_steps):
            if deterministic:
                a = agent.actor_mu(obs).clamp(-1.0, 1.0)
            else:
                a = agent.get_action_and_value(obs)[0]
            obs, _, done = v.step_device(a, full_info=True)
            st = v.state  # writes the stepped state back into x, y, flags (rx_state_export)
            r64 = v.buf["reward64"]
            info = v.buf["info"][:, 0]
            total_reward += torch.where(active, r64, torch.zeros_like(r64))
            if not first:  # metrics.py:59-64: distance between consecutive post-step positions
                d = torch.sqrt((x - px) ** 2 + (y - py) ** 2)
                total_dist += torch.where(active, d, torch.zeros_like(d))
            first = False
            px.copy_(x)
            py.copy_(y)
            steps += active.long()
            fl = st["flags"]
            fin = torch.where(active, (fl & 2) != 0, fin)
            crash = torch.where(active, (fl & 1) != 0, crash)
            prog = torch.where(active, info[:, 1], prog)
            speed = torch.where(active, info[:, 0], speed)
            active &= ~done.bool()
            if t % 50 == 49 and not bool(active.any()):
                break
        fin, crash = fin.cpu().numpy(), crash.cpu().numpy()
        prog, speed = prog.cpu().numpy(), speed.cpu().numpy()
        steps, total_reward, total_dist = steps.cpu().numpy(), total_reward.cpu().numpy(), total_dist.cpu().numpy()
        return _summary(total_reward, steps, prog, fin, crash, speed, total_dist)

    def close(self):
        self.venv.close()


def _episodes(total_reward, steps, prog, fin, crash, speed, dist, placement=None):
    """Per-episode dicts (utils/metrics.py:70-78 / 131-141 keys), evaluate.py's 'all_episodes'."""
    out = []
    for i in range(len(steps)):
        n = int(steps[i])
        m = {"total_reward": float(total_reward[i]), "steps": n, "progress": float(prog[i]),
             "finished": bool(fin[i]), "crashed": bool(crash[i]), "speed": float(speed[i]),
             "total_distance": float(dist[i]), "distance_per_step": float(dist[i]) / n if n > 1 else 0.0}
        if placement is not None:
            m["placement"] = int(placement[i]) if placement[i] > 0 else None
        out.append(m)
    return out


class MultiEvaluator:
    """evaluate.py:68-122 + utils/metrics.py:80-142 (self-play model): every
    two-car episode of the protocol at once, BOTH cars driven by the evaluated
    policy (one batched forward over the 2N car observations per step), at
    most 3,000 steps, stopping at dones['__all__'].  The reported agent is car
    0 unless only car 1 finished (metrics.py:124-131)."""

    def __init__(self, num_tracks=40, num_runs=5, seed=42, global_seed=0, max_steps=3000, device=None,
                 n_sensors=11, env_seed=0, backend="eager"):
        from .vector_env import RacingVectorEnv
        self.backend = _check_backend(backend)
        cps, ws, self.ids = eval_pool(num_tracks, num_runs, seed, global_seed)
        self.max_steps = max_steps
        self.venv = RacingVectorEnv(cps, ws, n_agents=2, n_sensors=n_sensors, device=device, autoreset="disabled",
                                    seed=env_seed)
        self.device = self.venv.device
        self.fused = FusedEval(self.venv) if backend == "fused" else None

    def run_actions(self, actions, max_steps=None):
        """Open-loop evaluation of ``actions`` [T, N, 2, 2] (fused backend): the summary dict.
        ``max_steps`` (default: the evaluator's) ends the loop as metrics.py:92 does: an
        episode still running then has no placement."""
        if self.fused is None:
            raise ValueError("run_actions needs backend='fused'")
        return _record_summary(self.fused.run_actions(actions, self.max_steps if max_steps is None else max_steps))

    @torch.no_grad()
    def run(self, agent, record_actions=False, prec="fp32"):
        """backend "fused", ``record_actions``: also returns the [T, N, 2, 2] actions taken."""
        if self.fused is not None:
            out = self.fused.run_policy(agent, self.max_steps, False, prec, record_actions)
            return (_record_summary(out[0]), out[1]) if record_actions else _record_summary(out)
        if record_actions:
            raise ValueError("record_actions needs backend='fused'")
        v = self.venv
        N, D = v.num_envs, v.D
        dev = self.device
        obs = v.reset_device()
        active = torch.ones(N, dtype=torch.bool, device=dev)
        total_reward = torch.zeros((N, 2), dtype=torch.float64, device=dev)
        total_dist = torch.zeros((N, 2), dtype=torch.float64, device=dev)
        steps = torch.zeros(N, dtype=torch.int64, device=dev)
        info_last = torch.zeros((N, 2, 4), dtype=torch.float64, device=dev)
        flags_last = torch.zeros((N, 2), dtype=torch.uint8, device=dev)
        x, y = v.state["x"].view(N, 2), v.state["y"].view(N, 2)
        px, py = x.clone(), y.clone()
        first = True
        for t in range(self.max_steps):
            a = agent.get_action_and_value(obs.reshape(2 * N, D))[0].reshape(N, 2, 2)
            obs, _, done = v.step_device(a, full_info=True)
            st = v.state  # writes the stepped state back into x, y, flags (rx_state_export)
            act2 = active.unsqueeze(1)
            total_reward += torch.where(act2, v.buf["reward64"], torch.zeros_like(total_reward))
            if not first:
                d = torch.sqrt((x - px) ** 2 + (y - py) ** 2)
                total_dist += torch.where(act2, d, torch.zeros_like(d))
            first = False
            px.copy_(x)
            py.copy_(y)
            steps += active.long()
            info_last = torch.where(act2.unsqueeze(2), v.buf["info"], info_last)
            flags_last = torch.where(act2, st["flags"].view(N, 2), flags_last)
            active &= ~done.bool()
            if t % 50 == 49 and not bool(active.any()):
                break
        fin = (flags_last & 2) != 0
        crash = (flags_last & 1) != 0
        pick = (~fin[:, 0] & fin[:, 1]).long()  # car 1 only if it finished and car 0 did not
        ar = torch.arange(N, device=dev)
        g = lambda t: t[ar, pick].cpu().numpy()  # noqa: E731
        fin_c, crash_c = g(fin), g(crash)
        prog, speed, place = g(info_last[:, :, 1]), g(info_last[:, :, 0]), g(info_last[:, :, 3])
        rew, dist = g(total_reward), g(total_dist)
        steps = steps.cpu().numpy()
        return _summary(rew, steps, prog, fin_c, crash_c, speed, dist, place)

    def close(self):
        self.venv.close()
