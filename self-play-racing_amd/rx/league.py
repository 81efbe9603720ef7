"""League play: which of two policies is the better racer?

``SelfPlayPPO`` trains against a pool of frozen snapshots, and the evaluators
(rx.evaluate, the reference's evaluate.py:68-122) put ONE policy into both cars.
Here policy A drives car 0 and policy B car 1 of the same two-car episode:

``PolicyBank``   P policies' flat parameters side by side in one device tensor;
``seating``      the [episodes, 2] table "which bank member drives which car";
``League``       every pairing x the evaluation protocol (eval_pool: 40 tracks x
                 5 runs) as ONE two-car vector env, stepped by rx_match_steps
                 (include/rx.h): per step one rx_policy_act_bank launch in which
                 every row picks its weights from the bank, the step's kernels
                 and k_eval_acc;
``LeagueResult`` the raw per-car record, and from it the games / wins / draws
                 matrices, per-policy rates and Bradley-Terry ratings.

Who wins: the env ranks both cars when the episode ends (MultiRacingEnv.place,
multi_racing_env.py:198-211: finished, then progress, then not crashed, then the
earlier finish) and k_eval_acc keeps the terminal step's placement in the record;
the car whose placement is 1 wins.  An episode the league's ``max_steps`` cut
before the env ended it has no placement: a draw.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

PARAM_KEYS = tuple(f"{net}.{i}.{k}" for net in ("actor_mu", "critic") for i in (0, 2, 4) for k in ("weight", "bias"))
STRIDE_ALIGN = 64  # floats: every policy's parameters start on a 256-byte boundary
ELO_CLAMP = 1200.0  # ratings(): the bound on an unbeaten / winless policy's distance from its opponents' mean


class PolicyBank:
    """P policies for rx_policy_act_bank / rx_match_steps: ``params`` float32
    [P, stride] (row p = rx.evaluate._flat_policy of policy p, zero padding up to
    ``stride``, a multiple of 64 floats) and ``log_std`` float32 [P, 2], each one
    contiguous tensor on ``device``.

    ``policies``: Agent modules or their state dicts (the keys of rx.agent.Agent).
    The modules are copied, never re-laid.  Refused (ValueError): an empty list, a
    module rx.ppo_fused.policy_supported refuses (another layout or observation
    width), mixed observation widths, parameters that are not float32."""

    def __init__(self, policies, device=None):
        policies = list(policies)
        if not policies:
            raise ValueError("PolicyBank needs at least one policy")
        rows, stds, dims = [], [], []
        for k, pol in enumerate(policies):
            flat, ls, D = self._row(pol, k)
            rows.append(flat)
            stds.append(ls)
            dims.append(D)
        if len(set(dims)) != 1:
            raise ValueError(f"PolicyBank: mixed observation widths {dims}")
        self.obs_dim = dims[0]
        self.n_policies = len(rows)
        self.n_params = int(rows[0].numel())
        self.stride = (self.n_params + STRIDE_ALIGN - 1) // STRIDE_ALIGN * STRIDE_ALIGN
        dev = torch.device(device) if device is not None else rows[0].device
        self.params = torch.zeros((self.n_policies, self.stride), dtype=torch.float32, device=dev)
        self.log_std = torch.zeros((self.n_policies, 2), dtype=torch.float32, device=dev)
        for p in range(self.n_policies):
            self.params[p, :self.n_params].copy_(rows[p])
            self.log_std[p].copy_(stds[p])
        self.device = dev

    @staticmethod
    def _row(pol, k):
        """(flat float32 parameters in module.parameters() order, log_std [2], D) of one policy."""
        from .ppo_fused import policy_supported
        if isinstance(pol, torch.nn.Module):
            params = [p.detach() for p in pol.parameters()]
            if not params or params[0].dim() != 2 or not hasattr(pol, "log_std"):
                raise ValueError(f"PolicyBank: policy {k} does not have the reference actor-critic layout")
            if any(p.dtype != torch.float32 for p in params) or pol.log_std.dtype != torch.float32:
                raise ValueError(f"PolicyBank: policy {k} has parameters that are not float32")
            D = int(params[0].shape[1])
            if not policy_supported(pol, D):
                raise ValueError(f"PolicyBank: policy {k} does not have the reference actor-critic layout with 15 "
                                 f"or 19 observation columns (its first layer reads {D})")
            ls = pol.log_std.detach()
        else:
            missing = [key for key in PARAM_KEYS + ("log_std",) if key not in pol]
            if missing:
                raise ValueError(f"PolicyBank: policy {k}'s state dict lacks {missing}")
            params = [torch.as_tensor(pol[key]).detach() for key in PARAM_KEYS]
            ls = torch.as_tensor(pol["log_std"]).detach()
            if any(p.dtype != torch.float32 for p in params) or ls.dtype != torch.float32:
                raise ValueError(f"PolicyBank: policy {k} has parameters that are not float32")
            D = int(params[0].shape[1]) if params[0].dim() == 2 else -1
            n = sum(p.numel() for p in params)
            if D not in (15, 19) or n != _lib.load().rx_ppo_n_params(D):
                raise ValueError(f"PolicyBank: policy {k} does not have the reference actor-critic layout with 15 "
                                 f"or 19 observation columns (its first layer reads {D}, {n} parameters)")
        if ls.numel() != 2:
            raise ValueError(f"PolicyBank: policy {k}'s log_std has {ls.numel()} entries, not 2")
        return torch.cat([p.reshape(-1) for p in params]), ls.reshape(2), D

    @classmethod
    def from_checkpoint(cls, path_or_dict, device=None):
        """The bank of a SelfPlayPPO checkpoint (save_checkpoint / load_checkpoint's
        dict, or the path of one): ``agent_state_dict`` first, then ``opponent_pool``
        in order."""
        ck = path_or_dict
        if isinstance(ck, (str, os.PathLike)):
            ck = torch.load(ck, map_location="cpu", weights_only=True)
        if "agent_state_dict" not in ck:
            raise ValueError("not a self-play checkpoint: no 'agent_state_dict'")
        return cls([ck["agent_state_dict"]] + list(ck.get("opponent_pool", [])), device=device)

    def to(self, device):
        dev = torch.device(device)
        if dev != self.params.device:
            self.params, self.log_std, self.device = self.params.to(dev), self.log_std.to(dev), dev
        return self

    def __len__(self):
        return self.n_policies


def _pairs(pairs, n_policies):
    a = np.asarray(pairs, dtype=np.int64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] == 0:
        raise ValueError("pairs: a non-empty list of (car 0's policy, car 1's policy)")
    if a.min() < 0 or (n_policies is not None and a.max() >= n_policies):
        hi = "" if n_policies is None else f" .. {n_policies - 1}"
        raise ValueError(f"pairs: policy indices must lie in 0{hi}, got {int(a.min())} .. {int(a.max())}")
    return a


def all_pairs(n_policies):
    """Every ordered pair i != j: both seatings of every pairing."""
    return [(i, j) for i in range(n_policies) for j in range(n_policies) if i != j]


def seating(pairs, episodes, n_policies=None):
    """The seat table of ``episodes`` episodes per pairing: int32 [n_pairs * episodes,
    2], row e = (car 0's policy, car 1's policy), each pairing's episodes contiguous
    -- so of rx_policy_act_bank's tiles (one car of 16 consecutive envs) at most one
    per car and pairing boundary holds two policies.  Indices below 0 (or, with
    ``n_policies``, beyond the bank) raise ValueError."""
    if int(episodes) <= 0:
        raise ValueError("episodes must be > 0")
    return np.ascontiguousarray(np.repeat(_pairs(pairs, n_policies), int(episodes), axis=0).astype(np.int32))


def bradley_terry(wins, draws=None, iters=10000, tol=1e-12):
    """Bradley-Terry strengths on the Elo scale from ``wins`` [P, P] (wins[i, j] =
    games i won against j) and symmetric ``draws`` [P, P] (a draw is half a win to
    each side).  Float64 NumPy, the MM iteration (Hunter 2004)
        s_i <- W_i / sum_j n_ij / (s_i + s_j),   W_i = i's wins, n_ij = games of i and j,
    renormalised to geometric mean 1 after each sweep, at most ``iters`` = 10,000
    sweeps, stopping when no log-strength moves by more than ``tol`` = 1e-12.
    Returned: 400 log10 s, shifted to mean 0.

    Clamp: the maximum-likelihood strength of a policy that never scored a point is
    0, of one that never lost one infinite.  So first every policy without a point is
    granted half a win, then every policy still without a lost point half a loss,
    each as virtual games spread over its opponents in proportion to the games
    played against them; the iteration then has a finite fixed point whenever the
    results connect the policies, and the rating is finally limited to +-1200 Elo
    around the mean (ELO_CLAMP), which also bounds a league whose results split
    into groups that never lost to each other.  A policy with no games gets the
    mean of the others before the shift."""
    w = np.array(wins, dtype=np.float64)
    P = w.shape[0]
    if w.ndim != 2 or w.shape != (P, P):
        raise ValueError("wins must be a square matrix")
    if draws is not None:
        w = w + 0.5 * np.asarray(draws, dtype=np.float64)
    np.fill_diagonal(w, 0.0)
    n0 = w + w.T                     # games per pairing
    tot = n0.sum(1)
    played = tot > 0
    share = np.divide(n0, tot[:, None], out=np.zeros_like(n0), where=played[:, None])
    for i in np.nonzero(played & (w.sum(1) == 0))[0]:
        w[i, :] += 0.5 * share[i]
    for i in np.nonzero(played & (w.sum(0) == 0))[0]:
        w[:, i] += 0.5 * share[i]
    n = w + w.T
    W = w.sum(1)
    logs = np.zeros(P)
    for _ in range(int(iters)):
        s = np.exp(logs)
        den = (n / (s[:, None] + s[None, :])).sum(1)
        new = np.zeros(P)
        new[played] = np.log(W[played] / den[played])
        if played.any():
            new[played] -= new[played].mean()
        moved = np.abs(new - logs).max()
        logs = new
        if moved <= tol:
            break
    elo = 400.0 / np.log(10.0) * logs
    elo -= elo.mean()
    return np.clip(elo, -ELO_CLAMP, ELO_CLAMP)


class LeagueResult:
    """``record`` float64 [N, 2, RX_EVAL_W] (rx.h rx_eval_io.acc: 0 total_reward, 2
    steps, 3 progress, 5 placement, 6 flags, ...) and ``seat`` int32 [N, 2] of one
    league run over ``n_policies`` policies.  Derived, all NumPy:

    games[i, j]   episodes with i in car 0 and j in car 1;
    wins[i, j]    episodes (either seating) in which i beat j: i's placement is 1;
    draws[i, j]   episodes of i and j (either seating, symmetric) in which no car
                  has a placement -- the step limit cut the episode;
    finish_rate, crash_rate, mean_reward   per policy over all its cars."""

    def __init__(self, record, seat, n_policies, names=None):
        self.record = np.asarray(record, dtype=np.float64)
        self.seat = np.asarray(seat, dtype=np.int32)
        N = self.seat.shape[0]
        if self.record.shape != (N, 2, _lib.RX_EVAL_W) or self.seat.shape != (N, 2):
            raise ValueError(f"record {self.record.shape} / seat {self.seat.shape}: [N, 2, {_lib.RX_EVAL_W}] and [N, 2]")
        P = self.n_policies = int(n_policies)
        if N and (self.seat.min() < 0 or self.seat.max() >= P):
            raise ValueError(f"seat: policy indices must lie in 0 .. {P - 1}")
        self.names = list(names) if names is not None else [str(p) for p in range(P)]
        s0, s1 = self.seat[:, 0].astype(np.int64), self.seat[:, 1].astype(np.int64)
        place = self.record[:, :, 5]
        self.games = np.zeros((P, P), np.int64)
        self.wins = np.zeros((P, P), np.int64)
        self.draws = np.zeros((P, P), np.int64)
        np.add.at(self.games, (s0, s1), 1)
        np.add.at(self.wins, (s0, s1), place[:, 0] == 1)
        np.add.at(self.wins, (s1, s0), place[:, 1] == 1)
        drawn = (place[:, 0] != 1) & (place[:, 1] != 1)
        np.add.at(self.draws, (s0, s1), drawn)
        np.add.at(self.draws, (s1, s0), drawn & (s0 != s1))
        flags = self.record[:, :, 6].astype(np.uint8)
        cars = np.bincount(self.seat.reshape(-1), minlength=P).astype(np.float64)

        def per_policy(v):
            tot = np.bincount(self.seat.reshape(-1), weights=np.asarray(v, np.float64).reshape(-1), minlength=P)
            return np.divide(tot, cars, out=np.zeros(P), where=cars > 0)
        self.finish_rate = per_policy((flags & _lib.RX_F_FINISHED) != 0)
        self.crash_rate = per_policy((flags & _lib.RX_F_CRASHED) != 0)
        self.mean_reward = per_policy(self.record[:, :, 0])

    def ratings(self):
        """bradley_terry(wins, draws) -- see there for the iteration, its stopping rule and the clamp."""
        off = ~np.eye(self.n_policies, dtype=bool)
        return bradley_terry(self.wins * off, self.draws * off)

    def table(self):
        """One dict per policy, best rating first."""
        r = self.ratings()
        g = self.games + self.games.T
        off = ~np.eye(self.n_policies, dtype=bool)
        rows = [{"policy": p, "name": self.names[p], "rating": float(r[p]), "games": int((g * off)[p].sum()),
                 "wins": int((self.wins * off)[p].sum()), "losses": int((self.wins * off)[:, p].sum()),
                 "draws": int((self.draws * off)[p].sum()), "finish_rate": float(self.finish_rate[p]),
                 "crash_rate": float(self.crash_rate[p]), "mean_reward": float(self.mean_reward[p])}
                for p in range(self.n_policies)]
        return sorted(rows, key=lambda d: (-d["rating"], d["policy"]))

    def to_json(self):
        return {"n_policies": self.n_policies, "names": self.names, "episodes": int(self.seat.shape[0]),
                "games": self.games.tolist(), "wins": self.wins.tolist(), "draws": self.draws.tolist(),
                "ratings": self.ratings().tolist(), "table": self.table()}

    def format(self):
        lines = [f"{'#':>2} {'policy':<12} {'rating':>8} {'games':>6} {'wins':>6} {'losses':>6} {'draws':>6} "
                 f"{'finish':>7} {'crash':>7} {'reward':>9}"]
        for k, d in enumerate(self.table()):
            lines.append(f"{k + 1:>2} {d['name']:<12} {d['rating']:>8.1f} {d['games']:>6} {d['wins']:>6} "
                         f"{d['losses']:>6} {d['draws']:>6} {d['finish_rate']:>7.3f} {d['crash_rate']:>7.3f} "
                         f"{d['mean_reward']:>9.2f}")
        return "\n".join(lines)


class Match:
    """rx_match_steps driver over one two-car (or single-agent) vector env: the
    record buffers of rx.evaluate.FusedEval plus the bank and the seat table.
    ``seat`` int32 [N, A] (host array), refused unless every entry names a bank
    member: the kernel cannot check device memory, it only skips such rows."""

    def __init__(self, venv, chunk=50):
        from .evaluate import FusedEval
        self.fe = FusedEval(venv, chunk)
        self.venv, self.chunk = venv, self.fe.chunk
        self.seat = torch.zeros((venv.num_envs, venv.n_agents), dtype=torch.int32, device=venv.device)

    def set_seat(self, seat, n_policies):
        N, A = self.venv.num_envs, self.venv.n_agents
        s = np.asarray(seat)
        if s.shape != (N, A) or s.dtype.kind not in "iu":
            raise ValueError(f"seat must be an integer [{N}, {A}] array, got {s.dtype} {s.shape}")
        if s.min() < 0 or s.max() >= n_policies:
            raise ValueError(f"seat: policy indices must lie in 0 .. {n_policies - 1}, got {int(s.min())} .. "
                             f"{int(s.max())}")
        self.seat.copy_(torch.from_numpy(np.ascontiguousarray(s.astype(np.int32))))

    def begin(self):
        self.fe.begin()

    def steps(self, bank, n, deterministic=False, prec="fp32"):
        """``n`` <= chunk steps (noise: ``FusedEval.draw_noise``); the actions taken are
        in ``self.fe.actions[:n]``.  Returns the number of episodes still running."""
        fe, v = self.fe, self.venv
        fe.check_n(n)
        if prec not in _lib.PRECISION:
            raise ValueError(f"prec={prec!r}: 'fp32' or 'bf16'")
        if bank.obs_dim != v.D:
            raise ValueError(f"the bank's policies read {bank.obs_dim} observation columns, the env has {v.D}")
        if bank.params.device != fe.acc.device:
            raise ValueError(f"the bank is on {bank.params.device}, the env on {fe.acc.device}")
        fe.draw_noise(deterministic)
        m = _lib.RxMatchIO(v.D, _lib.PRECISION[prec], _lib.ptr(bank.params), _lib.ptr(bank.log_std), _lib.ptr(fe.eps),
                           _lib.ptr(fe.actions), _lib.ptr(fe._lp), _lib.ptr(fe._val), _lib.ptr(fe.acc),
                           _lib.ptr(fe.active), _lib.ptr(fe.n_active), bank.n_policies, 0, bank.stride,
                           _lib.ptr(self.seat))
        _lib.check(fe.L.rx_match_steps(v._h, v._io(full=True), ctypes.byref(m), int(n), _lib.stream_ptr(None)),
                   "rx_match_steps")
        v._launched(None)
        return int(fe.n_active.item())

    @torch.no_grad()
    def run(self, bank, max_steps, deterministic=False, prec="fp32", record_actions=False):
        """Reset, then step until ``max_steps`` or until every episode has ended.  Returns
        the [N, A, RX_EVAL_W] record (and with ``record_actions`` the [T, N, A, 2] actions)."""
        return self.fe.run_chunks(lambda n: self.steps(bank, n, deterministic, prec), max_steps, record_actions)


class League:
    """Head-to-head tables over rx.evaluate.eval_pool's protocol (``num_tracks``
    tracks x ``num_runs`` runs per pairing, evaluate.py:12-122's tracks and
    widths).  ``play`` seats every pairing in its own block of episodes of ONE
    two-car env (autoreset disabled; built once per pair count and kept) and steps
    all of them together, 50 steps per rx_match_steps call with one normal_() per
    chunk, as rx.evaluate.FusedEval does."""

    def __init__(self, num_tracks=40, num_runs=5, seed=42, global_seed=0, max_steps=3000, n_sensors=11, env_seed=0,
                 device=None):
        self.pool_args = (num_tracks, num_runs, seed, global_seed)
        self.episodes = int(num_tracks) * int(num_runs)
        self.max_steps, self.n_sensors, self.env_seed, self.device = int(max_steps), n_sensors, env_seed, device
        self._matches = {}

    def _match(self, n_pairs):
        m = self._matches.get(n_pairs)
        if m is None:
            from .evaluate import eval_pool
            from .vector_env import RacingVectorEnv
            cps, ws, _ = eval_pool(*self.pool_args)
            venv = RacingVectorEnv(cps * n_pairs, ws * n_pairs, n_agents=2, n_sensors=self.n_sensors,
                                   device=self.device, autoreset="disabled", seed=self.env_seed)
            m = self._matches[n_pairs] = Match(venv)
        return m

    def play(self, bank, pairs=None, deterministic=False, prec="fp32", record_actions=False):
        """``pairs``: (car 0's policy, car 1's policy) per pairing; None = every ordered
        pair i != j, so both seatings are played (the env's start-side draw already
        randomises the grid side per reset).  Returns a LeagueResult (and with
        ``record_actions`` the [T, N, 2, 2] actions).  Every play resets the env, and
        every reset draws the start sides anew: a second play of the same League is
        another sample even with ``deterministic``; an identically built League
        repeats the first one's."""
        if pairs is None:
            pairs = all_pairs(bank.n_policies)
        if prec not in _lib.PRECISION:
            raise ValueError(f"prec={prec!r}: 'fp32' or 'bf16'")
        seat = seating(pairs, self.episodes, bank.n_policies)  # refuses out-of-range indices before any upload
        m = self._match(len(pairs))
        bank.to(m.venv.device)
        m.set_seat(seat, bank.n_policies)
        out = m.run(bank, self.max_steps, deterministic, prec, record_actions)
        res = LeagueResult(out[0] if record_actions else out, seat, bank.n_policies)
        return (res, out[1]) if record_actions else res

    def close(self):
        for m in self._matches.values():
            m.venv.close()
        self._matches = {}
