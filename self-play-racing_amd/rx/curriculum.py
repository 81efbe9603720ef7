"""Track curriculum: per-track tallies and prioritised draws on the device.

``PPO.resample_tracks`` throws the whole pool away and draws a new one blindly,
env i always runs slot i % n, and the only training statistics are three global
sums.  Here every finished episode is counted against its track slot where it
happens (one small kernel per rollout step), and at every
``config["track_resample_every"]`` boundary the envs are redrawn over the slots,
weighted towards the tracks the learner still fails -- a pool-level form of
prioritised level replay; optionally the mastered slots are retired for fresh
tracks.  The rollout stays one library call (rx_track_rollout_steps,
include/rx.h) that a HIP graph can record.

``TrackCurriculum``        the device tensors (tally, cdf, p, track_of_env) and
                           the three kernels (rx_track_tally / _scores / _draw);
``CurriculumStepRollout``  ppo_fused.StepRollout on rx_track_rollout_steps;
``CurriculumPPO``          the trainer: PPO with the tally in the rollout and the
                           prioritised ``resample_tracks``.

The rules (tally, scores, draw) are csrc/rx_curriculum.h; DESIGN.md §4.

Episodes in flight at a reassignment are dropped untallied (``set_tracks``'
semantics), which biases the tallies against long episodes: keep
``track_resample_every * num_steps`` well above an episode's length.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import dist as rdist
from .ppo import PPO
from .ppo_fused import StepRollout

PROGRESS_Q = 1048576.0  # progress_q's fixed point (csrc/rx_curriculum.h)


def _score_id(score):
    if score not in _lib.TRACK_SCORES:
        raise ValueError(f"curriculum score must be one of {sorted(_lib.TRACK_SCORES)}, got {score!r}")
    return _lib.TRACK_SCORES[score]


def check_rules(power, mix, prior, score):
    """The ranges rx_track_scores / rx_track_draw accept, as ValueErrors naming the config key."""
    if not 0 <= int(power) <= _lib.RX_TRACK_MAX_POWER:
        raise ValueError(f"curriculum_power={power} outside 0..{_lib.RX_TRACK_MAX_POWER}")
    if not 0.0 <= float(mix) <= 1.0:
        raise ValueError(f"curriculum_mix={mix} outside [0, 1]")
    if not float(prior) > 0.0:
        raise ValueError(f"curriculum_prior={prior} must be > 0")
    return int(power), float(mix), float(prior), _score_id(score)


def host_fresh_tracks(seed, generation, n):
    """``n`` fresh host tracks for the slots a resample at ``generation`` retires ->
    (control points, widths): ``gen_tracks(seed=None)`` and one ``randint(6, 10)`` width
    each from ``RandomState(seed + 7919 * generation)``, so np.random does not move."""
    from .track import gen_tracks
    rng = np.random.RandomState((seed + 7919 * generation) % 2 ** 32)
    cps = gen_tracks(n, seed=None, rng=rng)
    return cps, [int(rng.randint(6, 10)) for _ in range(n)]


def mastered_slots(episodes, p, refresh, mastery, min_episodes):
    """Up to floor(refresh * n_tracks) slots with at least ``min_episodes`` episodes and p
    at least ``mastery``, highest p first, ties by slot (host arrays of one scores call)."""
    budget = int(math.floor(refresh * len(p)))
    if budget <= 0:
        return np.zeros(0, dtype=np.int64)
    ok = np.nonzero((episodes >= min_episodes) & (p >= mastery))[0]
    return ok[np.lexsort((ok, -p[ok]))][:budget].astype(np.int64)


class TrackCurriculum:
    """The tallies of ``venv``'s track slots and the draw of its envs over them.

    ``tally`` int64 [n_tracks, 4] = (episodes, finishes, crashes, progress_q),
    ``cdf`` int64 [n_tracks], ``p`` float64 [n_tracks], ``track_of_env`` int32 [N]:
    device tensors at fixed addresses, so one struct serves every call and any
    captured graph.  The slot of env e is read from the env's bound ``track`` array,
    which rx_assign rewrites in place."""

    def __init__(self, venv, seed, power=1, mix=0.1, prior=1.0, score="fail"):
        if venv.n_agents != 1:
            raise ValueError("the track curriculum tallies single-agent envs only (DESIGN.md §8)")
        self.power, self.mix, self.prior, self.score = check_rules(power, mix, prior, score)
        self.L = _lib.load()
        self.venv, self.seed = venv, int(seed) & (2**64 - 1)
        self.n_tracks = len(venv._table) if venv._table is not None else len(venv.tracks)
        n, dev = venv.num_envs, venv.device
        self.tally = torch.zeros((self.n_tracks, _lib.RX_TRACK_TALLY_W), dtype=torch.int64, device=dev)
        self.cdf = torch.zeros(self.n_tracks, dtype=torch.int64, device=dev)
        self.p = torch.full((self.n_tracks,), 0.5, dtype=torch.float64, device=dev)
        self.track_of_env = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tc = _lib.RxTrackIO(self.n_tracks, self.score, _lib.ptr(venv._st["track"]), _lib.ptr(self.tally),
                                 _lib.ptr(self.cdf), _lib.ptr(self.p), _lib.ptr(self.track_of_env), self.seed)

    def tally_step(self, done=None, stream=None):
        """Count the envs whose episode ended in the step just enqueued (rx_track_tally on
        the env's own terminated / info rows; ``done``: the step's done row when it went
        into a rollout buffer).  The step must have run with ``full_info=True``."""
        b = self.venv.buf
        _lib.check(self.L.rx_track_tally(ctypes.byref(self.tc), self.venv.num_envs,
                                         _lib.ptr(b["done_f32"] if done is None else done), _lib.ptr(b["terminated"]),
                                         _lib.ptr(b["info"]), _lib.stream_ptr(stream)), "rx_track_tally")

    def episodic(self):
        """The episodic draw's io (rx_track_episode_io), made on first use: ``draws``
        int32 [N] (the bits of the library's uint32 counters), zero-filled, at a fixed
        address like the other tensors.  The handle-bound calls use the handle's own
        wave-order arrays, so env_pos / pos_slot stay null here."""
        if getattr(self, "ep", None) is None:
            self.draws = torch.zeros(self.venv.num_envs, dtype=torch.int32, device=self.venv.device)
            self.ep = _lib.RxTrackEpisodeIO(_lib.ptr(self.draws), None, None, None, self.mix)
        return self.ep

    def episode_step(self, done=None, stream=None):
        """``tally_step`` plus the episodic draw (rx_track_episode_step): every env whose
        episode ended in the step just enqueued is tallied and takes its next slot from
        the table ``scores`` left, which the next step resets it on.  Lane-varying
        handles with next-step autoreset only; the step must have run with
        ``full_info=True``."""
        ep, v = self.episodic(), self.venv
        _lib.check(self.L.rx_track_episode_step(v._h, ctypes.byref(self.tc), ctypes.byref(ep), v._io_info(),
                                                _lib.ptr(v.buf["done_f32"] if done is None else done),
                                                _lib.stream_ptr(stream)), "rx_track_episode_step")
        v._track_ids_stale = True  # the device moved envs between slots: track_ids() downloads them

    def scores(self, stream=None):
        """tallies -> ``p`` and the integer sampling table ``cdf`` (rx_track_scores)."""
        _lib.check(self.L.rx_track_scores(ctypes.byref(self.tc), self.power, self.prior, _lib.stream_ptr(stream)),
                   "rx_track_scores")

    def draw(self, generation, stream=None):
        """A slot for every env from the current table (rx_track_draw) -> ``track_of_env``."""
        _lib.check(self.L.rx_track_draw(ctypes.byref(self.tc), self.venv.num_envs, int(generation) & 0xFFFFFFFF,
                                        self.mix, _lib.stream_ptr(stream)), "rx_track_draw")
        return self.track_of_env

    def reset_slots(self, idx):
        """Zero the tallies of the slots ``idx`` (their tracks were replaced)."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size:
            if idx.min() < 0 or idx.max() >= self.n_tracks:
                raise ValueError(f"slots must lie in [0, {self.n_tracks})")
            self.tally[torch.from_numpy(idx).to(self.tally.device)] = 0

    def table(self):
        """The host view per slot, arrays of length n_tracks: episodes, finishes,
        crashes, mean_progress (NaN before the first episode), p, prob (the draw
        probability of the slot under the current tallies).  Runs ``scores`` and
        downloads; call it between updates."""
        self.scores()
        t = self.tally.cpu().numpy()
        cdf = self.cdf.cpu().numpy().astype(np.uint64)
        w = np.diff(np.concatenate([[np.uint64(0)], cdf])).astype(np.float64)
        n, F = self.n_tracks, float(cdf[-1])
        prob = np.full(n, 1.0 / n) if F == 0 else (1.0 - self.mix) * (w / F) + self.mix / n
        ep = t[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_progress = np.where(ep > 0, t[:, 3] / PROGRESS_Q / ep, np.nan)
        return {"episodes": t[:, 0].copy(), "finishes": t[:, 1].copy(), "crashes": t[:, 2].copy(),
                "mean_progress": mean_progress, "p": self.p.cpu().numpy(), "prob": prob}


class CurriculumStepRollout(StepRollout):
    """rx_track_rollout_steps driver: the single-agent rollout loop with one
    rx_track_tally after every step.  The step runs with the env's terminated and
    info rows, which the tally reads; every rollout output equals StepRollout's bit
    for bit (tests/test_curriculum_gpu.py).  Every address handed to the library is
    fixed, so a captured graph of the call stays valid until the tracks are swapped."""

    FN = "rx_track_rollout_steps"

    def __init__(self, agent, flat, venv, T, curriculum, prec=_lib.RX_PREC_FP32):
        super().__init__(agent, flat, venv, T, prec)
        self.curriculum = curriculum

    def _enqueue(self, args, stream):
        _lib.check(self.L.rx_track_rollout_steps(self.venv._h, self.venv._io_info(), *args,
                                                 ctypes.byref(self.curriculum.tc), self.prec, stream), self.FN)


class CurriculumPPO(PPO):
    """PPO that tallies every finished episode against its track slot and, every
    ``config["track_resample_every"]`` updates, redraws the envs over the slots
    weighted towards the tracks it still fails.

    Config keys (defaults): ``curriculum_power`` 1, ``curriculum_mix`` 0.1,
    ``curriculum_prior`` 1.0, ``curriculum_score`` "fail" (or "potential"),
    ``curriculum_refresh`` 0.25 (the largest fraction of the slots retired per
    resample), ``curriculum_mastery`` 0.8 and ``curriculum_min_episodes`` 4 (a slot
    is retired once it has that many episodes and p at least the mastery).  With
    ``track_resample_every`` 0 it only tallies: ``track_table()`` still answers
    which tracks fail.

    The slots are the distinct (control points, width) pairs the envs were built
    on.  The rollout always goes through rx_track_rollout_steps or the per-step
    loop; the persistent small-N rollout (``fused_rollout``) does not tally and is
    bypassed.

    Refused (ValueError): a world size above 1 (per-rank tallies would need an
    all-reduce) and two-car envs."""

    def __init__(self, env_fn, config, device="cuda"):
        if rdist.world() > 1:
            raise ValueError("CurriculumPPO needs world size 1: the per-track tallies are per rank and the "
                             "sampling table would need their all-reduce (DESIGN.md §8)")
        c = config
        self._rules = check_rules(c.get("curriculum_power", 1), c.get("curriculum_mix", 0.1),
                                  c.get("curriculum_prior", 1.0), c.get("curriculum_score", "fail"))
        self.refresh = float(c.get("curriculum_refresh", 0.25))
        self.mastery = float(c.get("curriculum_mastery", 0.8))
        self.min_episodes = int(c.get("curriculum_min_episodes", 4))
        if not 0.0 <= self.refresh <= 1.0:
            raise ValueError(f"curriculum_refresh={self.refresh} outside [0, 1]")
        # one spec, built and dropped with np.random put back: a train.py env_fn may draw its track id there
        state = np.random.get_state()
        spec = env_fn(0)
        np.random.set_state(state)
        if getattr(spec, "num_agents", 1) != 1:
            raise ValueError("CurriculumPPO trains single-agent envs: two-car envs are not tallied per track "
                             "(DESIGN.md §8)")
        super().__init__(env_fn, config, device)
        if not hasattr(self.envs, "reassign_tracks") or self.envs.n_agents != 1:
            raise ValueError("CurriculumPPO needs a single-agent RacingVectorEnv")
        geoms = self.envs.tracks.geoms
        self._cps = [g.control_points for g in geoms]
        self._widths = [g.track_width for g in geoms]
        power, mix, prior, _ = self._rules
        self.curriculum = TrackCurriculum(self.envs, c["seed"], power, mix, prior, c.get("curriculum_score", "fail"))
        self.retired = []  # the slots each resample replaced, oldest first

    # ------------------------------------------------------------ rollout
    def _fused_rollout(self, T):
        return None  # k_rollout does not tally

    def _step_rollout(self, obs):
        from . import ppo_fused
        c = self.config
        if self._fused_policy(obs) is None or not StepRollout.supported(self.envs, self.agent, c):
            return None
        T, prec = obs.shape[0], ppo_fused.precision(c)
        sr = self.__dict__.get("_tc_steps_rollout")
        if sr is None or sr.T != T or sr.n != self.envs.num_envs or sr.prec != prec:
            sr = self._tc_steps_rollout = self._make_step_rollout(T, prec)
        return sr

    def _make_step_rollout(self, T, prec):
        """The rollout driver; with ``_after_step`` the two places a subclass changes what follows a step."""
        return CurriculumStepRollout(self.agent, self._flat, self.envs, T, self.curriculum, prec)

    def _after_step(self, done):
        """The per-step loop's launch after every step: the tally of its done row."""
        self.curriculum.tally_step(done)

    def _rollout_body(self, obs, actions, logprobs, dones, rewards, values, next_obs, next_done):
        sr = self._step_rollout(obs)
        if sr is not None:
            obs[0].copy_(next_obs)
            dones[0].copy_(next_done)
            sr(obs, actions, logprobs, dones, rewards, values, next_obs, next_done)
            return
        # PPO's per-step loop with the info rows and the tally of every step
        T = obs.shape[0]
        obs[0].copy_(next_obs)
        dones[0].copy_(next_done)
        fused = self._fused_policy(obs)
        for step in range(T):
            if fused is not None:
                action = fused(obs[step], actions[step], logprobs[step], values[step])
            else:
                with self._policy_ctx():
                    action, logprob, _, value = self.agent.get_action_and_value(obs[step])
                actions[step].copy_(action)
                logprobs[step].copy_(logprob)
                values[step].copy_(value.flatten())
            last = step + 1 == T
            _, _, done = self.envs.step_device(action, obs_out=next_obs if last else obs[step + 1],
                                               reward_out=rewards[step],
                                               done_out=next_done if last else dones[step + 1], full_info=True)
            self._after_step(done)

    # ------------------------------------------------------------ resampling
    def _mastered(self):
        """Up to floor(refresh * n_tracks) slots with enough episodes and p at least the
        mastery, highest p first, ties by slot (from the scores just computed)."""
        cur = self.curriculum
        if int(math.floor(self.refresh * cur.n_tracks)) <= 0:
            return np.zeros(0, dtype=np.int64)
        return mastered_slots(cur.tally[:, 0].cpu().numpy(), cur.p.cpu().numpy(), self.refresh, self.mastery,
                              self.min_episodes)

    def _draw_tracks(self, generation, retired):
        """The slot of every env for ``generation`` (device int32 [N]); ``retired``: the slots
        whose tracks were just replaced.  The one place a subclass changes the draw."""
        return self.curriculum.draw(generation)

    def _replace_tracks(self, generation, slots, control_points, widths):
        """Put the given host tracks into ``slots`` and build the pool's table (one
        ``DeviceTrackTable.build`` of every slot's control points)."""
        from .track_device import DeviceTrackTable
        for k, cp, w in zip(slots, control_points, widths):
            self._cps[k], self._widths[k] = cp, w
        return DeviceTrackTable.build(self._cps, self._widths, device=self.device)

    def _spawn_tracks(self, generation, retired):
        """New tracks for the ``retired`` slots -> the ``DeviceTrackTable`` of the whole
        pool.  The one place a subclass changes where new tracks come from; here the
        host draw: ``gen_tracks(seed=None)`` and one ``randint(6, 10)`` width each
        from ``RandomState(seed + 7919 * generation)``."""
        new_cps, new_widths = host_fresh_tracks(self.config["seed"], generation, len(retired))
        return self._replace_tracks(generation, retired, new_cps, new_widths)

    def resample_tracks(self, control_points=None, widths=None):
        """Redraw the envs over the track slots from the tallies.  With no arguments:
        the scores; up to floor(curriculum_refresh * n_tracks) mastered slots are
        retired for fresh tracks (``gen_tracks(seed=None)`` and one ``randint(6, 10)``
        width each from ``RandomState(seed + 7919 * g)``, as ``PPO.resample_tracks``
        draws them: np.random does not move; ``_spawn_tracks``), their tallies start
        again and the table is rebuilt on the device; then every env draws its slot
        (generation g) and is reset.  With nothing retired the table stays and only
        the assignment moves (``reassign_tracks``).  ``control_points`` and ``widths``
        (one per slot) replace the whole pool instead.  The captured rollout graphs
        are dropped.  Returns the new (next_obs, next_done)."""
        cur, envs = self.curriculum, self.envs
        g = envs.track_generation + 1
        cur.scores()
        table = None
        if control_points is not None or widths is not None:
            if control_points is None or widths is None or len(control_points) != cur.n_tracks \
                    or len(widths) != cur.n_tracks:
                raise ValueError(f"resample_tracks: pass control_points and widths for all {cur.n_tracks} slots")
            retired = np.arange(cur.n_tracks, dtype=np.int64)
            table = self._replace_tracks(g, retired, list(control_points), list(widths))
        else:
            retired = self._mastered()
            if len(retired):
                table = self._spawn_tracks(g, retired)
        if len(retired):
            cur.reset_slots(retired)
            cur.scores()  # a fresh slot weighs what an unseen one does
            toe = self._draw_tracks(g, retired).cpu().numpy()
            next_obs = envs.set_tracks(table, toe)
        else:
            toe = self._draw_tracks(g, retired).cpu().numpy()
            next_obs = envs.reassign_tracks(toe)
        self.retired.append([int(k) for k in retired])
        self._graphs = {}
        return next_obs, torch.zeros(self.num_local_envs, device=self.device)

    def track_table(self):
        """``TrackCurriculum.table()``: which tracks this policy still fails."""
        return self.curriculum.table()


def format_track_table(table, limit=None):
    """The per-slot table as text, the most failed slots first."""
    order = np.lexsort((np.arange(len(table["p"])), table["p"]))
    if limit is not None:
        order = order[:limit]
    duel = "wins" in table  # a two-car table (rx.track_selfplay): the win columns follow
    head = f"{'slot':>6} {'episodes':>9} {'finishes':>9} {'crashes':>9} {'progress':>9} {'p':>7} {'prob':>9}"
    if duel:
        head += f" {'wins':>9} {'win rate':>9} {'opp fin':>9} {'opp prog':>9} {'timeouts':>9}"
    lines = [head]
    num = lambda x: "-" if np.isnan(x) else f"{x:.3f}"  # noqa: E731
    for k in order:
        line = (f"{k:>6} {table['episodes'][k]:>9} {table['finishes'][k]:>9} {table['crashes'][k]:>9} "
                f"{num(table['mean_progress'][k]):>9} {table['p'][k]:>7.3f} {table['prob'][k]:>9.2e}")
        if duel:
            line += (f" {table['wins'][k]:>9} {num(table['win_rate'][k]):>9} {table['opp_finishes'][k]:>9} "
                     f"{num(table['opp_mean_progress'][k]):>9} {table['timeouts'][k]:>9}")
        lines.append(line)
    return "\n".join(lines)


__all__ = ["TrackCurriculum", "CurriculumStepRollout", "CurriculumPPO", "format_track_table", "check_rules",
           "host_fresh_tracks", "mastered_slots"]
