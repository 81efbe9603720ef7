"""Track curriculum for self-play: per-track tallies of two-car episodes.

``rx.curriculum`` answers "which tracks does the learner still fail" for
single-agent envs; a self-play or league run trained for its whole life on the
pool it was built with, env i on slot i % n, and ``head_to_head()`` answered
"whom does the learner lose to" but nothing answered "on which tracks".  Here
every finished two-car episode is counted against its track slot where it
happens (one small kernel per rollout step) -- the learner's finishes, the
both-cars-crashed terminations and progress in rx.curriculum's columns, its wins,
the opponent's finishes and progress and the timeouts beside them -- and at every
``config["track_resample_every"]`` boundary the envs are redrawn over the slots,
weighted towards the tracks the learner still loses on; the mastered slots are
retired for fresh tracks.  ``SelfPlayPPO.update_opponent`` rebuilds (= resets)
every env before every update anyway, so the redraw drops no episode that was
not dropped already.  The rollout stays one library call
(rx_track_duel_rollout_steps, include/rx.h) that a HIP graph can record.

``DuelTrackCurriculum``       the device tensors (tally, duel, cdf, p, track_of_env)
                              and the kernels (rx_track_tally2 / rx_track_duel_scores /
                              rx_track_draw);
``DuelSelfPlayStepRollout``   ppo_fused.SelfPlayStepRollout on rx_track_duel_rollout_steps;
``DuelLeagueStepRollout``     league_train.LeagueStepRollout on the same call with the bank;
``SelfPlayCurriculumPPO``     SelfPlayPPO with the tally and the resample;
``LeagueCurriculumPPO``       LeagueSelfPlayPPO with the same.

The rules (tally, scores) are csrc/rx_track_duel.h; DESIGN.md §4.  Losses are
``episodes - wins``: placement 1 is always awarded when an episode ends.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import dist as rdist
from .curriculum import PROGRESS_Q, format_track_table, host_fresh_tracks, mastered_slots
from .league_train import LeagueSelfPlayPPO, LeagueStepRollout
from .ppo_fused import SelfPlayStepRollout
from .selfplay import SelfPlayPPO


def check_duel_rules(power, mix, prior, score):
    """The ranges rx_track_duel_scores / rx_track_draw accept, as ValueErrors naming the config key."""
    if not 0 <= int(power) <= _lib.RX_TRACK_MAX_POWER:
        raise ValueError(f"curriculum_power={power} outside 0..{_lib.RX_TRACK_MAX_POWER}")
    if not 0.0 <= float(mix) <= 1.0:
        raise ValueError(f"curriculum_mix={mix} outside [0, 1]")
    if not float(prior) > 0.0:
        raise ValueError(f"curriculum_prior={prior} must be > 0")
    if score not in _lib.TRACK_DUEL_SCORES:
        raise ValueError(f"curriculum score must be one of {sorted(_lib.TRACK_DUEL_SCORES)}, got {score!r}")
    return int(power), float(mix), float(prior), _lib.TRACK_DUEL_SCORES[score]


class DuelTrackCurriculum:
    """The tallies of a two-car ``venv``'s track slots, car ``agent_idx`` the learner's,
    and the draw of its envs over them.

    ``tally`` int64 [n_tracks, 4] = (episodes, finishes, crashes, progress_q) of the
    learner's car, ``duel`` int64 [n_tracks, 4] = (wins, opp_finishes, opp_progress_q,
    timeouts), ``cdf`` int64 [n_tracks], ``p`` float64 [n_tracks], ``track_of_env``
    int32 [N]: device tensors at fixed addresses, so the two structs serve every call
    and any captured graph.  The slot of env e is read from the env's bound ``track``
    array, which rx_assign rewrites in place."""

    def __init__(self, venv, agent_idx=0, seed=0, power=1, mix=0.1, prior=1.0, score="lose"):
        if getattr(venv, "n_agents", None) != 2:
            raise ValueError("DuelTrackCurriculum tallies two-car envs (rx.curriculum.TrackCurriculum: single-agent)")
        if agent_idx not in (0, 1):
            raise ValueError(f"agent_idx={agent_idx} must be 0 or 1")
        self.power, self.mix, self.prior, self.score = check_duel_rules(power, mix, prior, score)
        self.L = _lib.load()
        self.venv, self.agent_idx, self.seed = venv, int(agent_idx), int(seed) & (2**64 - 1)
        self.n_tracks = len(venv._table) if venv._table is not None else len(venv.tracks)
        n, dev = venv.num_envs, venv.device
        self.tally = torch.zeros((self.n_tracks, _lib.RX_TRACK_TALLY_W), dtype=torch.int64, device=dev)
        self.duel = torch.zeros((self.n_tracks, _lib.RX_TRACK_DUEL_W), dtype=torch.int64, device=dev)
        self.cdf = torch.zeros(self.n_tracks, dtype=torch.int64, device=dev)
        self.p = torch.full((self.n_tracks,), 0.5, dtype=torch.float64, device=dev)
        self.track_of_env = torch.zeros(n, dtype=torch.int32, device=dev)
        self.tc = _lib.RxTrackIO(self.n_tracks, self.score, _lib.ptr(venv._st["track"]), _lib.ptr(self.tally),
                                 _lib.ptr(self.cdf), _lib.ptr(self.p), _lib.ptr(self.track_of_env), self.seed)
        self.td = _lib.RxTrackDuelIO(self.agent_idx, _lib.ptr(self.duel))

    def tally_step(self, done=None, stream=None):
        """Count the envs whose episode ended in the step just enqueued (rx_track_tally2 on
        the env's own terminated / info rows; ``done``: the step's done row when it went
        into a rollout buffer).  The step must have run with ``full_info=True``."""
        b = self.venv.buf
        _lib.check(self.L.rx_track_tally2(ctypes.byref(self.tc), ctypes.byref(self.td), self.venv.num_envs,
                                          _lib.ptr(b["done_f32"] if done is None else done),
                                          _lib.ptr(b["terminated"]), _lib.ptr(b["info"]), _lib.stream_ptr(stream)),
                   "rx_track_tally2")

    def scores(self, stream=None):
        """tallies -> ``p`` and the integer sampling table ``cdf`` (rx_track_duel_scores)."""
        _lib.check(self.L.rx_track_duel_scores(ctypes.byref(self.tc), ctypes.byref(self.td), self.power, self.prior,
                                               _lib.stream_ptr(stream)), "rx_track_duel_scores")

    def draw(self, generation, stream=None):
        """A slot for every env from the current table (rx_track_draw) -> ``track_of_env``."""
        _lib.check(self.L.rx_track_draw(ctypes.byref(self.tc), self.venv.num_envs, int(generation) & 0xFFFFFFFF,
                                        self.mix, _lib.stream_ptr(stream)), "rx_track_draw")
        return self.track_of_env

    def reset_slots(self, idx):
        """Zero both rows of the slots ``idx`` (their tracks were replaced)."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size:
            if idx.min() < 0 or idx.max() >= self.n_tracks:
                raise ValueError(f"slots must lie in [0, {self.n_tracks})")
            rows = torch.from_numpy(idx).to(self.tally.device)
            self.tally[rows] = 0
            self.duel[rows] = 0

    def table(self):
        """The host view per slot, arrays of length n_tracks: ``TrackCurriculum.table()``'s
        columns (episodes, finishes, crashes, mean_progress, p, prob; for the learner's
        car, p of the chosen score) plus wins, win_rate (NaN before the first episode),
        opp_finishes, opp_mean_progress and timeouts.  Losses are episodes - wins.  Runs
        ``scores`` and downloads; call it between updates."""
        self.scores()
        t, d = self.tally.cpu().numpy(), self.duel.cpu().numpy()
        cdf = self.cdf.cpu().numpy().astype(np.uint64)
        w = np.diff(np.concatenate([[np.uint64(0)], cdf])).astype(np.float64)
        n, F = self.n_tracks, float(cdf[-1])
        prob = np.full(n, 1.0 / n) if F == 0 else (1.0 - self.mix) * (w / F) + self.mix / n
        ep = t[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_progress = np.where(ep > 0, t[:, 3] / PROGRESS_Q / ep, np.nan)
            opp_mean_progress = np.where(ep > 0, d[:, 2] / PROGRESS_Q / ep, np.nan)
            win_rate = np.where(ep > 0, d[:, 0] / ep, np.nan)
        return {"episodes": t[:, 0].copy(), "finishes": t[:, 1].copy(), "crashes": t[:, 2].copy(),
                "mean_progress": mean_progress, "p": self.p.cpu().numpy(), "prob": prob, "wins": d[:, 0].copy(),
                "win_rate": win_rate, "opp_finishes": d[:, 1].copy(), "opp_mean_progress": opp_mean_progress,
                "timeouts": d[:, 3].copy()}


class _DuelEnqueue:
    """What the two drivers share: the curriculum, and the call with or without the league io."""

    FN = "rx_track_duel_rollout_steps"

    def __init__(self, agent, flat, spenv, T, curriculum, prec=_lib.RX_PREC_FP32):
        super().__init__(agent, flat, spenv, T, prec)
        self.curriculum = curriculum

    def _league(self):
        return None

    def _enqueue(self, args, stream):
        cur = self.curriculum
        _lib.check(self.L.rx_track_duel_rollout_steps(self.venv._h, self.venv._io_info(), *args, self._league(),
                                                      ctypes.byref(cur.tc), ctypes.byref(cur.td), self.prec, stream),
                   self.FN)


class DuelSelfPlayStepRollout(_DuelEnqueue, SelfPlayStepRollout):
    """rx_track_duel_rollout_steps driver with one frozen opponent: SelfPlayStepRollout's
    launches with one rx_track_tally2 after every step.  The step runs with the env's
    terminated and info rows, which the tally reads; every rollout output equals
    SelfPlayStepRollout's bit for bit (tests/test_track_selfplay_gpu.py)."""


class DuelLeagueStepRollout(_DuelEnqueue, LeagueStepRollout):
    """The same call with the league io: LeagueStepRollout's launches, its ids, draw
    counts and head-to-head tally, and the track tally after every step."""

    def _league(self):
        return ctypes.byref(self.spenv.lg)


class _DuelCurriculumTrainer:
    """SelfPlayCurriculumPPO's and LeagueCurriculumPPO's shared half (a mixin in front of
    the parent trainer): the tally in both rollout paths, the resample in the place of
    the env rebuild, the per-slot table and the checkpoint entry."""

    resamples_tracks = True
    _parent_driver = None  # whose ``supported`` decides between the library call and the per-step path
    _driver = None

    def __init__(self, env_fn, config, device="cuda"):
        if rdist.world() > 1:
            raise ValueError(f"{type(self).__name__} needs world size 1: the per-track tallies are per rank and the "
                             "sampling table would need their all-reduce (DESIGN.md §8)")
        c = config
        self._rules = check_duel_rules(c.get("curriculum_power", 1), c.get("curriculum_mix", 0.1),
                                       c.get("curriculum_prior", 1.0), c.get("curriculum_score", "lose"))
        self.refresh = float(c.get("curriculum_refresh", 0.25))
        self.mastery = float(c.get("curriculum_mastery", 0.8))
        self.min_episodes = int(c.get("curriculum_min_episodes", 4))
        if not 0.0 <= self.refresh <= 1.0:
            raise ValueError(f"curriculum_refresh={self.refresh} outside [0, 1]")
        if env_fn is not None:
            # one spec, built and dropped with np.random put back: a train.py env_fn may draw its track id there
            state = np.random.get_state()
            spec = env_fn(0)
            np.random.set_state(state)
            if getattr(spec, "num_agents", 1) != 2:
                raise ValueError(f"{type(self).__name__} trains two-car envs (rx.curriculum.CurriculumPPO: "
                                 "single-agent)")
        self._update = 0
        super().__init__(env_fn, config, device)
        venv = self.envs.venv
        geoms = venv.tracks.geoms
        self._cps = [np.asarray(g.control_points, dtype=np.float64) for g in geoms]
        self._widths = [float(g.track_width) for g in geoms]
        power, mix, prior, _ = self._rules
        self.curriculum = DuelTrackCurriculum(venv, self.envs.agent_idx, c["seed"], power, mix, prior,
                                              c.get("curriculum_score", "lose"))
        self.retired = []  # the slots each resample replaced, oldest first

    # ------------------------------------------------------------ rollout
    def _step_rollout(self, obs):
        from . import ppo_fused
        c = self.config
        if self._fused_policy(obs) is None or not self._parent_driver.supported(self.envs, self.agent, c):
            return None
        T, prec = obs.shape[0], ppo_fused.precision(c)
        sr = self.__dict__.get("_td_steps_rollout")
        if sr is None or sr.T != T or sr.n != self.envs.num_envs or sr.prec != prec:
            sr = self._td_steps_rollout = self._driver(self.agent, self._flat, self.envs, T, self.curriculum, prec)
        return sr

    def _rollout_body(self, obs, actions, logprobs, dones, rewards, values, next_obs, next_done):
        T = obs.shape[0]
        obs[0].copy_(next_obs)
        dones[0].copy_(next_done)
        sr = self._step_rollout(obs)
        if sr is not None:
            sr(obs, actions, logprobs, dones, rewards, values, next_obs, next_done)
            return
        # the parent's per-step loop (the random opponent of an empty pool, rollout_steps "off") with
        # the info rows and the tally of every step
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
            self.curriculum.tally_step(done)

    # ------------------------------------------------------------ resampling
    def advance_pool(self, update):
        self._update = int(update)  # update_opponent follows: its rebuild needs to know the boundary
        super().advance_pool(update)

    def _rebuild_envs(self):
        K = int(self.config.get("track_resample_every", 0))
        if K > 0 and self._update > 0 and self._update % K == 0:
            self.resample_tracks()
        else:
            super()._rebuild_envs()

    def _mastered(self):
        cur = self.curriculum
        if int(math.floor(self.refresh * cur.n_tracks)) <= 0:
            return np.zeros(0, dtype=np.int64)
        return mastered_slots(cur.tally[:, 0].cpu().numpy(), cur.p.cpu().numpy(), self.refresh, self.mastery,
                              self.min_episodes)

    def _pool_table(self):
        from .track_device import DeviceTrackTable
        return DeviceTrackTable.build(self._cps, self._widths, device=self.device)

    def resample_tracks(self):
        """Redraw the envs over the track slots from the tallies, in the place of the
        parent's env rebuild: the scores; up to floor(curriculum_refresh * n_tracks)
        mastered slots (p of the chosen score) are retired for fresh host tracks
        (``curriculum.host_fresh_tracks``, CurriculumPPO's draw: np.random does not move),
        their ``tally`` and ``duel`` rows start again and the table is rebuilt on the
        device; the scores again; then every env draws its slot (generation g) and is
        reset once, by ``set_tracks`` when slots were retired and ``reassign_tracks``
        otherwise.  The captured rollout graphs of every opponent kind are dropped.  The
        league's ids, draw counts and tallies are env-indexed and stay."""
        cur, venv = self.curriculum, self.envs.venv
        g = venv.track_generation + 1
        cur.scores()
        retired = self._mastered()
        if len(retired):
            cps, widths = host_fresh_tracks(self.config["seed"], g, len(retired))
            for k, cp, w in zip(retired, cps, widths):
                self._cps[k], self._widths[k] = np.asarray(cp, dtype=np.float64), float(w)
            table = self._pool_table()
            cur.reset_slots(retired)
            cur.scores()  # a fresh slot weighs what an unseen one does
            venv.set_tracks(table, cur.draw(g).cpu().numpy())
        else:
            venv.reassign_tracks(cur.draw(g).cpu().numpy())
        self.retired.append([int(k) for k in retired])
        self._graphs_by_kind = {}
        self._graphs = {}
        return self.envs.buf["obs"], torch.zeros(self.num_local_envs, device=self.device)

    def track_table(self):
        """``DuelTrackCurriculum.table()``: on which tracks this policy still loses."""
        return self.curriculum.table()

    # ------------------------------------------------------------ checkpoints
    def _checkpoint_extra(self):
        cur, venv = self.curriculum, self.envs.venv
        return {**super()._checkpoint_extra(),
                "track_state": {"tally": cur.tally.cpu(), "duel": cur.duel.cpu(),
                                "control_points": [torch.from_numpy(np.ascontiguousarray(cp)) for cp in self._cps],
                                "widths": torch.tensor(self._widths, dtype=torch.float64),
                                "track_of_env": torch.from_numpy(np.array(venv.track_of_env, dtype=np.int32)),
                                "generation": int(venv.track_generation)}}

    def _checkpoint_loaded(self, ck):
        """Restore the tallies, the pool and the assignment; a checkpoint without
        "track_state" loads as a fresh curriculum on the built pool."""
        super()._checkpoint_loaded(ck)
        cur, venv = self.curriculum, self.envs.venv
        cur.tally.zero_()
        cur.duel.zero_()
        ts = ck.get("track_state")
        if not ts:
            return
        if tuple(ts["tally"].shape) != tuple(cur.tally.shape) or ts["track_of_env"].numel() != venv.num_envs:
            raise ValueError("the checkpoint's track_state does not fit this pool or env count")
        cps = [cp.cpu().numpy().copy() for cp in ts["control_points"]]  # load_checkpoint maps to the device
        widths = [float(w) for w in ts["widths"].cpu()]
        toe = ts["track_of_env"].cpu().numpy().astype(np.int32)
        same_pool = widths == self._widths and all(a.shape == b.shape and np.array_equal(a, b)
                                                   for a, b in zip(cps, self._cps))
        self._cps, self._widths = cps, widths
        if not same_pool:
            venv.set_tracks(self._pool_table(), toe)
        elif not np.array_equal(toe, venv.track_of_env):
            venv.reassign_tracks(toe)
        venv.track_generation = int(ts["generation"])
        cur.tally.copy_(ts["tally"])
        cur.duel.copy_(ts["duel"])
        self._graphs_by_kind = {}
        self._graphs = {}


class SelfPlayCurriculumPPO(_DuelCurriculumTrainer, SelfPlayPPO):
    """SelfPlayPPO that tallies every finished episode against its track slot and, every
    ``config["track_resample_every"]`` updates, redraws the envs over the slots weighted
    towards the tracks it still loses on, in the place of that update's env rebuild.

    Config keys (defaults): ``track_resample_every`` 0 (tally only: ``track_table()``
    still answers on which tracks it loses), ``curriculum_power`` 1, ``curriculum_mix``
    0.1, ``curriculum_prior`` 1.0, ``curriculum_score`` "lose" (or "fail", "potential",
    "contested"), ``curriculum_refresh`` 0.25 (the largest fraction of the slots retired
    per resample), ``curriculum_mastery`` 0.8 and ``curriculum_min_episodes`` 4 (a slot
    is retired once it has that many episodes and p, of the chosen score, at least the
    mastery).  Until the first resample a run equals SelfPlayPPO's bit for bit;
    ``next_obs`` after a resample follows the parent's rule (stale unless
    ``refresh_obs_on_rebuild``).

    Refused (ValueError): a world size above 1, single-agent envs, an unknown score."""

    _parent_driver, _driver = SelfPlayStepRollout, DuelSelfPlayStepRollout


class LeagueCurriculumPPO(_DuelCurriculumTrainer, LeagueSelfPlayPPO):
    """LeagueSelfPlayPPO with SelfPlayCurriculumPPO's tally and resample (the same config
    keys).  ``head_to_head()`` answers whom the learner loses to, ``track_table()`` on
    which tracks."""

    _parent_driver, _driver = LeagueStepRollout, DuelLeagueStepRollout


__all__ = ["DuelTrackCurriculum", "DuelSelfPlayStepRollout", "DuelLeagueStepRollout", "SelfPlayCurriculumPPO",
           "LeagueCurriculumPPO", "check_duel_rules", "format_track_table"]
