"""Episodic track draws: an env takes a new track when its own episode ends.

``CurriculumPPO`` moves envs between tracks only by resetting all of them at a
pool-level redraw, which drops the episodes in flight and runs rx_assign in host
code.  Here the draw follows the episode, as prioritised level replay does: the
kernel that tallies an ended episode (rx_track_episode, include/rx.h) also draws
the env's next slot, and the next step's autoreset starts it there.  Nothing is
dropped, nothing is reset by the curriculum, and the step, ray and policy kernels
are the ones every other rollout runs.

It needs a handle on the lane-varying schedule (``sched=dict(lane_tracks=1)``:
the wave order does not depend on the assignment) with next-step autoreset.

``EpisodicStepRollout``     ppo_fused.StepRollout on rx_track_episodic_rollout_steps;
``EpisodicCurriculumPPO``   the trainer: CurriculumPPO without the global redraw.

The rules are csrc/rx_curriculum.h; DESIGN.md §4 "Episodic track draws".
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .curriculum import CurriculumPPO, CurriculumStepRollout
from .ppo import build_vector_env
from . import dist as rdist


class EpisodicStepRollout(CurriculumStepRollout):
    """rx_track_episodic_rollout_steps driver: CurriculumStepRollout with the
    episodic draw in the tally's place.  ``record_slots=True`` keeps ``slots``,
    int32 [T, N]: the slot every env ran at every step of the last rollout.  The
    draw counters (``curriculum.draws``) and ``slots`` sit at fixed addresses and
    the counters live on the device, so a captured graph of the call keeps drawing
    fresh slots on replay."""

    FN = "rx_track_episodic_rollout_steps"

    def __init__(self, agent, flat, venv, T, curriculum, prec=_lib.RX_PREC_FP32, record_slots=False):
        super().__init__(agent, flat, venv, T, curriculum, prec)
        self.ep = curriculum.episodic()
        self.slots = torch.zeros((T, venv.num_envs), dtype=torch.int32, device=venv.device) if record_slots else None

    def _enqueue(self, args, stream):
        _lib.check(self.L.rx_track_episodic_rollout_steps(self.venv._h, self.venv._io_info(), *args,
                                                          ctypes.byref(self.curriculum.tc), ctypes.byref(self.ep),
                                                          _lib.ptr(self.slots), self.prec, stream), self.FN)
        self.venv._track_ids_stale = True  # the device moved envs between slots: track_ids() downloads them


class EpisodicCurriculumPPO(CurriculumPPO):
    """CurriculumPPO whose envs change track one at a time, when their episode ends.

    The envs are built on the lane-varying schedule (``lane_tracks`` = 1); the
    sampling table is refreshed (rx_track_scores) before the rollout of every
    ``config["episodic_scores_every"]`` (1) updates; ``reassign_tracks`` is never
    called.  ``resample_tracks`` with nothing to retire only refreshes the scores
    and hands back the rollout's own next_obs / next_done; with slots retired it is
    by default the parent's ``set_tracks`` path, which resets every env.
    ``config["episodic_partial"]`` = True (default False) keeps the run free of
    global resets: the retired slots' tracks are replaced in place
    (``RacingVectorEnv.replace_tracks``), only the envs on those slots are reset,
    every other episode goes on, rx_assign does not run and the captured rollout
    graphs stay (no address moved).  A slot keeps its point count there
    (``spawn_same_points``), so the pool's point-count histogram stays the initial
    pool's.
    ``config["episodic_slots"]`` = True records the [T, N] slots of each rollout
    (``slots()``).
    ``config["episodic_regroup_every"]`` = K (default 0 = never): before the rollout of
    every update u > 0 with u % K == 0 the envs' positions are put back in slot order
    (``RacingVectorEnv.regroup_slots``, outside the captured rollout graph, which stays);
    scheduling only, every result is the same bit for bit.

    Refused (ValueError): what CurriculumPPO refuses, and envs whose schedule does
    not come out lane-varying or whose autoreset is not next-step."""

    def __init__(self, env_fn, config, device="cuda"):
        self.scores_every = int(config.get("episodic_scores_every", 1))
        if self.scores_every < 1:
            raise ValueError(f"episodic_scores_every={self.scores_every} must be >= 1")
        self.partial = bool(config.get("episodic_partial", False))
        self.regroup_every = int(config.get("episodic_regroup_every", 0))
        if self.regroup_every < 0:
            raise ValueError(f"episodic_regroup_every={self.regroup_every} must be >= 0 (0 = never)")
        self._updates = 0
        self._carry = None  # the last rollout's (next_obs, next_done)
        super().__init__(env_fn, config, device)

    def _make_envs(self, env_fn):
        c = self.config
        lo, n = rdist.shard(c["num_envs"])
        fn = env_fn if lo == 0 else (lambda i: env_fn(lo + i))
        envs = build_vector_env(fn, n, c["seed"] + rdist.rank(), self.device,
                                track_backend=c.get("track_backend", "scipy"), sched=dict(lane_tracks=1))
        check_episodic(envs)
        return envs

    # ------------------------------------------------------------ rollout
    def _make_step_rollout(self, T, prec):
        return EpisodicStepRollout(self.agent, self._flat, self.envs, T, self.curriculum, prec,
                                   bool(self.config.get("episodic_slots", False)))

    def _after_step(self, done):
        self.curriculum.episode_step(done)  # the per-step loop: the tally and the draw of every step

    def collect_rollout(self, obs, actions, logprobs, dones, rewards, values, next_obs, next_done):
        if self._updates % self.scores_every == 0:
            self.curriculum.scores()  # outside any captured graph: the draws read the table it leaves
        if self.regroup_every and self._updates and self._updates % self.regroup_every == 0:
            self.envs.regroup_slots()  # the draws of the rollouts so far scattered the slots over the waves
        self._updates += 1
        out = super().collect_rollout(obs, actions, logprobs, dones, rewards, values, next_obs, next_done)
        self._carry = (out[6], out[7])
        return out

    def slots(self):
        """int32 [T, N]: the slot of every env at every step of the last rollout
        (``config["episodic_slots"]``), or None."""
        sr = self.__dict__.get("_tc_steps_rollout")
        return None if sr is None else sr.slots

    # ------------------------------------------------------------ resampling
    def _after_retire(self, retired):
        """The partial path's hook between the tallies' reset and the new scores: what else a
        subclass keeps per slot starts again here."""

    def _before_retire(self, generation, retired):
        """The partial path's hook before the retired slots' tallies are reset: what a
        subclass reads of the slots as they stand (their ranks, say) is read here."""

    def _replace_retired(self, generation, retired):
        """The partial path's replacement itself -> ``replace_tracks``' (obs, mask).  Here:
        fresh host tracks of the slots' own point counts (``spawn_same_points``),
        ``RacingVectorEnv.replace_tracks``, and the host copy of the pool."""
        cps, widths = spawn_same_points(self.config["seed"], generation, [len(self._cps[k]) for k in retired])
        obs, mask = self.envs.replace_tracks(retired, cps, widths)
        for k, cp, w in zip(retired, cps, widths):
            self._cps[k], self._widths[k] = cp, w
        return obs, mask

    def _resample_partial(self, retired):
        """``retired`` (ascending) replaced in place: fresh tracks of the slots' own point
        counts (``spawn_same_points``, generation g), their tallies start again, the envs
        on them are reset; everything else goes on.  No ``set_tracks``, no
        ``reassign_tracks``, no draw: an env leaves a replaced slot when its episode ends."""
        cur, envs = self.curriculum, self.envs
        g = envs.track_generation + 1
        self._before_retire(g, retired)
        cur.reset_slots(retired)
        self._after_retire(retired)
        cur.scores()  # a fresh slot weighs what an unseen one does
        obs, mask = self._replace_retired(g, retired)
        if self._carry is None:
            next_obs, next_done = obs.clone(), torch.zeros(self.num_local_envs, device=self.device)
        else:  # the carried rows, the reset envs' replaced: their reset observations, not done
            next_obs, next_done = self._carry
            hit = mask.bool()
            next_obs[hit] = obs[hit]
            next_done[hit] = 0
        self.retired.append([int(k) for k in retired])
        return next_obs, next_done

    def resample_tracks(self, control_points=None, widths=None):
        """With no arguments and no slot to retire: the scores only; the envs keep
        running and the rollout's own (next_obs, next_done) come back.  With slots to
        retire and ``episodic_partial``: ``_resample_partial``.  Otherwise
        ``CurriculumPPO.resample_tracks``' ``set_tracks`` path: new tracks in the retired
        slots, every env redrawn and reset."""
        if control_points is None and widths is None:
            self.curriculum.scores()
            retired = self._mastered()
            if not len(retired):
                self.retired.append([])
                if self._carry is not None:
                    return self._carry
                return self.envs.buf["obs"].clone(), torch.zeros(self.num_local_envs, device=self.device)
            if self.partial:
                return self._resample_partial(np.sort(retired))
        return super().resample_tracks(control_points, widths)


def spawn_same_points(seed, generation, point_counts):
    """Fresh tracks for retired slots that keep their point counts -> (control points,
    widths), one per entry of ``point_counts``.  The RandomState of
    ``CurriculumPPO._spawn_tracks`` (``seed + 7919 * generation``); per slot the
    parameters of ``gen_tracks`` (``_draw_params``, its drawn point count discarded for
    the slot's own), the track, then one ``randint(6, 10)`` width.  Host only;
    ``np.random`` does not move."""
    from .track import _draw_params, gen_random_track
    rng = np.random.RandomState((int(seed) + 7919 * int(generation)) % 2 ** 32)
    cps, widths = [], []
    for P in point_counts:
        _, base, var, jit, smooth = _draw_params(rng)
        cps.append(gen_random_track(int(P), base, var, jit, smooth, None, rng))
        widths.append(int(rng.randint(6, 10)))
    return cps, widths


def check_episodic(envs):
    """ValueError unless ``envs`` can take episodic draws: single-agent, lane-varying
    schedule, next-step autoreset (what rx_track_episode_step refuses, before any launch)."""
    if envs.n_agents != 1:
        raise ValueError("episodic track draws move single-agent envs only (DESIGN.md §8)")
    if envs.autoreset != "next_step":
        raise ValueError(f"episodic track draws need autoreset='next_step', got {envs.autoreset!r}: same-step "
                         "autoreset resets inside the step on the old slot (DESIGN.md §8)")
    if not envs.schedule()["lane_tracks"]:
        raise ValueError("episodic track draws need the lane-varying schedule: build the envs with "
                         "sched=dict(lane_tracks=1) (with at most 2,048 envs, dyn_lpe=1 as well)")


__all__ = ["EpisodicStepRollout", "EpisodicCurriculumPPO", "check_episodic", "spawn_same_points"]
