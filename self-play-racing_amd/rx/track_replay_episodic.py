"""Prioritised level replay per episode: the replay scores on episodic draws.

``ReplayCurriculumPPO`` can apply its value-loss scores only at a pool-level redraw
(every env reset, every env drawing at once); ``EpisodicCurriculumPPO`` moves one
env at a time, when its own episode ends, but draws from the finish tallies only.
Here the two meet, as in Jiang et al. 2021: an env whose episode ends draws its
next slot from the uniform / staleness / rank mix of the replay tables
(rx_track_learn_episode, include/rx.h), inside the rollout and without a reset, and
after the GAE launch the advantages are tallied by the slot every step ran on
(rx_track_learn_tally_slots over the rollout's ``slots[T][N]``), leaving out the
autoreset rows, whose advantage spans two tracks.

``ReplayEpisodicStepRollout``     EpisodicStepRollout on
                                  rx_track_learn_episodic_rollout_steps;
``EpisodicReplayCurriculumPPO``   the trainer.

The rules are csrc/rx_track_replay.h; DESIGN.md §4 "Replay scores on episodic draws".
"""
import ctypes

import torch

from . import _lib
from .track_episodic import EpisodicCurriculumPPO, EpisodicStepRollout
from .track_replay import TrackReplay, check_replay_rules


class ReplayEpisodicStepRollout(EpisodicStepRollout):
    """rx_track_learn_episodic_rollout_steps driver: EpisodicStepRollout whose draw reads
    ``replay``'s tables.  ``slots`` is always recorded: the tally needs it."""

    FN = "rx_track_learn_episodic_rollout_steps"

    def __init__(self, agent, flat, venv, T, curriculum, replay, prec=_lib.RX_PREC_FP32):
        super().__init__(agent, flat, venv, T, curriculum, prec, record_slots=True)
        self.replay = replay

    def _enqueue(self, args, stream):
        _lib.check(self.L.rx_track_learn_episodic_rollout_steps(
            self.venv._h, self.venv._io_info(), *args, ctypes.byref(self.curriculum.tc), ctypes.byref(self.replay.lt),
            ctypes.byref(self.ep), self.replay.stale_mix, _lib.ptr(self.slots), self.prec, stream), self.FN)
        self.venv._track_ids_stale = True  # the device moved envs between slots: track_ids() downloads them


class EpisodicReplayCurriculumPPO(EpisodicCurriculumPPO):
    """``EpisodicCurriculumPPO`` whose ended envs draw from the replay scores.

    It owns a ``TrackReplay`` (``replay``; the ``replay_*`` config keys of
    ``ReplayCurriculumPPO``, ``curriculum_mix`` the uniform part).  Before the rollout
    of every ``episodic_scores_every`` updates the replay tables are rebuilt
    (``replay.tables``) next to ``curriculum.scores()``, outside any captured graph;
    inside the rollout every ended env draws from them, in the one-call rollout and
    in the per-step loop alike, and the slots of every step are always recorded
    (``slots()``).  After the GAE launch the raw advantages are tallied by those
    slots without the autoreset rows and folded into the scores.  The finish tallies
    are kept and still decide which slots are retired; a resample that retires slots
    is ``ReplayCurriculumPPO``'s: the retired slots start again as never scored and
    every env is redrawn by ``replay.draw`` and reset.  With ``episodic_partial`` the
    retired slots are replaced in place instead (``EpisodicCurriculumPPO``): they start
    again as never scored, only their envs are reset, and the run stays free of global
    resets.

    Refused (ValueError) as in ``EpisodicCurriculumPPO`` and ``ReplayCurriculumPPO``,
    before a device is touched."""

    def __init__(self, env_fn, config, device="cuda"):
        c = config
        self._replay_rules = (c.get("replay_kind", "value_l1"), c.get("replay_power", 4), c.get("replay_alpha", 1.0),
                              c.get("curriculum_mix", 0.1), c.get("replay_stale_mix", 0.1))
        check_replay_rules(*self._replay_rules)
        self._loop_slots = None   # the per-step loop's slots [T, N]
        self._loop_row = 0
        self._slots_last = None   # the slots of the last rollout, whichever form collected it
        super().__init__(env_fn, config, device)
        self.replay = TrackReplay(self.envs, c["seed"], *self._replay_rules)
        self.replay_updates = 0  # the folds so far: the index of the next update

    # ------------------------------------------------------------ rollout
    def _make_step_rollout(self, T, prec):
        return ReplayEpisodicStepRollout(self.agent, self._flat, self.envs, T, self.curriculum, self.replay, prec)

    def _after_step(self, done):
        row = self._loop_slots[self._loop_row]  # the per-step loop: the tally, the draw and this step's slots row
        self._loop_row += 1
        self.replay.episode_step(self.curriculum, done, slot_out=row)

    def _rollout_body(self, obs, *rest):
        sr = self._step_rollout(obs)
        self._loop_row = 0
        self._slots_last = self._loop_slots if sr is None else sr.slots
        super()._rollout_body(obs, *rest)

    def collect_rollout(self, obs, *rest):
        if self._updates % self.scores_every == 0:
            self.replay.tables(self.replay_updates)  # outside any captured graph, as curriculum.scores()
        shape = (obs.shape[0], obs.shape[1])
        if self._step_rollout(obs) is None and (self._loop_slots is None or tuple(self._loop_slots.shape) != shape):
            self._loop_slots = torch.zeros(shape, dtype=torch.int32, device=self.device)  # before any capture
            self._graphs = {}
        return super().collect_rollout(obs, *rest)

    def slots(self):
        """int32 [T, N]: the slot of every env at every step of the last rollout."""
        return self._slots_last

    # ------------------------------------------------------------ scores
    def compute_advantages(self, rewards, dones, values, next_value, next_done):
        advantages, returns = super().compute_advantages(rewards, dones, values, next_value, next_done)
        # the raw GAE output by the slot of every step; dones[t] != 0 marks the autoreset rows
        self.replay.tally_slots(advantages, self.slots(), dones)
        self.replay.fold(self.replay_updates)
        self.replay_updates += 1
        return advantages, returns

    def _after_retire(self, retired):
        self.replay.reset_slots(retired)  # the partial path: the replaced slots read as never scored
        self.replay.tables(self.replay_updates)

    def _draw_tracks(self, generation, retired):
        if len(retired):
            self.replay.reset_slots(retired)
        self.replay.tables(self.replay_updates)
        return self.replay.draw(generation)

    def track_table(self):
        """``CurriculumPPO.track_table()`` plus the replay columns score, seen, rank and
        staleness; ``prob`` is the replay draw's and ``prob_finishes`` the finish table's."""
        tab = super().track_table()
        rep = self.replay.table(self.replay_updates)
        tab["prob_finishes"] = tab["prob"]
        tab.update(rep)
        return tab


__all__ = ["ReplayEpisodicStepRollout", "EpisodicReplayCurriculumPPO"]
