"""Track evolution under the episodic trainers: retired slots evolved in place.

``EvolvingCurriculumPPO`` fills retired slots on the device with fresh tracks and
edited children of high-ranked tracks (ACCEL), but on the oldest path: a new pool
buffer, ``set_tracks`` and a reset of every env per resample.
``EpisodicReplayCurriculumPPO`` with ``episodic_partial`` replaces retired slots in
place and keeps every other episode running, but fills them from a host loop
(``spawn_same_points``) and cannot edit.  Here the two meet.  A slot that is
replaced in place keeps its point count, so an edited child needs a parent of that
point count: the rank table is regrouped by point count on the device
(rx_track_evolve_classes) and the parent is drawn inside the slot's own class.  The
host knows every retired slot's point count beforehand, so nothing comes down
between the plan and the spawn: the class table, the spawn into a staging buffer
(rx_track_evolve_inplace), the source table, the patch of the live env and the
commit to the pool (rx_track_evolve_commit) are queued one after the other, and
no control point crosses PCIe in either direction.  The plan (16 bytes per
retired slot) comes down last, for the lineage.

``EpisodicEvolvingCurriculumPPO``   the trainer.

The rules are csrc/rx_track_evolve.h; DESIGN.md §4 "Track evolution in place".
"""
import numpy as np

from .track_evolve import TrackEvolver, check_edit_frac
from .track_replay_episodic import EpisodicReplayCurriculumPPO


class EpisodicEvolvingCurriculumPPO(EpisodicReplayCurriculumPPO):
    """``EpisodicReplayCurriculumPPO`` on the partial path whose retired slots are filled
    on the device by a ``TrackEvolver``: with probability ``evolve_edit`` by an edited
    child of a track of the slot's own point count, drawn from the rank table of the
    replay scores, else by a fresh track of that point count.

    A retiring resample: the rank tables as they stand, ``evolver.classes``,
    ``evolver.spawn_in_place``; the retired slots' tallies and replay scores start
    again and the tables and scores are rebuilt; ``replace_tracks_device`` (the handle
    refuses a bad track before anything is written), and only then ``evolver.commit``;
    last the plan's download.  ``set_tracks``, ``reassign_tracks``, ``_draw_tracks``,
    rx_assign and ``spawn_same_points`` never run, only the envs on retired slots are
    reset, and the captured rollout graphs stay.  The pool's point-count histogram
    stays the initial pool's.

    Config key (default): ``evolve_edit`` 0.5, in [0, 1]; ``episodic_partial`` may be
    left out or True.  Until the first retiring resample a run equals
    ``EpisodicReplayCurriculumPPO(episodic_partial=True)``'s bit for bit.
    ``resample_tracks(control_points, widths)`` with a whole pool is the parents'
    global path (``set_tracks``); the pool is uploaded into the evolver's buffer.

    Refused (ValueError) as in the parents, plus an explicit ``episodic_partial`` =
    False and a bad ``evolve_edit``, all before any device call."""

    def __init__(self, env_fn, config, device="cuda"):
        edit_frac = check_edit_frac(config.get("evolve_edit", 0.5))
        if not config.get("episodic_partial", True):
            raise ValueError("episodic_partial=False: EpisodicEvolvingCurriculumPPO evolves retired slots in place, "
                             "it has no global path (rx.track_evolve.EvolvingCurriculumPPO is the one with set_tracks)")
        super().__init__(env_fn, config, device)
        self.partial = True
        self.evolver = TrackEvolver(self.envs, config["seed"], edit_frac)
        self._cps = self._widths = None  # the pool lives in the evolver's device buffer
        n = self.evolver.n_tracks
        self.lineage = {"parent": np.full(n, -1, dtype=np.int32), "kind": np.full(n, -1, dtype=np.int32),
                        "edits": np.zeros(n, dtype=np.int32), "born": np.zeros(n, dtype=np.int32)}
        self.plans = []  # (generation, slots ascending, plan) of every spawn, oldest first
        self._pending = None

    def _record(self, generation, slots, plan):
        lin = self.lineage
        lin["kind"][slots], lin["parent"][slots], lin["edits"][slots] = plan[:, 0], plan[:, 1], plan[:, 3]
        lin["born"][slots] = generation
        self.plans.append((int(generation), np.array(slots, dtype=np.int64), plan.copy()))

    # ------------------------------------------------------------ the partial path's hooks
    def _before_retire(self, generation, retired):
        self.replay.tables(self.replay_updates)  # the ranks before the retired slots' scores start again
        self.evolver.classes(self.replay.cdf_score)
        self._pending = self.evolver.spawn_in_place(retired, generation)

    def _replace_retired(self, generation, retired):
        p, self._pending = self._pending, None
        obs, mask = self.envs.replace_tracks_device(p.slots, p.out_off, p.cp_out, p.width_out)
        ev = self.evolver
        ev.commit(p)  # only now: a refused track has left the pool as it was
        self.envs._table.point_at(ev.cp_off_host, ev.cp, ev.width)
        self._record(generation, p.slots, p.plan.cpu().numpy())
        return obs, mask

    # ------------------------------------------------------------ a whole pool given by the caller
    def _replace_tracks(self, generation, slots, control_points, widths):
        self.evolver.load(control_points, widths)  # resample_tracks passes every slot
        n = self.evolver.n_tracks
        self._record(generation, np.arange(n), np.tile(np.array([-1, -1, 0, 0], dtype=np.int32), (n, 1)))
        return self.evolver.table()

    def control_points(self):
        """-> (list of [P, 2] arrays, widths [n_tracks]): the current pool, downloaded."""
        return self.evolver.control_points()

    def track_table(self):
        """``EpisodicReplayCurriculumPPO.track_table()`` plus each slot's lineage: ``kind`` (-1
        the initial pool or a given track, 0 fresh, 1 edit), ``parent`` (the slot of the pool
        before, -1 for none), ``edits`` (applied) and ``born`` (the generation)."""
        tab = super().track_table()
        tab.update({k: v.copy() for k, v in self.lineage.items()})
        return tab


__all__ = ["EpisodicEvolvingCurriculumPPO"]
