"""Track evolution: the slots the curriculum retires are filled on the device.

``CurriculumPPO`` and ``ReplayCurriculumPPO`` decide on the device which tracks to
train on and which slots to retire, but what goes into a retired slot is a host
Python loop (``gen_tracks``), a host list of control points and a fresh upload of
every slot, and the new tracks know nothing of what the scores have learnt.  Here
the control points live in device memory and a kernel writes the new ones: a fresh
track of the generator's distribution, or -- ACCEL (Parker-Holder et al. 2022) -- a
small edit of a track the replay scores still rank high, so the pool moves to the
learner's frontier instead of being redrawn at random.

``TrackEvolver``           the device control-point buffer (cp, width, cp_off), the
                           two calls (rx_track_evolve_plan / rx_track_evolve) and the
                           in-place form (rx_track_evolve_classes / _inplace / _commit;
                           its trainer is rx.track_evolve_episodic);
``EvolvingCurriculumPPO``  ``ReplayCurriculumPPO`` whose retired slots are filled by
                           the evolver.

A resample downloads the plan (16 bytes per retired slot), forms the new offsets
on the host (rx_build_tracks wants them there anyway), and hands the new buffer to
``DeviceTrackTable.build_from_device``: no control point crosses PCIe in either
direction.  The rules are csrc/rx_track_evolve.h; DESIGN.md §4.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .track import DEFAULT_CONTROL_POINTS, DEFAULT_WIDTH
from .track_device import DeviceTrackTable
from .track_replay import ReplayCurriculumPPO

KINDS = {-1: "initial", _lib.RX_TRACK_EVOLVE_FRESH: "fresh", _lib.RX_TRACK_EVOLVE_EDIT: "edit"}


def check_edit_frac(edit_frac):
    """The range rx_track_evolve_plan accepts, as a ValueError naming the config key."""
    f = float(edit_frac)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"evolve_edit={edit_frac} outside [0, 1]")
    return f


class TrackEvolver:
    """The control points of ``venv``'s track slots in device memory and what fills
    the slots that are replaced.

    ``cp`` float64 [total, 2], ``width`` float64 [n_tracks] and ``cp_off`` int32
    [n_tracks + 1] (in points) are device tensors, initialised from the env's slots;
    ``cp_off_host`` is the host copy of the offsets.  ``spawn`` writes the next pool
    into new tensors and swaps them in (the point counts change, so the buffer is
    not edited in place); ``classes`` / ``spawn_in_place`` / ``commit`` are the form for slots
    that keep their point counts: the same tensors, written in place."""

    def __init__(self, venv, seed, edit_frac=0.5, factor=30):
        if venv.n_agents != 1:
            raise ValueError("track evolution fills the slots of single-agent envs only (DESIGN.md §8)")
        if venv._table is not None:
            cps, widths = venv._table.control_points, venv._table.widths
            if cps is None or widths is None or any(c is None for c in cps):
                raise ValueError("the env's table carries no control points to evolve")
        else:
            geoms = venv.tracks.geoms
            cps, widths = [g.control_points for g in geoms], [g.track_width for g in geoms]
        self._setup(venv.device, seed, edit_frac, factor)
        self.load(cps, widths)

    @classmethod
    def from_tracks(cls, control_points, widths, seed, edit_frac=0.5, factor=30, device="cuda"):
        """An evolver over the given host tracks, without an env (tools, tests)."""
        self = cls.__new__(cls)
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._setup(dev, seed, edit_frac, factor)
        self.load(control_points, widths)
        return self

    def _setup(self, device, seed, edit_frac, factor):
        self.edit_frac = check_edit_frac(edit_frac)
        self.L = _lib.load()
        self.seed, self.factor, self.device = int(seed) & (2**64 - 1), factor, device
        self._classes = None  # (order, cdf_class, class_end) of the last classes() call

    def load(self, control_points, widths):
        """Replace the whole pool by host tracks (one upload)."""
        cps = [np.asarray(DEFAULT_CONTROL_POINTS if c is None else c, dtype=np.float64) for c in control_points]
        ws = [DEFAULT_WIDTH if w is None else w for w in widths]
        if not cps or len(ws) != len(cps) or any(c.ndim != 2 or c.shape[1] != 2 for c in cps):
            raise ValueError("need at least one track of [P, 2] control points and one width per track")
        self.n_tracks = len(cps)
        self.cp_off_host = np.concatenate([[0], np.cumsum([len(c) for c in cps])]).astype(np.int32)
        self.cp = torch.from_numpy(np.ascontiguousarray(np.concatenate(cps))).to(self.device)
        self.width = torch.from_numpy(np.ascontiguousarray(ws, dtype=np.float64)).to(self.device)
        self.cp_off = torch.from_numpy(self.cp_off_host).to(self.device)
        self._classes = None

    def table(self):
        """The ``DeviceTrackTable`` of the pool as it stands (one rx_build_tracks launch)."""
        return DeviceTrackTable.build_from_device(self.cp_off_host, self.cp, self.width, self.factor)

    def control_points(self):
        """-> (list of [P, 2] float64 arrays, widths float64 [n_tracks]): the pool, downloaded."""
        cp, off = self.cp.cpu().numpy(), self.cp_off_host
        return [cp[off[k]:off[k + 1]].copy() for k in range(self.n_tracks)], self.width.cpu().numpy()

    def spawn(self, slots, generation, cdf_score, stream=None):
        """Replace ``slots`` at ``generation``: rx_track_evolve_plan from the rank table
        ``cdf_score`` (device int64 [n_tracks], as rx_track_learn_tables left it), the
        plan's download, the new offsets, rx_track_evolve into a new buffer, which
        becomes the pool.  -> (the new ``DeviceTrackTable``, plan int32 [n_spawn, 4] =
        (kind, parent or -1, P, edits applied), rows in ascending slot order)."""
        n = self.n_tracks
        slots = np.unique(np.asarray(slots, dtype=np.int64).reshape(-1))
        if slots.size and (slots[0] < 0 or slots[-1] >= n):
            raise ValueError(f"slots must lie in [0, {n})")
        if cdf_score.dtype != torch.int64 or tuple(cdf_score.shape) != (n,) or cdf_score.device != self.cp.device \
                or not cdf_score.is_contiguous():
            raise ValueError(f"rx_track_evolve_plan: cdf_score must be a contiguous int64 [{n}] on the env's device")
        g, ns, dev, q = int(generation) & 0xFFFFFFFF, len(slots), self.cp.device, _lib.ptr
        with torch.cuda.device(dev):
            s = _lib.stream_ptr(stream)
            slots_d = torch.from_numpy(slots.astype(np.int32)).to(dev)
            plan_d = torch.zeros((ns, _lib.RX_TRACK_EVOLVE_W), dtype=torch.int32, device=dev)
            ev = _lib.RxTrackEvolveIO(n, ns, q(slots_d), q(self.cp_off), q(self.cp), q(self.width), q(cdf_score),
                                      q(plan_d), None, None, None, self.seed)
            _lib.check(self.L.rx_track_evolve_plan(ctypes.byref(ev), g, self.edit_frac, s), "rx_track_evolve_plan")
            points = np.diff(self.cp_off_host)
            points[slots] = plan_d.cpu().numpy()[:, 2]
            off_new = np.concatenate([[0], np.cumsum(points)]).astype(np.int32)
            off_new_d = torch.from_numpy(off_new).to(dev)
            cp_new = torch.empty((int(off_new[-1]), 2), dtype=torch.float64, device=dev)
            width_new = torch.empty(n, dtype=torch.float64, device=dev)
            ev.cp_off_new, ev.cp_new, ev.width_new = q(off_new_d), q(cp_new), q(width_new)
            _lib.check(self.L.rx_track_evolve(ctypes.byref(ev), g, s), "rx_track_evolve")
            plan = plan_d.cpu().numpy()
        self.cp, self.width, self.cp_off, self.cp_off_host = cp_new, width_new, off_new_d, off_new
        self._classes = None  # the class table was the old pool's
        return self.table(), plan

    # ------------------------------------------------------------ in place: a slot keeps its point count
    def _inplace_io(self, ns=0, slots=None, cdf_score=None, plan=None, out_off=None, cp_out=None, width_out=None):
        q = _lib.ptr
        order, cdf_class, class_end = self._classes or (None, None, None)
        return _lib.RxTrackEvolveInplaceIO(self.n_tracks, ns, q(slots), q(self.cp_off), q(self.cp), q(self.width),
                                           q(cdf_score), q(order), q(cdf_class), q(class_end), q(plan), q(out_off),
                                           q(cp_out), q(width_out), self.seed)

    def classes(self, cdf_score, stream=None):
        """rx_track_evolve_classes: the rank table ``cdf_score`` (device int64 [n_tracks], as
        rx_track_learn_tables left it) regrouped by point count, for the parent draws of
        ``spawn_in_place``.  One launch, no download and no wait.  -> the device tensors
        (order int32 [n_tracks], cdf_class int64 [n_tracks], class_end int32 [65]), which the
        evolver keeps and the next call overwrites."""
        n, dev = self.n_tracks, self.cp.device
        if cdf_score.dtype != torch.int64 or tuple(cdf_score.shape) != (n,) or cdf_score.device != dev \
                or not cdf_score.is_contiguous():
            raise ValueError(f"rx_track_evolve_classes: cdf_score must be a contiguous int64 [{n}] on the env's device")
        with torch.cuda.device(dev):
            if self._classes is None or len(self._classes[0]) != n:
                self._classes = (torch.empty(n, dtype=torch.int32, device=dev),
                                 torch.empty(n, dtype=torch.int64, device=dev),
                                 torch.empty(_lib.RX_TRACK_MAX_P + 1, dtype=torch.int32, device=dev))
            ev = self._inplace_io(cdf_score=cdf_score)
            _lib.check(self.L.rx_track_evolve_classes(ctypes.byref(ev), _lib.stream_ptr(stream)),
                       "rx_track_evolve_classes")
        return self._classes

    def spawn_in_place(self, slots, generation, stream=None):
        """New tracks for ``slots`` at ``generation``, each of its slot's own point count, by the
        class table ``classes`` left: rx_track_evolve_inplace into a compact staging buffer.  The
        pool is not written (``commit`` does that) and nothing is downloaded or waited for: the
        host knows every slot's point count, so it forms the staging offsets itself.
        -> ``PendingSpawn``: ``slots`` (ascending, host int32), ``out_off`` (host int32
        [n_spawn + 1], in points), and the device tensors ``cp_out`` float64 [out_off[-1], 2],
        ``width_out`` float64 [n_spawn] and ``plan`` int32 [n_spawn, 4] = (kind, parent or -1,
        P, edits applied)."""
        n = self.n_tracks
        if self._classes is None:
            raise RuntimeError("spawn_in_place needs the class table: call classes(cdf_score) first")
        slots = np.unique(np.asarray(slots, dtype=np.int64).reshape(-1))
        if slots.size and (slots[0] < 0 or slots[-1] >= n):
            raise ValueError(f"slots must lie in [0, {n})")
        g, ns, dev = int(generation) & 0xFFFFFFFF, len(slots), self.cp.device
        out_off = np.concatenate([[0], np.cumsum(np.diff(self.cp_off_host)[slots])]).astype(np.int32)
        slots = slots.astype(np.int32)
        with torch.cuda.device(dev):
            slots_d, out_off_d = torch.from_numpy(slots).to(dev), torch.from_numpy(out_off).to(dev)
            cp_out = torch.empty((int(out_off[-1]), 2), dtype=torch.float64, device=dev)
            width_out = torch.empty(ns, dtype=torch.float64, device=dev)
            plan = torch.zeros((ns, _lib.RX_TRACK_EVOLVE_W), dtype=torch.int32, device=dev)
            ev = self._inplace_io(ns, slots_d, None, plan, out_off_d, cp_out, width_out)
            _lib.check(self.L.rx_track_evolve_inplace(ctypes.byref(ev), g, self.edit_frac, _lib.stream_ptr(stream)),
                       "rx_track_evolve_inplace")
        return PendingSpawn(slots, out_off, cp_out, width_out, plan, g, slots_d, out_off_d)

    def commit(self, pending, stream=None):
        """rx_track_evolve_commit: ``pending``'s staging rows over its slots' spans of the pool;
        every other byte of ``cp`` and ``width`` stays.  One launch, no wait."""
        p = pending
        with torch.cuda.device(self.cp.device):
            ev = self._inplace_io(len(p.slots), p.slots_d, None, None, p.out_off_d, p.cp_out, p.width_out)
            _lib.check(self.L.rx_track_evolve_commit(ctypes.byref(ev), _lib.stream_ptr(stream)),
                       "rx_track_evolve_commit")


PendingSpawn = collections.namedtuple("PendingSpawn",
                                      "slots out_off cp_out width_out plan generation slots_d out_off_d")


class EvolvingCurriculumPPO(ReplayCurriculumPPO):
    """``ReplayCurriculumPPO`` whose retired slots are filled on the device by a
    ``TrackEvolver``: with probability ``evolve_edit`` by an edited child of a track
    drawn from the rank table of the replay scores, else by a fresh track.
    Retirement is unchanged (``_mastered()``: the finish tallies).  Inside a resample:
    the rank tables, the plan, the spawn, the retired slots' tallies and scores start
    again, the tables again, the draw, ``set_tracks``.

    Config key (default): ``evolve_edit`` 0.5, in [0, 1]; every ``ReplayCurriculumPPO``
    key keeps its meaning.  Until the first resample the run equals
    ``ReplayCurriculumPPO``'s bit for bit.  ``resample_tracks(control_points, widths)``
    uploads the given pool into the evolver's buffer.

    Refused as in the parents (a world size above 1, two-car envs), plus a
    ValueError naming ``evolve_edit``, all before any device call."""

    def __init__(self, env_fn, config, device="cuda"):
        edit_frac = check_edit_frac(config.get("evolve_edit", 0.5))
        super().__init__(env_fn, config, device)
        self.evolver = TrackEvolver(self.envs, config["seed"], edit_frac)
        self._cps = self._widths = None  # the pool lives in the evolver's device buffer
        n = self.evolver.n_tracks
        self.lineage = {"parent": np.full(n, -1, dtype=np.int32), "kind": np.full(n, -1, dtype=np.int32),
                        "edits": np.zeros(n, dtype=np.int32), "born": np.zeros(n, dtype=np.int32)}
        self.plans = []  # (generation, slots ascending, plan) of every spawn, oldest first

    def _record(self, generation, slots, plan):
        lin = self.lineage
        lin["kind"][slots], lin["parent"][slots], lin["edits"][slots] = plan[:, 0], plan[:, 1], plan[:, 3]
        lin["born"][slots] = generation
        self.plans.append((int(generation), slots.copy(), plan.copy()))

    def _spawn_tracks(self, generation, retired):
        slots = np.sort(np.asarray(retired, dtype=np.int64))
        self.replay.tables(self.replay_updates)  # the ranks before the retired slots' scores start again
        table, plan = self.evolver.spawn(slots, generation, self.replay.cdf_score)
        self._record(generation, slots, plan)
        return table

    def _replace_tracks(self, generation, slots, control_points, widths):
        self.evolver.load(control_points, widths)  # the whole pool: resample_tracks passes every slot
        n = self.evolver.n_tracks
        self._record(generation, np.arange(n), np.tile(np.array([-1, -1, 0, 0], dtype=np.int32), (n, 1)))
        return self.evolver.table()

    def control_points(self):
        """-> (list of [P, 2] arrays, widths [n_tracks]): the current pool, downloaded."""
        return self.evolver.control_points()

    def track_table(self):
        """``ReplayCurriculumPPO.track_table()`` plus each slot's lineage: ``kind`` (-1 the
        initial pool or a given track, 0 fresh, 1 edit), ``parent`` (the slot of the pool
        before, -1 for none), ``edits`` (applied) and ``born`` (the generation)."""
        tab = super().track_table()
        tab.update({k: v.copy() for k, v in self.lineage.items()})
        return tab


__all__ = ["TrackEvolver", "PendingSpawn", "EvolvingCurriculumPPO", "check_edit_frac", "KINDS"]
