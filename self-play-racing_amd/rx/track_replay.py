"""Track curriculum with replay scores: value-loss scores, rank prioritisation and
staleness on the device.

``CurriculumPPO`` scores a track slot by its finishes alone, so before the first
finish every slot weighs the same, and a slot finished nine times in ten looks
mastered however wrong the critic still is about it.  Here every slot also carries
the learning-potential score of prioritised level replay (Jiang et al. 2021): the
mean GAE magnitude of the data just collected on it.  After every rollout the
advantages [T, N] are summed per slot (one kernel) and folded into the scores; at
a resample the slots are ranked, weighted ``(1 / rank) ** power`` (beta = 1 /
power), and every env draws its slot from a three-way mix: uniform, staleness
(updates since the slot's score was last refreshed) and rank.

``TrackReplay``          the device tensors (learn, score, seen, rank, cdf_score,
                         cdf_stale, track_of_env) and the four calls
                         (rx_track_learn_tally / _fold / _tables / _draw), plus the
                         two of the episodic form (``tally_slots``, ``episode_step``:
                         rx.track_replay_episodic);
``ReplayCurriculumPPO``  ``CurriculumPPO`` with the tally after the GAE launch and
                         the replay draw in ``resample_tracks``.

The rules are csrc/rx_track_replay.h; DESIGN.md §4.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .curriculum import CurriculumPPO


def check_replay_rules(kind, power, alpha, mix, stale_mix):
    """The ranges rx_track_learn_* accept, as ValueErrors naming the config key."""
    if kind not in _lib.TRACK_LEARN_KINDS:
        raise ValueError(f"replay_kind must be one of {sorted(_lib.TRACK_LEARN_KINDS)}, got {kind!r}")
    if not 0 <= int(power) <= _lib.RX_TRACK_LEARN_MAX_POWER:
        raise ValueError(f"replay_power={power} outside 0..{_lib.RX_TRACK_LEARN_MAX_POWER}")
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"replay_alpha={alpha} outside (0, 1]")
    if not 0.0 <= float(mix) <= 1.0:
        raise ValueError(f"curriculum_mix={mix} outside [0, 1]")
    if not 0.0 <= float(stale_mix) <= 1.0:
        raise ValueError(f"replay_stale_mix={stale_mix} outside [0, 1]")
    if not float(mix) + float(stale_mix) <= 1.0:
        raise ValueError(f"curriculum_mix + replay_stale_mix = {mix} + {stale_mix} above 1")
    return _lib.TRACK_LEARN_KINDS[kind], int(power), float(alpha), float(mix), float(stale_mix)


class TrackReplay:
    """The replay scores of ``venv``'s track slots and the draw of its envs over them.

    ``learn`` int64 [n_tracks, 2] = (samples, mag_q), ``score`` float64, ``seen``
    int32 (-1: never scored), ``rank`` int32 (1-based), ``cdf_score`` / ``cdf_stale``
    int64 [n_tracks], ``track_of_env`` int32 [N]: device tensors at fixed addresses,
    so one struct serves every call.  The slot of env e is read from the env's bound
    ``track`` array."""

    def __init__(self, venv, seed, kind="value_l1", power=4, alpha=1.0, mix=0.1, stale_mix=0.1):
        if venv.n_agents != 1:
            raise ValueError("the track replay scores single-agent envs only (DESIGN.md §8)")
        self.kind, self.power, self.alpha, self.mix, self.stale_mix = check_replay_rules(kind, power, alpha, mix,
                                                                                        stale_mix)
        self.L = _lib.load()
        self.venv, self.seed = venv, int(seed) & (2**64 - 1)
        self.n_tracks = n = len(venv._table) if venv._table is not None else len(venv.tracks)
        dev = venv.device
        self.learn = torch.zeros((n, _lib.RX_TRACK_LEARN_W), dtype=torch.int64, device=dev)
        self.score = torch.zeros(n, dtype=torch.float64, device=dev)
        self.seen = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.rank = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
        self.cdf_score = torch.zeros(n, dtype=torch.int64, device=dev)
        self.cdf_stale = torch.zeros(n, dtype=torch.int64, device=dev)
        self.track_of_env = torch.zeros(venv.num_envs, dtype=torch.int32, device=dev)
        self.now = 0  # the `now` of the last tables()
        q = _lib.ptr
        self.lt = _lib.RxTrackLearnIO(n, self.kind, q(venv._st["track"]), q(self.learn), q(self.score), q(self.seen),
                                      q(self.rank), q(self.cdf_score), q(self.cdf_stale), q(self.track_of_env),
                                      self.seed)

    def tally(self, advantages, stream=None):
        """Sum the magnitudes of ``advantages`` (float32 [T, N], contiguous, raw GAE) per
        slot into ``learn`` (rx_track_learn_tally)."""
        n = self.venv.num_envs
        if advantages.dim() != 2 or advantages.shape[1] != n or advantages.dtype != torch.float32 \
                or not advantages.is_contiguous() or advantages.device != self.learn.device:
            raise ValueError(f"rx_track_learn_tally: advantages must be a contiguous float32 [T, {n}] on the env's "
                             f"device, got {tuple(advantages.shape)} {advantages.dtype}")
        _lib.check(self.L.rx_track_learn_tally(ctypes.byref(self.lt), advantages.shape[0], n, _lib.ptr(advantages),
                                               _lib.stream_ptr(stream)), "rx_track_learn_tally")

    def tally_slots(self, advantages, slots, dones=None, stream=None):
        """``tally`` with the slot of every element read from ``slots`` (int32 [T, N], the
        slot env e ran at step t: episodic draws move an env inside a rollout) and, with
        ``dones`` (float32 [T, N], the rollout's done rows), without the autoreset rows
        ``dones[t, e] != 0``, whose advantage belongs to neither the old slot nor the new
        one (rx_track_learn_tally_slots)."""
        n, dev = self.venv.num_envs, self.learn.device
        T = advantages.shape[0] if advantages.dim() == 2 else -1
        for name, x, dtype in (("advantages", advantages, torch.float32), ("slots", slots, torch.int32),
                               ("dones", dones, torch.float32)):
            if x is None and name == "dones":
                continue
            if x is None or tuple(x.shape) != (T, n) or x.dtype != dtype or not x.is_contiguous() or x.device != dev:
                raise ValueError(f"rx_track_learn_tally_slots: {name} must be a contiguous {dtype} [T, {n}] on the "
                                 f"env's device, got {None if x is None else (tuple(x.shape), x.dtype)}")
        _lib.check(self.L.rx_track_learn_tally_slots(ctypes.byref(self.lt), T, n, _lib.ptr(advantages),
                                                     _lib.ptr(slots), _lib.ptr(dones), _lib.stream_ptr(stream)),
                   "rx_track_learn_tally_slots")

    def episode_step(self, curriculum, done=None, stream=None, slot_out=None):
        """``TrackCurriculum.episode_step`` with the next slot drawn from the replay tables
        (rx_track_learn_episode_step): every env whose episode ended in the step just
        enqueued is tallied into ``curriculum.tally`` and takes its next slot from the
        tables ``tables`` left, at its own counter ``curriculum.draws``.  ``slot_out``
        (int32 [N]) receives the slot every env ran in this step."""
        v = self.venv
        ep = curriculum.episodic()
        if slot_out is not None:
            ep = _lib.RxTrackEpisodeIO(ep.draws, None, None, _lib.ptr(slot_out), ep.mix)
        _lib.check(self.L.rx_track_learn_episode_step(v._h, ctypes.byref(curriculum.tc), ctypes.byref(self.lt),
                                                      ctypes.byref(ep), self.stale_mix, v._io_info(),
                                                      _lib.ptr(v.buf["done_f32"] if done is None else done),
                                                      _lib.stream_ptr(stream)), "rx_track_learn_episode_step")
        v._track_ids_stale = True  # the device moved envs between slots: track_ids() downloads them

    def fold(self, update, stream=None):
        """``learn`` -> ``score`` and ``seen`` of the slots that have samples; ``learn``
        starts again (rx_track_learn_fold)."""
        _lib.check(self.L.rx_track_learn_fold(ctypes.byref(self.lt), int(update), self.alpha,
                                              _lib.stream_ptr(stream)), "rx_track_learn_fold")

    def tables(self, now, stream=None):
        """scores -> ``rank`` and the two integer sampling tables (rx_track_learn_tables)."""
        self.now = int(now)
        _lib.check(self.L.rx_track_learn_tables(ctypes.byref(self.lt), self.power, self.now,
                                                _lib.stream_ptr(stream)), "rx_track_learn_tables")

    def draw(self, generation, stream=None):
        """A slot for every env from the current tables (rx_track_learn_draw) -> ``track_of_env``."""
        _lib.check(self.L.rx_track_learn_draw(ctypes.byref(self.lt), self.venv.num_envs,
                                              int(generation) & 0xFFFFFFFF, self.mix, self.stale_mix,
                                              _lib.stream_ptr(stream)), "rx_track_learn_draw")
        return self.track_of_env

    def reset_slots(self, idx):
        """The slots ``idx`` start again as never scored (their tracks were replaced)."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size:
            if idx.min() < 0 or idx.max() >= self.n_tracks:
                raise ValueError(f"slots must lie in [0, {self.n_tracks})")
            i = torch.from_numpy(idx).to(self.learn.device)
            self.learn[i] = 0
            self.score[i] = 0.0
            self.seen[i] = -1

    def table(self, now=None):
        """The host view per slot, arrays of length n_tracks: score, seen, rank,
        staleness (``now`` - seen; 0 for a slot never scored) and prob, the draw
        probability of the slot under the current scores.  Runs ``tables`` (at
        ``now``, default the last one) and downloads; call it between updates."""
        self.tables(self.now if now is None else now)
        n = self.n_tracks

        def weights(cdf):
            c = cdf.cpu().numpy().astype(np.uint64)
            return np.diff(np.concatenate([[np.uint64(0)], c])).astype(np.float64), float(c[-1])

        w, F = weights(self.cdf_score)
        s, Fs = weights(self.cdf_stale)
        uniform = np.full(n, 1.0 / n)
        by_score = uniform if F == 0 else w / F
        stale_mix = self.stale_mix if Fs > 0 else 0.0
        prob = self.mix * uniform + stale_mix * (s / Fs if Fs > 0 else 0.0) + (1.0 - self.mix - stale_mix) * by_score
        return {"score": self.score.cpu().numpy(), "seen": self.seen.cpu().numpy(), "rank": self.rank.cpu().numpy(),
                "staleness": s.astype(np.int64), "prob": prob}


class ReplayCurriculumPPO(CurriculumPPO):
    """``CurriculumPPO`` whose resample draws the envs by the replay scores: after
    every rollout's GAE launch the raw advantages are tallied per track slot and
    folded into the scores (two launches on the same stream, outside the rollout
    graph), and ``resample_tracks`` ranks the slots and draws from the uniform /
    staleness / rank mix.  The finish tallies are kept as in ``CurriculumPPO`` and
    still decide which slots are retired; a retired slot starts again as never
    scored, which ranks it first.

    Config keys (defaults): ``replay_kind`` "value_l1" (mean |A|; or "value_pos",
    mean max(A, 0)), ``replay_power`` 4 (beta = 1 / power), ``replay_alpha`` 1.0 (the
    score's moving-average step), ``replay_stale_mix`` 0.1; ``curriculum_mix`` stays
    the uniform part, and ``curriculum_mix + replay_stale_mix <= 1``.  Every other
    ``CurriculumPPO`` key keeps its meaning.

    The rank weight is steep: at power 4 the rank-1 slot alone holds 1 / zeta(4) =
    92 % of the rank part, and every env is drawn at once, so about three envs in
    four land on one slot; a smaller ``replay_power`` flattens it.

    Until the first resample the training run equals ``CurriculumPPO``'s bit for
    bit.  Refused as in ``CurriculumPPO``, plus ValueErrors naming the bad key."""

    def __init__(self, env_fn, config, device="cuda"):
        c = config
        self._replay_rules = (c.get("replay_kind", "value_l1"), c.get("replay_power", 4), c.get("replay_alpha", 1.0),
                              c.get("curriculum_mix", 0.1), c.get("replay_stale_mix", 0.1))
        check_replay_rules(*self._replay_rules)
        super().__init__(env_fn, config, device)
        self.replay = TrackReplay(self.envs, c["seed"], *self._replay_rules)
        self.replay_updates = 0  # the folds so far: the index of the next update

    def compute_advantages(self, rewards, dones, values, next_value, next_done):
        advantages, returns = super().compute_advantages(rewards, dones, values, next_value, next_done)
        self.replay.tally(advantages)  # the raw GAE output, before ppo_update's per-minibatch normalisation
        self.replay.fold(self.replay_updates)
        self.replay_updates += 1
        return advantages, returns

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


__all__ = ["TrackReplay", "ReplayCurriculumPPO", "check_replay_rules"]
