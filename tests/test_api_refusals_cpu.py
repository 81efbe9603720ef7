"""Every refusal of the C ABI that needs neither a handle nor a device, byte for byte.

A table of bad calls -- ctypes, numpy host arrays and null handles only -- whose (return code,
rx_last_error()) pairs are compared with tests/golden/api_refusals.json.  The other CPU tests match
substrings, which a reworded or reordered refusal slips past; this one pins the text, the code and,
with the cases that have two bad arguments, the order of the checks.  It covers both twins of every
device / host pair of include/rx.h and the handle-bound entry points up to their `null handle`.

    RX_LIB_PATH=/path/to/librx.so python tests/test_api_refusals_cpu.py --record

writes the golden file from the library RX_LIB_PATH names.  Record it from the library of the commit
whose behaviour is to be kept (a build of the parent revision: tools/build_rev.py), never from the
code under test.

Every case must be refused, or return before anything is read (the in-place evolve stages with
nothing to spawn): a case that passed its checks would launch on a device or write through the
placeholder pointers.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))

from rx import _lib  # noqa: E402

PAD = np.zeros(4096, dtype=np.uint8)  # what every pointer that is never followed points to
P = PAD.ctypes.data
NAN = float("nan")
I32 = np.int32


def S(cls, **ints):
    """A struct argument: its pointer fields point to PAD, its other fields are `ints` (default 0)."""
    return (cls, ints)


# The 25 device / host pairs of include/rx.h: name -> the parameters of a call that would pass every check
# (were its pointers real), in order.  A case overrides some of them; "lg.n_slots" is a field of struct lg.
TC = S(_lib.RxTrackIO, n_tracks=4)
TD = S(_lib.RxTrackDuelIO)
EP = S(_lib.RxTrackEpisodeIO, mix=0.25)
LT = S(_lib.RxTrackLearnIO, n_tracks=4)
LG = S(_lib.RxLeagueIO, n_slots=4, params_stride=1 << 20)
EV = S(_lib.RxTrackEvolveIO, n_tracks=4, n_spawn=2)
EVI = S(_lib.RxTrackEvolveInplaceIO, n_tracks=4, n_spawn=2)
RIO = S(_lib.RxRasterIO, K=1, A=1, size=64, n_envs=1, n_layers=1, out_pitch=192, out_size=192 * 64)
ROWS = [("n", 8), ("done", P), ("terminated", P), ("info", P), ("stream", None)]
CP3 = np.array([[0.0, 0.0], [100.0, 0.0], [50.0, 80.0]])
TABLE = [("n", 2), ("wp_off", np.array([0, 4, 8], I32)), ("wp", P), ("nrm", P), ("seg", P), ("meta", P), ("G", 4),
         ("SG", 2), ("t", S(_lib.RxCullTables)), ("p", S(_lib.RxTrackPatch, n_upd=1)), ("stream", None)]
PAIRS = {
    "rx_build_tracks": [("n", 1), ("factor", 4), ("cp_off", np.array([0, 3], I32)), ("cp", CP3), ("width", np.array([10.0])),
                        ("wp_off", np.zeros(2, I32)), ("wp", P), ("nrm", P), ("seg", P), ("meta", P), ("stream", None)],
    "rx_build_cull_tables": [p for p in TABLE if p[0] not in ("nrm", "p")],
    "rx_patch_tracks": TABLE,
    "rx_raster_static": [("n", 1), ("size", 64), ("n_edges", 4), ("edge_off", P), ("edges", P), ("layer", P), ("stream", None)],
    "rx_raster_trail": [("r", RIO), ("stream", None)],
    "rx_raster_frame": [("r", RIO), ("stream", None)],
    "rx_league_weights": [("lg", LG), ("n_live", 2), ("power", 1), ("mix", 0.5), ("prior", 1.0), ("stream", None)],
    "rx_league_draw": [("lg", LG), ("n", 8), ("done", None), ("info", None), ("stream", None)],
    "rx_track_tally": [("tc", TC)] + ROWS,
    "rx_track_scores": [("tc", TC), ("power", 1), ("prior", 1.0), ("stream", None)],
    "rx_track_draw": [("tc", TC), ("n", 8), ("generation", 3), ("mix", 0.5), ("stream", None)],
    "rx_track_tally2": [("tc", TC), ("td", TD)] + ROWS,
    "rx_track_duel_scores": [("tc", TC), ("td", TD), ("power", 1), ("prior", 1.0), ("stream", None)],
    "rx_track_episode": [("tc", TC), ("ep", EP)] + ROWS,
    "rx_track_learn_tally": [("lt", LT), ("T", 4), ("n", 8), ("adv", P), ("stream", None)],
    "rx_track_learn_fold": [("lt", LT), ("update", 1), ("alpha", 0.5), ("stream", None)],
    "rx_track_learn_tables": [("lt", LT), ("power", 1), ("now", 1), ("stream", None)],
    "rx_track_learn_draw": [("lt", LT), ("n", 8), ("generation", 3), ("mix", 0.25), ("stale_mix", 0.25), ("stream", None)],
    "rx_track_learn_tally_slots": [("lt", LT), ("T", 4), ("n", 8), ("adv", P), ("slots", P), ("dones", P), ("stream", None)],
    "rx_track_learn_episode": [("tc", TC), ("lt", LT), ("ep", EP), ("stale_mix", 0.25)] + ROWS,
    "rx_track_evolve_plan": [("ev", EV), ("generation", 3), ("edit_frac", 0.5), ("stream", None)],
    "rx_track_evolve": [("ev", EV), ("generation", 3), ("stream", None)],
    "rx_track_evolve_classes": [("ev", EVI), ("stream", None)],
    "rx_track_evolve_inplace": [("ev", EVI), ("generation", 3), ("edit_frac", 0.5), ("stream", None)],
    "rx_track_evolve_commit": [("ev", EVI), ("stream", None)],
}
# The handle-bound entries, called with a null handle: what they refuse before they look at it.
IO, RO, SP = S(_lib.RxIO), S(_lib.RxRolloutIO, T=4, obs_dim=15), S(_lib.RxSelfplayIO)
SINGLES = {
    "rx_cull_table_sizes": [("n", 2), ("wp_off", np.array([0, 4, 8], I32)), ("G", 4), ("SG", 2), ("out", np.zeros(4, np.int64))],
    "rx_reset": [("h", None), ("mask", None), ("io", IO), ("stream", None)],
    "rx_step": [("h", None), ("io", IO), ("stream", None)],
    "rx_step_phases": [("h", None), ("io", IO), ("phases", 3), ("stream", None)],
    "rx_steps": [("h", None), ("io", IO), ("n_steps", 4), ("strides", None), ("stream", None)],
    "rx_rollout": [("h", None), ("io", IO), ("r", RO), ("stream", None)],
    "rx_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("precision", 0), ("stream", None)],
    "rx_selfplay_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("sp", SP), ("precision", 0), ("stream", None)],
    "rx_eval_steps": [("h", None), ("io", IO), ("ev", S(_lib.RxEvalIO, obs_dim=15)), ("n_steps", 4), ("stream", None)],
    "rx_match_steps": [("h", None), ("io", IO), ("m", S(_lib.RxMatchIO, obs_dim=15)), ("n_steps", 4), ("stream", None)],
    "rx_upload_tracks_device": [("h", None), ("n", 2), ("wp_off", P), ("wp", P), ("nrm", P), ("seg", P), ("meta", P),
                                ("stream", None)],
    "rx_replace_tracks_device": [("h", None), ("p", S(_lib.RxTrackPatch, n_upd=1)), ("stream", None)],
    "rx_league_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("sp", SP), ("lg", LG), ("precision", 0), ("stream", None)],
    "rx_track_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("tc", TC), ("precision", 0), ("stream", None)],
    "rx_track_duel_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("sp", SP), ("lg", None), ("tc", TC), ("td", TD),
                                    ("precision", 0), ("stream", None)],
    "rx_track_episode_step": [("h", None), ("tc", TC), ("ep", EP), ("io", IO), ("done", None), ("stream", None)],
    "rx_track_episodic_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("tc", TC), ("ep", EP), ("slots", None),
                                        ("precision", 0), ("stream", None)],
    "rx_track_learn_episode_step": [("h", None), ("tc", TC), ("lt", LT), ("ep", EP), ("stale_mix", 0.25), ("io", IO),
                                    ("done", None), ("stream", None)],
    "rx_track_learn_episodic_rollout_steps": [("h", None), ("io", IO), ("r", RO), ("tc", TC), ("lt", LT), ("ep", EP),
                                              ("stale_mix", 0.25), ("slots", None), ("precision", 0), ("stream", None)],
}

# ---- the cases: (case name, overrides); one per fail( site, then a few with two bad arguments ----------
ROWS_BAD = [("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}), ("done", {"done": None}), ("terminated", {"terminated": None}),
            ("info", {"info": None}), ("n,done", {"n": 0, "done": None})]
SCALARS4 = [("power<0", {"power": -1}), ("power>4", {"power": 5}), ("prior=0", {"prior": 0.0}), ("prior=nan", {"prior": NAN}),
            ("power,prior", {"power": 9, "prior": -1.0})]
TRACK0 = [("tc", {"tc": None}), ("n_tracks", {"tc.n_tracks": 0}), ("track", {"tc.track": None}), ("tally", {"tc.tally": None})]
TRACK1 = [("tc", {"tc": None}), ("n_tracks", {"tc.n_tracks": 0}), ("tally", {"tc.tally": None}), ("cdf", {"tc.cdf": None}),
          ("p", {"tc.p": None})]
DUEL = [("td", {"td": None}), ("td.agent", {"td.agent": 2}), ("duel", {"td.duel": None})]
EPISODE = [("ep", {"ep": None}), ("draws", {"ep.draws": None}), ("env_pos", {"ep.env_pos": None}),
           ("pos_slot", {"ep.pos_slot": None}), ("ep.mix", {"ep.mix": 1.5}), ("ep.mix=nan", {"ep.mix": NAN})]
LEARN_IO = [("lt", {"lt": None}), ("lt.n_tracks", {"lt.n_tracks": 0})]
STALE = [("stale_mix", {"stale_mix": -0.5}), ("stale_mix=nan", {"stale_mix": NAN}),
         ("cdf_stale", {"lt.cdf_stale": None}), ("stale,cdf_stale", {"stale_mix": 2.0, "lt.cdf_stale": None})]
LEARN_EPISODE = (TRACK0 + EPISODE + LEARN_IO +
                 [("n_tracks differ", {"lt.n_tracks": 5}), ("cdf_score", {"lt.cdf_score": None}),
                  ("mix+stale", {"ep.mix": 0.75, "stale_mix": 0.75})] + STALE)
LEAGUE0 = [("lg", {"lg": None}), ("n_slots=0", {"lg.n_slots": 0}), ("n_slots=65", {"lg.n_slots": 65}),
           ("tally", {"lg.tally": None}), ("cdf", {"lg.cdf": None})]
LEAGUE1 = LEAGUE0 + [("lg.agent", {"lg.agent": 2}), ("opp_id", {"lg.opp_id": None}), ("draw_count", {"lg.draw_count": None})]
LEAGUE2 = LEAGUE1 + [("params", {"lg.params": None}), ("log_std", {"lg.log_std": None}),
                     ("params_stride", {"lg.params_stride": 8}), ("opp_precision", {"lg.opp_precision": 7})]
EVOLVE_IO = [("ev", {"ev": None}), ("n_tracks", {"ev.n_tracks": 0}), ("n_spawn<0", {"ev.n_spawn": -1}),
             ("n_spawn>n", {"ev.n_spawn": 5}), ("slots", {"ev.slots": None}), ("plan", {"ev.plan": None}),
             ("cp_off", {"ev.cp_off": None}), ("n_spawn,slots", {"ev.n_spawn": 9, "ev.slots": None})]


def nulls(prefix, fields):
    return [(prefix + f, {prefix + f: None}) for f in fields]


INPLACE = [("ev", {"ev": None}), ("n_tracks", {"ev.n_tracks": 0}), ("n_spawn<0", {"ev.n_spawn": -1}),
           ("n_spawn>n", {"ev.n_spawn": 5})]
RASTER_IO = ([("r", {"r": None}), ("size<", {"r.size": 8}), ("size>", {"r.size": 4096}), ("A", {"r.A": 3}), ("K=0", {"r.K": 0}),
              ("K>", {"r.K": 65536}), ("n_envs", {"r.n_envs": 0}), ("size,A", {"r.size": 0, "r.A": 0})] +
             nulls("r.", ["env_ids", "x", "y", "view", "trail"]))
PRECISION = [("precision", {"precision": 7})]
NULL_H = [("null handle", {})]
TABLE_BAD = ([("n=0", {"n": 0})] + nulls("", ["wp_off", "wp", "seg", "meta", "t"]) +
             nulls("t.", ["seg_f", "slot_hdr", "chunk_off", "super_box_f"]) +
             [("SG<0", {"SG": -1}), ("SG>64", {"SG": 65}), ("wp_off[0]", {"wp_off": np.array([1, 4, 8], I32)}),
              ("W<2", {"wp_off": np.array([0, 1, 8], I32)}), ("W>max", {"wp_off": np.array([0, 4, 4000], I32)}),
              ("n,wp_off", {"n": -1, "wp_off": None})])
PATCH_OK = {"p.slots": np.array([1], I32), "p.src_off": np.array([0, 4], I32)}


def patch(**o):
    return dict(PATCH_OK, **o)


CASES = {
    "rx_build_tracks": [("n=0", {"n": 0}), ("cp_off", {"cp_off": None}), ("meta", {"meta": None}), ("factor", {"factor": 0}),
                        ("cp_off[0]", {"cp_off": np.array([1, 4], I32)}), ("P<3", {"cp_off": np.array([0, 2], I32)}),
                        ("P>64", {"cp_off": np.array([0, 65], I32)}), ("W>max", {"cp_off": np.array([0, 64], I32), "factor": 33}),
                        ("sum", {"n": (1 << 20) + 1, "cp_off": (np.arange((1 << 20) + 2, dtype=np.int64) * 64).astype(I32),
                                 "factor": 32}),
                        ("n,factor", {"n": 0, "factor": 0})],
    "rx_build_tracks_host": [("coord", {"cp": np.array([[0.0, 0.0], [NAN, 0.0], [50.0, 80.0]])}),
                             ("chord", {"cp": np.array([[0.0, 0.0], [0.0, 0.0], [50.0, 80.0]])}),
                             ("width", {"width": np.array([-1.0])})],
    "rx_cull_table_sizes": [("out", {"out": None}), ("n=0", {"n": 0}), ("wp_off", {"wp_off": None}), ("SG>64", {"SG": 65}),
                            ("W<2", {"wp_off": np.array([0, 1, 8], I32)})],
    "rx_build_cull_tables": TABLE_BAD,
    "rx_patch_tracks": ([c for c in TABLE_BAD if c[0] != "t"] + nulls("", ["nrm", "p"]) + nulls("p.", ["slots", "meta"]) +
                        [("n_upd=0", patch(**{"p.n_upd": 0})), ("n_upd>n", patch(**{"p.n_upd": 3})),
                         ("src_off[0]", patch(**{"p.src_off": np.array([1, 5], I32)})),
                         ("slot range", patch(**{"p.slots": np.array([2], I32)})),
                         ("ascending", patch(**{"p.n_upd": 2, "p.slots": np.array([1, 1], I32),
                                                "p.src_off": np.array([0, 4, 8], I32)})),
                         ("count", patch(**{"p.src_off": np.array([0, 5], I32)})),
                         ("no tables: count", patch(**{"t": None, "p.src_off": np.array([0, 5], I32)}))]),
    "rx_patch_tracks_host": [("meta width", patch(**{"t": None, "p.meta": np.array([0, 0, 0, -1.0, 1, 0, 0, 0])})),
                             ("meta reach", patch(**{"t": None, "p.meta": np.array([0, 0, 0, 1.0, NAN, 0, 0, 0])}))],
    "rx_raster_static": [("n=0", {"n": 0}), ("n>", {"n": 65536}), ("size<", {"size": 8}), ("size>", {"size": 4096}),
                         ("n_edges", {"n_edges": -1}), ("edge_off", {"edge_off": None}), ("edges", {"edges": None}),
                         ("layer", {"layer": None}), ("n,size", {"n": 0, "size": 0})],
    "rx_raster_trail": RASTER_IO + nulls("r.", ["last"]),
    "rx_raster_frame": (RASTER_IO + nulls("r.", ["angle", "layer_of", "layer", "out", "out_off"]) +
                        [("n_layers", {"r.n_layers": 0}), ("out_pitch<0", {"r.out_pitch": -1}),
                         ("out_pitch<3*size", {"r.out_pitch": 100}), ("out_size", {"r.out_size": -1}),
                         ("out,n_layers", {"r.out": None, "r.n_layers": 0})]),
    "rx_league_weights": (LEAGUE0 + [("n_live=0", {"n_live": 0}), ("n_live>", {"n_live": 5}), ("mix<0", {"mix": -0.1}),
                                     ("mix>1", {"mix": 1.5}), ("mix=nan", {"mix": NAN}), ("mix,prior", {"mix": 2.0, "prior": 0.0}),
                                     ("power,mix", {"power": 5, "mix": 2.0})] + SCALARS4),
    "rx_league_draw": LEAGUE1 + [("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}), ("info", {"done": P}),
                                 ("agent,n", {"lg.agent": -1, "n": 0})],
    "rx_track_tally": TRACK0 + ROWS_BAD + [("track,n", {"tc.track": None, "n": 0})],
    "rx_track_scores": (TRACK1 + SCALARS4 + [("score=2", {"tc.score": 2}), ("score<0", {"tc.score": -1}),
                                             ("score,power", {"tc.score": 2, "power": 5})]),
    "rx_track_draw": ([("tc", {"tc": None}), ("n_tracks", {"tc.n_tracks": 0}), ("cdf", {"tc.cdf": None}),
                       ("track_of_env", {"tc.track_of_env": None}), ("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}),
                       ("mix<0", {"mix": -0.5}), ("mix=nan", {"mix": NAN}), ("n,mix", {"n": 0, "mix": 2.0})]),
    "rx_track_tally2": TRACK0 + DUEL + ROWS_BAD + [("tally,td", {"tc.tally": None, "td": None}),
                                                   ("duel,n", {"td.duel": None, "n": 0})],
    "rx_track_duel_scores": (TRACK1 + [("score=4", {"tc.score": 4}), ("score<0", {"tc.score": -1})] + DUEL + SCALARS4 +
                             [("score,td", {"tc.score": 4, "td": None}), ("duel,power", {"td.duel": None, "power": 5})]),
    "rx_track_episode": (TRACK0 + [("cdf", {"tc.cdf": None})] + EPISODE + ROWS_BAD +
                         [("cdf,ep", {"tc.cdf": None, "ep": None}), ("mix,n", {"ep.mix": 2.0, "n": 0})]),
    "rx_track_learn_tally": LEARN_IO + [("kind", {"lt.kind": 2}), ("track", {"lt.track": None}), ("learn", {"lt.learn": None}),
                                        ("T", {"T": 0}), ("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}), ("adv", {"adv": None}),
                                        ("kind,T", {"lt.kind": 2, "T": 0}), ("T,n", {"T": 0, "n": 0})],
    "rx_track_learn_fold": (LEARN_IO + nulls("lt.", ["learn", "score", "seen"]) +
                            [("alpha=0", {"alpha": 0.0}), ("alpha>1", {"alpha": 1.5}), ("alpha=nan", {"alpha": NAN})]),
    "rx_track_learn_tables": (LEARN_IO + nulls("lt.", ["score", "seen", "rank", "cdf_score", "cdf_stale"]) +
                              [("power<0", {"power": -1}), ("power>10", {"power": 11}), ("now", {"now": -1}),
                               ("power,now", {"power": 11, "now": -1})]),
    "rx_track_learn_draw": (LEARN_IO + nulls("lt.", ["cdf_score", "track_of_env"]) +
                            [("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}), ("mix", {"mix": 1.5}), ("mix=nan", {"mix": NAN}),
                             ("mix+stale", {"mix": 0.75, "stale_mix": 0.75}), ("n,mix", {"n": 0, "mix": 2.0})] + STALE),
    "rx_track_learn_tally_slots": LEARN_IO + [("kind", {"lt.kind": -1}), ("learn", {"lt.learn": None}), ("T", {"T": 0}),
                                              ("n=0", {"n": 0}), ("n=2^31", {"n": 1 << 31}), ("adv", {"adv": None}),
                                              ("slots", {"slots": None}), ("adv,slots", {"adv": None, "slots": None})],
    "rx_track_learn_episode": LEARN_EPISODE + ROWS_BAD + [("ep.mix,lt", {"ep.mix": 2.0, "lt": None}),
                                                          ("cdf_score,n", {"lt.cdf_score": None, "n": 0})],
    "rx_track_evolve_plan": EVOLVE_IO + [("cdf_score", {"ev.cdf_score": None}), ("edit_frac", {"edit_frac": 1.5}),
                                         ("edit_frac=nan", {"edit_frac": NAN}),
                                         ("cdf_score,edit_frac", {"ev.cdf_score": None, "edit_frac": 2.0})],
    "rx_track_evolve": EVOLVE_IO + nulls("ev.", ["cp", "width", "cp_off_new", "cp_new", "width_new"]),
    "rx_track_evolve_classes": INPLACE + nulls("ev.", ["cp_off", "cdf_score", "order", "cdf_class", "class_end"]),
    "rx_track_evolve_inplace": (INPLACE + [("edit_frac", {"edit_frac": -0.5}),
                                           ("nothing to spawn", {"ev.n_spawn": 0, "ev.slots": None}),
                                           ("edit_frac, nothing to spawn", {"edit_frac": 2.0, "ev.n_spawn": 0})] +
                                nulls("ev.", ["slots", "cp_off", "cp", "width", "order", "cdf_class", "class_end", "plan", "out_off",
                                              "cp_out", "width_out"])),
    "rx_track_evolve_commit": (INPLACE + [("nothing to spawn", {"ev.n_spawn": 0, "ev.slots": None})] +
                               nulls("ev.", ["slots", "cp_off", "cp", "width", "out_off", "cp_out", "width_out"])),
    # the handle-bound entries, up to and including their null handle
    "rx_reset": NULL_H, "rx_step": NULL_H, "rx_steps": NULL_H, "rx_rollout": NULL_H, "rx_rollout_steps": NULL_H,
    "rx_selfplay_rollout_steps": NULL_H, "rx_eval_steps": NULL_H, "rx_match_steps": NULL_H,
    "rx_upload_tracks_device": NULL_H, "rx_replace_tracks_device": NULL_H,
    "rx_step_phases": NULL_H + [("phases=0", {"phases": 0}), ("phases=4", {"phases": 4})],
    "rx_league_rollout_steps": LEAGUE2 + PRECISION + NULL_H + [("opp_precision,precision", {"lg.opp_precision": 7,
                                                                                            "precision": 7})],
    "rx_track_rollout_steps": TRACK0 + PRECISION + NULL_H + [("tally,precision", {"tc.tally": None, "precision": 7})],
    "rx_track_duel_rollout_steps": (TRACK0 + DUEL + PRECISION + NULL_H +
                                    [("lg." + n, dict(o, lg=LG) if "lg" not in o else o) for n, o in LEAGUE2[1:]] +
                                    [("duel,precision", {"td.duel": None, "precision": 7})]),
    "rx_track_episode_step": TRACK0 + [("cdf", {"tc.cdf": None})] + EPISODE + NULL_H,
    "rx_track_episodic_rollout_steps": TRACK0 + [("cdf", {"tc.cdf": None})] + EPISODE + PRECISION + NULL_H +
                                       [("mix,precision", {"ep.mix": 2.0, "precision": 7})],
    "rx_track_learn_episode_step": LEARN_EPISODE + NULL_H,
    "rx_track_learn_episodic_rollout_steps": (LEARN_EPISODE + PRECISION + NULL_H +
                                              [("cdf_stale,precision", {"lt.cdf_stale": None, "precision": 7})]),
}
# the twins differ: with nothing to spawn the device form of the plan returns before its launch, the host twin runs
DEVICE_ONLY = {"rx_track_evolve_plan": [("nothing to spawn", {"ev.n_spawn": 0, "ev.slots": None, "ev.plan": None})]}


def build(params, over, keep):
    """The ctypes arguments of one call: params with the case's overrides applied."""
    args = []
    unused = set(over)
    for name, value in params:
        if name in over:
            value = over[name]
            unused.discard(name)
        if isinstance(value, tuple):  # a struct: pointer fields -> PAD, the rest from its defaults
            cls, ints = value
            s = cls()
            for field, ftype in ((f[0], f[1]) for f in cls._fields_):
                key = name + "." + field
                v = over[key] if key in over else ints.get(field, P if ftype is ctypes.c_void_p else 0)
                unused.discard(key)
                if isinstance(v, np.ndarray):
                    keep.append(v)
                    v = v.ctypes.data
                if ftype is ctypes.c_void_p or v is not None:
                    setattr(s, field, v)
            keep.append(s)
            value = ctypes.byref(s)
        elif isinstance(value, np.ndarray):
            keep.append(value)
            value = value.ctypes.data
        args.append(value)
    assert not unused, f"overrides that name no parameter: {unused}"
    return args


def calls():
    """(case id, function name, parameters, overrides) of every call of the table."""
    for fn, params in PAIRS.items():
        for sfx in ("", "_host"):
            cases = CASES[fn] + CASES.get(fn + "_host", []) * (sfx == "_host") + DEVICE_ONLY.get(fn, []) * (sfx == "")
            for case, over in cases:
                yield f"{fn}{sfx}: {case}", fn + sfx, params, over
    for fn, params in SINGLES.items():
        for case, over in CASES[fn]:
            yield f"{fn}: {case}", fn, params, over


def run_all(L):
    out = {}
    for cid, fn, params, over in calls():
        assert cid not in out, cid
        keep = []
        rc = getattr(L, fn)(*build(params, over, keep))
        out[cid] = [rc, L.rx_last_error().decode() if rc else ""]
    return out


@pytest.fixture(scope="module")
def results():
    return run_all(_lib.load())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_pair_of_the_header_is_in_the_table():
    import re
    text = open(os.path.join(ROOT, "include", "rx.h")).read()
    hosts = set(re.findall(r"^int (rx_\w+)_host\(", text, flags=re.M))
    assert len(hosts) == 25 and hosts == set(PAIRS)
    assert all(re.search(rf"^int {fn}\(", text, flags=re.M) for fn in hosts)


def test_refusals_match_the_recorded_ones(results, golden):
    assert set(results) == set(golden)
    wrong = {cid: (results[cid], golden[cid]) for cid in golden if results[cid] != golden[cid]}
    assert not wrong, wrong


def test_only_the_listed_cases_return_ok(results):
    ok = sorted(cid for cid, (rc, _) in results.items() if rc == 0)
    assert ok == sorted(cid for cid in results if "nothing to spawn" in cid and "edit_frac," not in cid)


def test_twins_agree_where_the_recorded_twins_agree(results, golden):
    """Up to the function's name, a host twin refuses as its device form does -- wherever the
    recorded library's twins do."""
    n = 0
    for fn in PAIRS:
        for case, _ in CASES[fn]:
            dev, host = f"{fn}: {case}", f"{fn}_host: {case}"
            def same(r):
                return r[host] == [r[dev][0], r[dev][1].replace(fn + ":", fn + "_host:", 1)]
            if same(golden):
                n += 1
                assert same(results), (results[dev], results[host])
    assert n >= 356  # every shared case of the table, as recorded


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    assert os.environ.get("RX_LIB_PATH"), "set RX_LIB_PATH to the library to record from"
    res = run_all(_lib.load(build_if_missing=False))
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(res)} cases -> {GOLDEN}")
