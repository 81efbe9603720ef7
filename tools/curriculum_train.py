"""Single-agent training with the track curriculum (rx.curriculum), against uniform sampling.

    python tools/curriculum_train.py --envs 4096 --steps 128 --updates 60 --tracks 512 --resample-every 4
    python tools/curriculum_train.py --envs 64 --steps 32 --updates 6 --tracks 8 --resample-every 2 --no-uniform
    python tools/curriculum_train.py --replay value_l1 --envs 4096 --steps 128 --updates 60 --tracks 512
    python tools/curriculum_train.py --evolve --envs 4096 --steps 128 --updates 60 --tracks 512
    python tools/curriculum_train.py --episodic --envs 4096 --steps 128 --updates 60 --tracks 512
    python tools/curriculum_train.py --episodic --replay value_l1 --envs 4096 --steps 128 --updates 60 --tracks 512
    python tools/curriculum_train.py --episodic --partial --evolve --envs 4096 --steps 128 --updates 60 --tracks 512
    python tools/curriculum_train.py --episodic --regroup-every 1 --envs 4096 --steps 128 --updates 60 --tracks 512

``CurriculumPPO`` on a pool of ``--tracks`` distinct tracks (env i starts on slot
i % tracks): every finished episode is tallied against its slot on the device;
every ``--resample-every`` updates the envs are redrawn over the slots, weighted
towards the tracks the learner still fails, and the mastered slots are retired for
fresh tracks.  Unless ``--no-uniform``, a plain ``PPO`` run of equal env-steps on
the same pool and the same cadence (``PPO.resample_tracks``: a blind new pool)
follows.  Both are evaluated every ``--eval-every`` updates and at the end with
rx.evaluate's protocol (40 held-out tracks x 5 runs, fused backend); the success
rates over env-steps, the first evaluation at or above 90 % and the curriculum's
per-slot table go to ``--out`` as JSON, and the table's most failed slots are
printed.  With ``--replay value_l1`` (or ``value_pos``) the curriculum run is
``rx.track_replay.ReplayCurriculumPPO``: the redraw follows the value-loss scores
of the rollouts (rank prioritisation ``--replay-power``, staleness ``--stale-mix``)
instead of the finish tallies; ``off`` (the default) runs ``CurriculumPPO``.
With ``--evolve`` it is ``rx.track_evolve.EvolvingCurriculumPPO``: the replay draw
(``--replay``, value_l1 when left off) and the retired slots filled on the device,
a fraction ``--evolve-edit`` of them by edited children of high-ranked tracks.
With ``--episodic`` it is ``rx.track_episodic.EpisodicCurriculumPPO``: an env draws
its next slot when its own episode ends, no episode is dropped, and a resample
with nothing to retire resets nobody; with ``--replay`` as well it is
``rx.track_replay_episodic.EpisodicReplayCurriculumPPO``, whose ended envs draw
from the value-loss scores (prioritised level replay per episode).  ``--episodic
--partial`` (``episodic_partial``) also replaces the retired slots in place, so a
resample that retires slots resets only the envs on them.  ``--episodic --partial
--evolve`` (``--evolve-edit`` as above) is
``rx.track_evolve_episodic.EpisodicEvolvingCurriculumPPO``: those retired slots are
filled on the device, by fresh tracks and by edited children of high-ranked tracks
of the slot's own point count.  ``--episodic --evolve`` without ``--partial`` is
refused: only the partial path keeps a slot's point count, and the global path
of ``--evolve`` rebuilds the table the episodic draws run on.  ``--episodic
--regroup-every K`` (``episodic_regroup_every``) puts the envs' positions back in slot
order on the device before the rollout of every K-th update (scheduling only).  Every curriculum run also reports the
episodes tallied per update, the slots that reached ``--min-episodes`` and, per
update, the share of the envs on the fullest slot (with replay scores also on the
slot ranked first).
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))


def run(kind, args, evaluator):
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.ppo import PPO
    from rx.track import gen_tracks
    cfg = base_config(num_envs=args.envs, num_steps=args.steps, seed=args.seed, shuffle="device",
                      track_resample_every=args.resample_every, policy_dtype=args.prec,
                      curriculum_power=args.power, curriculum_mix=args.mix, curriculum_prior=args.prior,
                      curriculum_score=args.score, curriculum_refresh=args.refresh, curriculum_mastery=args.mastery,
                      curriculum_min_episodes=args.min_episodes)
    cfg["total_timesteps"] = args.updates * cfg["batch_size"]
    evolve = kind == "curriculum" and args.evolve
    replay_kind = "value_l1" if evolve and args.replay == "off" else args.replay
    replay = kind == "curriculum" and replay_kind != "off"
    if replay:
        cfg.update(replay_kind=replay_kind, replay_power=args.replay_power, replay_alpha=args.replay_alpha,
                   replay_stale_mix=args.stale_mix)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    rng = np.random.RandomState(args.seed)
    pool = gen_tracks(args.tracks, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(args.tracks)]
    n = args.tracks
    cls = CurriculumPPO if kind == "curriculum" else PPO
    if replay:
        from rx.track_replay import ReplayCurriculumPPO as cls
    if evolve:
        from rx.track_evolve import EvolvingCurriculumPPO as cls
        cfg["evolve_edit"] = args.evolve_edit
    episodic = kind == "curriculum" and args.episodic
    if episodic:
        from rx.track_episodic import EpisodicCurriculumPPO as cls
        if replay:
            from rx.track_replay_episodic import EpisodicReplayCurriculumPPO as cls
        cfg["episodic_partial"] = bool(args.partial)
        cfg["episodic_regroup_every"] = args.regroup_every
        if evolve:  # (only with --partial: main() refuses the rest)
            from rx.track_evolve_episodic import EpisodicEvolvingCurriculumPPO as cls
    t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % n, track_width=widths[i % n]), cfg,
            device="cuda")
    info, curve, tallied, top_share, rank1_share = {"steps": [], "rewards": []}, [], [], [], []
    for update, num_updates, gstep, ep in t.train_iter():
        t._log(update, num_updates, gstep, ep, info)
        if kind == "curriculum":  # the tally's running episode total (retired slots start again at 0)
            tallied.append(int(t.curriculum.tally[:, 0].sum().item()))
            ids = t.envs._st["track"].long()  # where the envs stand after this update's rollout
            top_share.append(round(torch.bincount(ids, minlength=n).max().item() / ids.numel(), 4))
            if hasattr(t, "replay"):  # the slot ranked first by the tables the last draws read
                first = int(torch.argmin(t.replay.rank).item())
                rank1_share.append(round((ids == first).float().mean().item(), 4))
        if (update + 1) % args.eval_every == 0 or update + 1 == num_updates:
            s = evaluator.run(t.agent)
            curve.append({"update": update + 1, "env_steps": gstep, "success_rate": s["success_rate"],
                          "crash_rate": s["crash_rate"]})
            print(f"[{kind}] update {update + 1}: eval success {s['success_rate']:.3f} crash {s['crash_rate']:.3f}",
                  flush=True)
    first90 = next((c["env_steps"] for c in curve if c["success_rate"] >= 0.9), None)
    out = {"kind": kind, "replay": replay_kind if kind == "curriculum" else "off", "evolve": bool(evolve),
           "evolve_edit": args.evolve_edit if evolve else None, "eval": curve, "env_steps_to_90": first90, "track_generation": t.envs.track_generation}
    if kind == "curriculum":
        from rx.curriculum import format_track_table
        tab = t.track_table()
        print(format_track_table(tab, limit=args.show))
        out["track_table"] = {k: [None if isinstance(x, float) and np.isnan(x) else x for x in v.tolist()]
                              for k, v in tab.items()}
        out["retired_per_resample"] = [len(r) for r in t.retired]
        out["episodic"] = bool(episodic)
        out["episodic_partial"] = bool(episodic and args.partial)
        out["tally_episodes_after_update"] = tallied
        out["share_of_envs_on_the_fullest_slot_after_update"] = top_share
        out["share_of_envs_on_the_rank1_slot_after_update"] = rank1_share if rank1_share else None
        out["slots_at_min_episodes"] = int((np.asarray(tab["episodes"]) >= args.min_episodes).sum())
    t.envs.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--updates", type=int, default=60)
    ap.add_argument("--tracks", type=int, default=512)
    ap.add_argument("--resample-every", type=int, default=4)
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--power", type=int, default=1)
    ap.add_argument("--mix", type=float, default=0.1)
    ap.add_argument("--prior", type=float, default=1.0)
    ap.add_argument("--score", choices=("fail", "potential"), default="fail")
    ap.add_argument("--refresh", type=float, default=0.25)
    ap.add_argument("--mastery", type=float, default=0.8)
    ap.add_argument("--min-episodes", type=int, default=4)
    ap.add_argument("--replay", choices=("off", "value_l1", "value_pos"), default="off",
                    help="draw by the rollouts' value-loss scores (rx.track_replay) instead of the finish tallies")
    ap.add_argument("--replay-power", type=int, default=4, help="rank weight (1 / rank) ** power")
    ap.add_argument("--replay-alpha", type=float, default=1.0)
    ap.add_argument("--stale-mix", type=float, default=0.1)
    ap.add_argument("--evolve", action="store_true",
                    help="fill the retired slots on the device (rx.track_evolve): fresh tracks and edited children")
    ap.add_argument("--evolve-edit", type=float, default=0.5, help="the fraction of retired slots filled by an edit")
    ap.add_argument("--episodic", action="store_true",
                    help="an env draws its next slot when its episode ends (rx.track_episodic), no global redraw")
    ap.add_argument("--partial", action="store_true",
                    help="with --episodic: retired slots are replaced in place and only their envs reset "
                         "(episodic_partial), no global reset")
    ap.add_argument("--regroup-every", type=int, default=0,
                    help="with --episodic: put the envs' positions back in slot order on the device before the "
                         "rollout of every K-th update (episodic_regroup_every; 0 = never; scheduling only)")
    ap.add_argument("--prec", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--show", type=int, default=20, help="slots of the table to print, the most failed first")
    ap.add_argument("--no-uniform", action="store_true", help="skip the uniform PPO run")
    ap.add_argument("--out", default="bench_out/curriculum_train.json")
    args = ap.parse_args()
    if args.episodic and args.evolve and not args.partial:
        sys.exit("--episodic moves envs between the slots of a fixed table, and --evolve on the global path gives a "
                 "retired slot a new point count and rebuilds that table: pass --partial as well, which evolves the "
                 "retired slots in place at their own point count (DESIGN.md §4)")
    if args.regroup_every and not args.episodic:
        sys.exit("--regroup-every regroups the lane-varying envs of the episodic trainers: pass --episodic as well")
    if args.partial and not args.episodic:
        sys.exit("--partial replaces retired slots under the episodic trainers: pass --episodic as well")
    if not torch.cuda.is_available():
        sys.exit("curriculum_train.py trains on the GPU: no device found")
    from rx.evaluate import Evaluator
    evaluator = Evaluator(backend="fused", device="cuda")
    res = {"command": "python tools/curriculum_train.py " + " ".join(sys.argv[1:]),
           "shape": {"envs": args.envs, "num_steps": args.steps, "updates": args.updates, "tracks": args.tracks,
                     "resample_every": args.resample_every},
           "protocol": "rx.evaluate.Evaluator: 40 held-out tracks x 5 runs, stochastic policy, fused backend",
           "runs": []}
    for kind in ("curriculum",) + (() if args.no_uniform else ("uniform",)):
        res["runs"].append(run(kind, args, evaluator))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # after every run: a later failure keeps what was measured
            json.dump(res, f, indent=1)
    evaluator.close()
    print("->", args.out)


if __name__ == "__main__":
    main()
