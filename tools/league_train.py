"""Self-play training in which every env races its own opponent (rx.league_train).

    python tools/league_train.py --envs 8192 --steps 128 --updates 40
    python tools/league_train.py --envs 64 --steps 32 --updates 6 --snapshot-freq 1 --pool-size 3
    python tools/league_train.py --curriculum --track-resample-every 2 --tracks 64 --envs 8192 --steps 128 --updates 12

SelfPlayPPO's loop with the opponent pool in a device bank: per env an opponent
drawn from the pool, weighted towards the snapshots the learner still loses to
(``--pfsp-power``, ``--pfsp-mix``, ``--pfsp-prior``), every finished episode
counted on the device.  The learner's head-to-head record against the pool is
printed at the end and written to ``--out`` as JSON; ``--save`` also writes a
checkpoint that tools/league.py reads.

``--curriculum`` trains rx.track_selfplay.LeagueCurriculumPPO instead: every finished
episode is also counted against its track slot, every ``--track-resample-every`` updates
the envs are redrawn over the ``--tracks`` slots towards the tracks the learner still loses
on (``--curriculum-score``), and the per-track table is printed beside the head-to-head one.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--snapshot-freq", type=int, default=15)
    ap.add_argument("--pool-size", type=int, default=5)
    ap.add_argument("--pfsp-power", type=int, default=1)
    ap.add_argument("--pfsp-mix", type=float, default=0.1)
    ap.add_argument("--pfsp-prior", type=float, default=1.0)
    ap.add_argument("--prec", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--resume", default=None, help="a checkpoint of an earlier run")
    ap.add_argument("--save", default=None, help="write a checkpoint here at the end")
    ap.add_argument("--out", default="bench_out/league_train.json")
    ap.add_argument("--curriculum", action="store_true", help="tally per track slot and resample (rx.track_selfplay)")
    ap.add_argument("--track-resample-every", type=int, default=0, metavar="K",
                    help="with --curriculum: redraw the envs over the slots every K updates (0: tally only)")
    ap.add_argument("--tracks", type=int, default=0, metavar="N",
                    help="distinct tracks in the pool, env i on track i %% N (default: one per env)")
    ap.add_argument("--curriculum-score", default="lose", choices=("fail", "potential", "lose", "contested"))
    args = ap.parse_args()
    if not args.curriculum and args.track_resample_every:
        ap.error("--track-resample-every needs --curriculum")
    from rx.configs import self_play_config
    from rx.envs import MultiRacingEnv
    from rx.league_train import LeagueSelfPlayPPO, format_head_to_head
    from rx.track import gen_tracks
    cfg = self_play_config(num_envs=args.envs, num_steps=args.steps, snapshot_freq=args.snapshot_freq,
                           pool_size=args.pool_size, seed=args.seed, shuffle="device", checkpoint=False,
                           policy_dtype=args.prec, pfsp_power=args.pfsp_power, pfsp_mix=args.pfsp_mix,
                           pfsp_prior=args.pfsp_prior)
    cfg["total_timesteps"] = args.updates * cfg["batch_size"]
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    n_tracks = args.tracks if args.tracks > 0 else args.envs
    if args.tracks > 0:  # N distinct tracks (the seeded pool below repeats after a few)
        rng = np.random.RandomState(args.seed)
        pool = gen_tracks(n_tracks, seed=None, rng=rng)
        widths = [int(rng.randint(6, 10)) for _ in range(n_tracks)]
    else:
        pool = gen_tracks(n_tracks, seed=args.seed)
        widths = [np.random.randint(6, 10) for _ in range(n_tracks)]
    cls = LeagueSelfPlayPPO
    if args.curriculum:
        from rx.track_selfplay import LeagueCurriculumPPO, format_track_table
        cls = LeagueCurriculumPPO
        cfg.update(track_resample_every=args.track_resample_every, curriculum_score=args.curriculum_score)
    t = cls(lambda i: MultiRacingEnv(2, 11, pool, i % n_tracks, widths), cfg, device="cuda")
    update = gstep = -1
    info = None
    for update, num_updates, gstep, ep, info in t.train_iter(resume_from=args.resume):
        t._log(update, num_updates, gstep, ep, info, extra=f" | Pool Size: {len(t.opponent_pool)}")
    rows = t.head_to_head()
    print(format_head_to_head(rows))
    tracks = None
    if args.curriculum:
        table = t.track_table()
        print(format_track_table(table, limit=32))
        tracks = {k: [None if isinstance(x, float) and np.isnan(x) else x for x in v.tolist()]
                  for k, v in table.items()}
        tracks["generation"], tracks["retired"] = t.envs.venv.track_generation, t.retired
    if args.save and update >= 0:
        print("checkpoint:", t.save_checkpoint(update, gstep, info, path=args.save))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"config": json.loads(json.dumps(cfg)), "updates": update + 1, "head_to_head": rows,
                   **({"tracks": tracks} if tracks is not None else {})}, f, indent=1)
    print("->", args.out)
    t.envs.close()


if __name__ == "__main__":
    main()
