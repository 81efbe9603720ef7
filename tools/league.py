"""Head-to-head league table of a self-play checkpoint's policies (rx.league).

    python tools/league.py models/checkpoint_update_100.pth
    python tools/league.py --random 4 --tracks 2 --runs 1 --max-steps 200

The checkpoint is SelfPlayPPO.save_checkpoint's file: policy 0 is the learner,
policies 1.. its opponent pool, oldest first.  ``--random P`` plays P freshly
initialised agents (seeds 1..P, output layer widened so they steer) instead.
Every ordered pair meets on ``--tracks`` x ``--runs`` episodes of the evaluation
protocol, all in one two-car device env (rx_match_steps); the table (Bradley-
Terry ratings on the Elo scale, wins, draws, finish / crash rates) is printed and
the matrices are written to ``--out`` as JSON.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))


def random_agents(P, n_sensors=11, device="cuda"):
    from rx.agent import Agent
    from rx.spaces import single_action_space, single_observation_space
    out = []
    for k in range(P):
        torch.manual_seed(k + 1)
        a = Agent(single_observation_space(n_sensors, 2), single_action_space(2)).to(device)
        with torch.no_grad():
            a.actor_mu[4].weight.mul_(40.0)  # the 0.01-gain head gives mu ~ 0 for every observation
            a.log_std.fill_(-0.5 - 0.1 * k)
        out.append(a)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", nargs="?", help="a SelfPlayPPO checkpoint (.pth)")
    ap.add_argument("--random", type=int, default=0, metavar="P", help="P seeded random agents instead of a checkpoint")
    ap.add_argument("--tracks", type=int, default=40)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--prec", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--deterministic", action="store_true", help="mean actions (zero noise)")
    ap.add_argument("--out", default="bench_out/league.json")
    args = ap.parse_args()
    if bool(args.checkpoint) == bool(args.random):
        ap.error("give a checkpoint path or --random P")
    from rx.league import League, PolicyBank
    if args.random:
        if args.random < 2:
            ap.error("--random needs at least 2 policies")
        bank = PolicyBank(random_agents(args.random), device="cuda")
        names = [f"random{k + 1}" for k in range(args.random)]
    else:
        bank = PolicyBank.from_checkpoint(args.checkpoint, device="cuda")
        names = ["learner"] + [f"pool{k}" for k in range(bank.n_policies - 1)]
        if bank.n_policies < 2:
            sys.exit("the checkpoint's opponent pool is empty: nobody to play against")
    lg = League(num_tracks=args.tracks, num_runs=args.runs, max_steps=args.max_steps, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = lg.play(bank, deterministic=args.deterministic, prec=args.prec)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.names = names
    print(res.format())
    out = res.to_json()
    out.update(tracks=args.tracks, runs=args.runs, max_steps=args.max_steps, prec=args.prec,
               deterministic=args.deterministic, wall_s=round(dt, 3), steps=int(np.max(res.record[:, :, 2])),
               source=args.checkpoint or f"--random {args.random}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"{res.seat.shape[0]} episodes, {out['steps']} steps, {dt:.2f} s -> {args.out}")
    lg.close()


if __name__ == "__main__":
    main()
