"""Evaluation wall-clock: rx.evaluate.Evaluator's eager loop against the fused
backend (rx_eval_steps) on the same agent in one process.

Trains the reference single-agent config (16 envs x 2,048 steps, seed 1, as
tools/time_to_success.py does) for ``--updates`` updates so that episodes last,
then times the evaluate.py protocol (40 tracks x 5 runs, <= 2,000 steps,
stochastic policy) with both backends: one warm-up run each, then ``--runs``
runs each, interleaved, torch.cuda.synchronize() around every run.  Prints one
JSON line: both medians, their ratio and the steps each run executed.

    python tools/bench_eval.py --out profiles/eval_fused/bench_eval.json

The two backends draw different noise, so their runs differ in length; the
steps executed are reported beside the times and per-step times are derived
from them.
"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))


def train(updates, seed=1):
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.ppo import PPO
    from rx.track import gen_tracks
    config = base_config(num_envs=16, num_steps=2048, seed=seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    pool = gen_tracks(num_tracks=16, seed=seed)
    widths = [np.random.randint(6, 10) for _ in range(16)]
    trainer = PPO(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i, track_width=widths[i]), config,
                  device="cuda")
    with contextlib.redirect_stdout(io.StringIO()):
        for update, _, _, _ in trainer.train_iter():
            if update + 1 >= updates:
                break
    torch.cuda.synchronize()
    return trainer


def timed(ev, agent):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.run(agent)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the loop runs until every episode has ended, checked every 50 steps
    steps = min(ev.max_steps, -(-max(e["steps"] for e in res["all_episodes"]) // 50) * 50)
    return dt, steps, res["success_rate"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=8, help="PPO updates before the evaluations")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rx.evaluate import Evaluator
    trainer = train(args.updates)
    evs = {b: Evaluator(device=trainer.device, backend=b) for b in ("eager", "fused")}
    rows = {b: [] for b in evs}
    torch.manual_seed(1234)
    for b, ev in evs.items():  # warm-up: first-use allocations, kernel loads
        timed(ev, trainer.agent)
    for _ in range(args.runs):
        for b, ev in evs.items():
            rows[b].append(timed(ev, trainer.agent))
    med = {b: statistics.median(r[0] for r in rows[b]) for b in rows}
    per_step_us = {b: statistics.median(r[0] / r[1] for r in rows[b]) * 1e6 for b in rows}
    out = {"metric": "evaluate.py protocol wall-clock, 200 episodes (s)", "updates_trained": args.updates,
           "runs": args.runs, "eager_median_s": round(med["eager"], 4), "fused_median_s": round(med["fused"], 4),
           "ratio_eager_over_fused": round(med["eager"] / med["fused"], 3),
           "eager_us_per_step": round(per_step_us["eager"], 1), "fused_us_per_step": round(per_step_us["fused"], 1),
           "eager_runs_s": [round(r[0], 4) for r in rows["eager"]],
           "fused_runs_s": [round(r[0], 4) for r in rows["fused"]],
           "eager_steps": [r[1] for r in rows["eager"]], "fused_steps": [r[1] for r in rows["fused"]],
           "eager_success_rate": [round(r[2], 3) for r in rows["eager"]],
           "fused_success_rate": [round(r[2], 3) for r in rows["fused"]],
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for ev in evs.values():
        ev.close()
    trainer.envs.close()


if __name__ == "__main__":
    main()
