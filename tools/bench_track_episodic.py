"""Episodic track draws: what the draw costs the rollout, and the redraw it removes.

    python tools/bench_track_episodic.py [--repeats 15] [--out profiles/track_episodic/bench_track_episodic.json]

(1) Rollout ms per update on lane-varying envs (``sched=dict(lane_tracks=1)``), three
    trainers in one process timed in turn (tools/bench_curriculum.py's protocol:
    ``collect_rollout`` on the wall clock between two device synchronises, two
    warm-up rollouts each, then --repeats interleaved rounds, untrained policy):
    ``rx.ppo.PPO`` on rx_rollout_steps, ``rx.curriculum.CurriculumPPO`` on
    rx_track_rollout_steps (the parent's tally) and
    ``rx.track_episodic.EpisodicCurriculumPPO`` on rx_track_episodic_rollout_steps,
    at 4,096 envs x 128 steps on 512 slots and 65,536 x 16 on 4,096 slots.  The
    episodic kernel replaces the tally one for one, so episodic / curriculum near 1
    is what the design predicts; ``within_spread`` says whether the ratio of the
    medians lies inside the larger of the two sides' own (max - min) / median.

(2) The redraw a pool-level resample pays and the episodic trainer does not:
    rx_track_draw plus the download of the ids, and ``reassign_tracks`` (rx_assign
    in host code, reset of every env), against the episodic resample with nothing
    retired (rx_track_scores alone), on the same two shapes.

(3) ``--trace curriculum|episodic``: nothing is timed; that one trainer collects
    2 + 8 rollouts at the first of --shapes and the process ends -- the program of a
    ``rocprofv3 --kernel-trace --stats`` run of its own, which says where the time goes
    per kernel (profiles/track_episodic/kernel_stats_*.csv).

It needs a HIP device and fails without one.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]

LANE = dict(lane_tracks=1)


def summary(ms):
    med = statistics.median(ms)
    return {"runs_ms": [round(x, 3) for x in ms], "min": round(min(ms), 3), "median": round(med, 3),
            "max": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def trainers(envs, T, slots, only=None):
    """-> {name: (trainer, rollout buffers)} on one pool of ``slots`` tracks, every env lane-varying."""
    import numpy as np
    import torch
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.ppo import PPO, build_vector_env
    from rx.track import gen_tracks
    from rx.track_episodic import EpisodicCurriculumPPO
    rng = np.random.RandomState(5)
    pool = gen_tracks(slots, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(slots)]

    def lane_varying(cls):
        class Lane(cls):
            def _make_envs(self, env_fn):
                c = self.config
                return build_vector_env(env_fn, c["num_envs"], c["seed"], self.device,
                                        track_backend=c.get("track_backend", "scipy"), sched=LANE)
        Lane.__name__ = cls.__name__
        return Lane

    side = {}
    for name, cls in (("ppo", lane_varying(PPO)), ("curriculum", lane_varying(CurriculumPPO)),
                      ("episodic", EpisodicCurriculumPPO)):
        if only not in (None, name):
            continue
        cfg = base_config(num_envs=envs, num_steps=T, kl_target=1e9, track_backend="device", curriculum_refresh=0.0)
        random.seed(1)
        np.random.seed(1)
        torch.manual_seed(1)
        t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % slots,
                                    track_width=widths[i % slots]), cfg, device="cuda")
        assert t.envs.schedule()["lane_tracks"] == 1
        bufs = list(t._buffers()) + [t.envs.buf["obs"].clone(), torch.zeros(envs, device="cuda")]
        side[name] = (t, bufs)
    return side


def shape(envs, T, slots, repeats):
    import torch
    side = trainers(envs, T, slots)
    sync, now = torch.cuda.synchronize, time.perf_counter
    ms = {k: [] for k in side}
    episodes = {k: 0 for k in side}
    for r in range(2 + repeats):
        for name, (t, bufs) in side.items():
            sync()
            t0 = now()
            out = t.collect_rollout(*bufs)
            sync()
            if r >= 2:
                ms[name].append((now() - t0) * 1e3)
                episodes[name] += len(out[8])
    res = {"envs": envs, "num_steps": T, "slots": slots, **{k: summary(v) for k, v in ms.items()},
           "episodes_ended_per_step": {k: round(v / (repeats * T), 1) for k, v in episodes.items()}}
    res["tally_episodes_total"] = {k: int(side[k][0].curriculum.tally[:, 0].sum().item())
                                   for k in ("curriculum", "episodic")}
    res["episodic_over_curriculum"] = round(res["episodic"]["median"] / res["curriculum"]["median"], 4)
    res["curriculum_over_ppo"] = round(res["curriculum"]["median"] / res["ppo"]["median"], 4)
    res["episodic_minus_curriculum_us_per_step"] = round(
        (res["episodic"]["median"] - res["curriculum"]["median"]) * 1e3 / T, 2)
    res["within_spread"] = bool(abs(res["episodic_over_curriculum"] - 1.0)
                                <= max(res["curriculum"]["spread"], res["episodic"]["spread"]))
    # (2) the redraw: the pool-level trainer's draw + download + reassign against the episodic scores-only resample
    cur_t, epi_t = side["curriculum"][0], side["episodic"][0]
    parts = {"scores_ms": [], "draw_and_download_ms": [], "reassign_ms": [], "episodic_resample_ms": []}
    for r in range(1 + repeats):
        cur, v = cur_t.curriculum, cur_t.envs
        sync()
        t0 = now()
        cur.scores()
        sync()
        t1 = now()
        toe = cur.draw(r + 1).cpu().numpy()
        t2 = now()
        v.reassign_tracks(toe)
        sync()
        t3 = now()
        epi_t.resample_tracks()
        sync()
        t4 = now()
        if r:
            for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                parts[k].append(dt * 1e3)
    res["resample"] = {k: summary(x) for k, x in parts.items()}
    res["redraw_ms_removed_per_resample"] = round(res["resample"]["draw_and_download_ms"]["median"]
                                                  + res["resample"]["reassign_ms"]["median"], 3)
    assert epi_t.envs.track_generation == 0, "the episodic resample reset the envs"
    for t, _ in side.values():
        t.envs.close()
    del side
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x128x512,65536x16x4096", help="envs x steps x slots, comma-separated")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_episodic", "bench_track_episodic.json"))
    ap.add_argument("--trace", choices=("curriculum", "episodic"), default=None,
                    help="collect 2 + 8 rollouts with this trainer at the first shape and exit (for a kernel trace)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_episodic measures on the GPU: no device found")
    if a.trace:
        envs, T, slots = (int(x) for x in a.shapes.split(",")[0].split("x"))
        t, bufs = trainers(envs, T, slots, only=a.trace)[a.trace]
        for _ in range(10):
            t.collect_rollout(*bufs)
        torch.cuda.synchronize()
        t.envs.close()
        return
    res = {"command": "python tools/bench_track_episodic.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "unit": "ms on the host clock between device synchronises", "shapes": []}
    for s in a.shapes.split(","):
        envs, T, slots = (int(x) for x in s.split("x"))
        res["shapes"].append(shape(envs, T, slots, a.repeats))
        print(json.dumps(res["shapes"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # after every shape: a later failure keeps what was measured
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
