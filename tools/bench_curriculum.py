"""Track curriculum: what the per-step tally costs the rollout, and what a resample costs.

    python tools/bench_curriculum.py [--repeats 15] [--out profiles/curriculum/bench_curriculum.json]

(1) Rollout ms per update, ``rx.ppo.PPO`` on rx_rollout_steps (the parent path,
    unchanged in this tree) against ``rx.curriculum.CurriculumPPO`` on
    rx_track_rollout_steps, at 4,096 envs x 128 steps and 65,536 x 16 (bench.py's
    seed-1 pool: 7 distinct slots, so many envs per slot -- the contended case of
    the tally).  Both trainers live in one process and are timed in turn
    (interleaved: drift hits both alike): ``collect_rollout`` on the wall clock
    between two device synchronises, two warm-up rollouts each, then --repeats
    rounds.  The policy is the untrained one (no update runs between rollouts): the
    cars crash early and often, so the tally sees about as many ended episodes per
    step as it ever will.  The difference between the two is T tally launches plus
    the info rows the step writes for them; a third trainer, ``PPO`` made to write
    the info rows (``ppo_info``), splits the two.  Reported per side: every run,
    min, median, max, spread = (max - min) / median; the ratios of the medians; and
    the two parts in microseconds per step.

(2) The resample step at 1,024 and 65,536 slots (one env per slot, distinct
    tracks): rx_track_scores, rx_track_draw plus the download of the ids, and
    ``reassign_tracks`` (rx_assign in host code, reset of every env), each between
    device synchronises.

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


def summary(ms):
    med = statistics.median(ms)
    return {"runs_ms": [round(x, 3) for x in ms], "min": round(min(ms), 3), "median": round(med, 3),
            "max": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def rollout_pair(envs, T, repeats):
    import numpy as np
    import torch
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.ppo import PPO
    from rx.track import gen_tracks
    random.seed(1)
    np.random.seed(1)
    pool = gen_tracks(envs, seed=1)
    widths = [np.random.randint(6, 10) for _ in range(envs)]
    side = {}
    for name, cls in (("ppo", PPO), ("ppo_info", PPO), ("curriculum", CurriculumPPO)):
        cfg = base_config(num_envs=envs, num_steps=T, kl_target=1e9)
        random.seed(1)
        np.random.seed(1)
        torch.manual_seed(1)
        t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i, track_width=widths[i]), cfg,
                device="cuda")
        if name == "ppo_info":  # every step io of this trainer also carries the info rows
            from rx import _lib
            v = t.envs
            plain = v._make_io

            def with_info(*a, v=v, plain=plain):
                io = plain(*a)
                io.info = _lib.ptr(v.buf["info"])
                return io
            v._make_io = with_info
            v._io_cache.clear()
        bufs = list(t._buffers()) + [t.envs.buf["obs"].clone(), torch.zeros(envs, device="cuda")]
        side[name] = (t, bufs)
    ms = {k: [] for k in side}
    episodes = {k: 0 for k in side}
    for r in range(2 + repeats):
        for name, (t, bufs) in side.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.collect_rollout(*bufs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= 2:
                ms[name].append(dt)
                episodes[name] += len(out[8])
    cur = side["curriculum"][0]
    tally = cur.curriculum.tally.cpu().numpy()
    res = {"envs": envs, "num_steps": T, "slots": int(cur.curriculum.n_tracks),
           "ppo": summary(ms["ppo"]), "ppo_info": summary(ms["ppo_info"]), "curriculum": summary(ms["curriculum"]),
           "episodes_ended_per_step": {k: round(v / (repeats * T), 1) for k, v in episodes.items()},
           "tally_episodes_total": int(tally[:, 0].sum())}
    res["curriculum_over_ppo"] = round(res["curriculum"]["median"] / res["ppo"]["median"], 4)
    res["ppo_info_over_ppo"] = round(res["ppo_info"]["median"] / res["ppo"]["median"], 4)
    res["tally_us_per_step"] = round((res["curriculum"]["median"] - res["ppo_info"]["median"]) * 1e3 / T, 2)
    res["info_us_per_step"] = round((res["ppo_info"]["median"] - res["ppo"]["median"]) * 1e3 / T, 2)
    res["within_spread"] = bool(abs(res["curriculum_over_ppo"] - 1.0)
                                <= max(res["ppo"]["spread"], res["curriculum"]["spread"]))
    for t, _ in side.values():
        t.envs.close()
    return res


def resample(n, repeats):
    import numpy as np
    import torch
    from rx.curriculum import TrackCurriculum
    from rx.track import gen_tracks
    from rx.vector_env import RacingVectorEnv
    rng = np.random.RandomState(5)
    pool = gen_tracks(n, seed=None, rng=rng)
    widths = [float(rng.randint(6, 10)) for _ in range(n)]
    v = RacingVectorEnv(pool, widths, device="cuda", track_backend="device")
    v.reset_device()
    cur = TrackCurriculum(v, seed=1)
    # tallies as a run would leave them: a few dozen episodes per slot, some slots mastered
    t = np.zeros((n, 4), dtype=np.int64)
    t[:, 0] = rng.randint(1, 60, size=n)
    t[:, 1] = (rng.rand(n) ** 3 * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
    cur.tally.copy_(torch.from_numpy(t))
    sync, now = torch.cuda.synchronize, time.perf_counter
    parts = {"scores_ms": [], "draw_and_download_ms": [], "reassign_ms": [], "total_ms": []}
    for r in range(1 + repeats):
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
        if r:
            for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                parts[k].append(dt * 1e3)
    out = {"slots": n, "envs": n, "distinct_slots_drawn_last": int(len(np.unique(toe)))}
    out.update({k: summary(x) for k, x in parts.items()})
    v.close()
    del v, cur
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x128,65536x16")
    ap.add_argument("--slots", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curriculum", "bench_curriculum.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_curriculum measures on the GPU: no device found")
    res = {"command": "python tools/bench_curriculum.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "unit": "ms on the host clock between device synchronises", "rollout": [], "resample": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for shape in a.shapes.split(","):
        envs, T = (int(x) for x in shape.split("x"))
        res["rollout"].append(rollout_pair(envs, T, a.repeats))
        print(json.dumps(res["rollout"][-1]), flush=True)
        save()  # after every part: a later failure keeps what was measured
    for n in a.slots:
        res["resample"].append(resample(n, a.repeats))
        print(json.dumps(res["resample"][-1]), flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
