"""Time a retiring resample's replacement on a live env: host spawn against in-place evolution.

    python tools/bench_track_evolve_episodic.py [--sizes 1024 65536] [--reps 7]
                                    [--out profiles/track_evolve_episodic/bench_track_evolve_episodic.json]

One lane-varying single-agent env per size, one distinct slot per env (pools as in
tools/bench_track_replace.py), 25 % of the slots retired per round (scattered, another
set every round).  The two routes of the partial resample, from the retired slots to
a reset env:

host    what ``EpisodicReplayCurriculumPPO(episodic_partial=True)`` does:
        ``spawn_same_points`` (numpy, one ``gen_random_track`` per slot in a Python
        loop), then ``RacingVectorEnv.replace_tracks`` (the upload, a small build, the
        patch, the masked reset);
device  what ``EpisodicEvolvingCurriculumPPO`` does: ``TrackEvolver.classes``,
        ``spawn_in_place``, ``RacingVectorEnv.replace_tracks_device`` (the same small
        build, patch and masked reset), ``commit``, and the plan's download (16 bytes
        per retired slot).

Wall clock with torch.cuda.synchronize() on both sides.  One warm-up round, then --reps
rounds; in every round both routes run one after the other on the same env, so they
alternate in one session (the evolver's pool does not see what the host route put
into the env's table; neither route's work depends on what a slot holds, and every
slot keeps its point count).  The device route is also timed in parts (classes + spawn,
replace, commit + plan), each ended by a synchronise, and the class kernel alone by
device events around 20 back-to-back launches.  All runs are listed with the median
and the spread; no threshold.  It needs a HIP device and fails without one.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--edit-frac", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_evolve_episodic",
                                                  "bench_track_evolve_episodic.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rx.track import gen_tracks
    from rx.track_episodic import spawn_same_points
    from rx.track_evolve import TrackEvolver
    from rx.vector_env import RacingVectorEnv
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_evolve_episodic needs a HIP device")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    now = time.perf_counter

    def stats(xs):
        med = float(np.median(xs))
        return {"median_ms": round(1e3 * med, 4), "min_ms": round(1e3 * min(xs), 4), "max_ms": round(1e3 * max(xs), 4),
                "spread": round((max(xs) - min(xs)) / med, 4), "runs_ms": [round(1e3 * x, 4) for x in xs]}

    res = {"command": "python tools/bench_track_evolve_episodic.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "reps": a.reps,
           "protocol": "wall clock between device synchronises, 1 warm-up round then --reps rounds, the routes "
                       "alternating; the class kernel by device events around 20 launches",
           "edit_frac": a.edit_frac, "sizes": {}}
    for n in a.sizes:
        np.random.seed(5)
        pool = gen_tracks(n, seed=None)
        widths = [float(np.random.randint(6, 10)) for _ in range(n)]
        v = RacingVectorEnv(pool, widths, device=dev, autoreset="next_step", track_backend="device",
                            sched=dict(wide_n=-1, dyn_lpe=1, lane_tracks=1))
        assert v.schedule()["lane_tracks"] == 1 and len(v.tracks) == n
        v.reset_device()
        act = torch.zeros((n, 1, 2), dtype=torch.float32, device=dev)
        points = [len(c) for c in pool]
        ev = TrackEvolver.from_tracks(pool, widths, seed=1, edit_frac=a.edit_frac, device=dev)
        # an inclusive integer rank table as rx_track_learn_tables leaves it: random weights below 2^32
        cdf = torch.from_numpy(np.cumsum(np.random.RandomState(9).randint(1, 1 << 32, size=n, dtype=np.int64))).to(dev)
        runs = {k: [] for k in ("host", "host_spawn", "host_replace", "device", "device_classes_spawn",
                                "device_replace", "device_commit_plan")}
        kinds = np.zeros(2, dtype=np.int64)
        n_reset = []
        for rep in range(a.reps + 1):  # round 0 warms both routes up
            slots = np.sort(np.random.RandomState(100 + rep).choice(n, size=n // 4, replace=False)).astype(np.int64)
            v.step_device(act)
            sync()
            t0 = now()
            cps, ws = spawn_same_points(7, 2 * rep + 1, [points[k] for k in slots])
            t1 = now()
            _, mask = v.replace_tracks(slots, cps, ws)
            sync()
            t2 = now()
            v.step_device(act)
            sync()
            t3 = now()
            ev.classes(cdf)
            p = ev.spawn_in_place(slots, 2 * rep + 2)
            sync()
            t4 = now()
            _, mask_d = v.replace_tracks_device(p.slots, p.out_off, p.cp_out, p.width_out)
            sync()
            t5 = now()
            ev.commit(p)
            plan = p.plan.cpu().numpy()
            sync()
            t6 = now()
            if not bool(torch.isfinite(p.width_out).all()):
                raise SystemExit(f"bench_track_evolve_episodic: a spawned track was marked bad (round {rep})")
            if rep:
                for k, x in (("host", t2 - t0), ("host_spawn", t1 - t0), ("host_replace", t2 - t1), ("device", t6 - t3),
                             ("device_classes_spawn", t4 - t3), ("device_replace", t5 - t4),
                             ("device_commit_plan", t6 - t5)):
                    runs[k].append(x)
                kinds += np.bincount(plan[:, 0], minlength=2)
                n_reset.append((int(mask.sum().item()), int(mask_d.sum().item())))
        # the class kernel's own device time
        launches = 20
        ev.classes(cdf)
        sync()
        kernel = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                ev.classes(cdf)
            e1.record()
            sync()
            kernel.append(e0.elapsed_time(e1) / launches * 1e-3)
        per = {"slots": n, "retired": n // 4, "envs_reset_host_device": n_reset[-1],
               "control_points_up_host": int(sum(points[k] for k in slots)), "plan_bytes_down_device": 16 * (n // 4),
               "spawned_fresh": int(kinds[0]), "spawned_edits": int(kinds[1]),
               **{k: stats(x) for k, x in runs.items()}, "class_kernel": stats(kernel)}
        per["host_over_device"] = round(per["host"]["median_ms"] / per["device"]["median_ms"], 2)
        res["sizes"][str(n)] = per
        print(f"n={n}: host {per['host']['median_ms']:.3f} ms (spawn {per['host_spawn']['median_ms']:.3f}, replace "
              f"{per['host_replace']['median_ms']:.3f})  device {per['device']['median_ms']:.3f} ms (classes + spawn "
              f"{per['device_classes_spawn']['median_ms']:.3f}, replace {per['device_replace']['median_ms']:.3f}, "
              f"commit + plan {per['device_commit_plan']['median_ms']:.3f})  class kernel "
              f"{per['class_kernel']['median_ms']:.4f} ms  host/device {per['host_over_device']}", flush=True)
        v.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # after every size: a later failure keeps what was measured
            json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
