"""Time the replacement of some track slots on a live env through both routes.

    python tools/bench_track_replace.py [--sizes 1024 65536] [--reps 5]
                                        [--out profiles/track_replace/bench_track_replace.json]

One lane-varying single-agent env per size, one distinct slot per env (pools as in
tools/bench_track_swap.py).  Per size and per share of the slots (1 slot, 25 % of
them) the same replacement tracks (rx.track_episodic.spawn_same_points: every slot
keeps its point count) go in through

(a) the global route: DeviceTrackTable.build of the WHOLE pool, then
    RacingVectorEnv.set_tracks (rx_upload_tracks_device: every culling table
    rebuilt; rx_assign in host code; every env reset);
(b) the partial route: RacingVectorEnv.replace_tracks (a small build, one
    k_patch_slots launch over the handle's buffers and one over the resident
    table, a masked reset), also with its parts apart: small build =
    DeviceTrackTable.replacement and a wait; patch = rx_replace_tracks_device
    (which waits itself) plus the resident table's rx_patch_tracks and a wait;
    reset = the mask, the masked rx_reset and a wait.

Wall clock with torch.cuda.synchronize() on both sides, the control points drawn
before the clock starts.  One warm-up of each route, then --reps rounds; in every
round (a), (b) and (b)-in-parts run one after the other, so the routes alternate in
one session.  All runs are listed; the median and the spread (min, max) are
reported, with the envs reset against N and the table bytes the patch replaces.
It needs a HIP device and fails without one.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_replace", "bench_track_replace.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rx import _lib
    from rx.track import gen_tracks
    from rx.track_device import DeviceTrackTable
    from rx.track_episodic import spawn_same_points
    from rx.vector_env import RacingVectorEnv
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_replace needs a HIP device")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    now = time.perf_counter

    def stats(xs):
        return {"median_ms": round(1e3 * float(np.median(xs)), 4), "min_ms": round(1e3 * min(xs), 4),
                "max_ms": round(1e3 * max(xs), 4), "runs_ms": [round(1e3 * x, 4) for x in xs]}

    res = {"device": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "reps": a.reps,
           "schedule": "lane_tracks", "sizes": {}}
    for n in a.sizes:
        np.random.seed(5)
        pool = gen_tracks(n, seed=None)
        widths = [float(np.random.randint(6, 10)) for _ in range(n)]
        v = RacingVectorEnv(pool, widths, device=dev, autoreset="next_step", track_backend="device",
                            sched=dict(wide_n=-1, dyn_lpe=1, lane_tracks=1))
        assert v.schedule()["lane_tracks"] == 1 and len(v.tracks) == n
        v.reset_device()
        act = torch.zeros((n, 1, 2), dtype=torch.float32, device=dev)
        cps_all, ws_all = list(pool), list(widths)
        toe = np.arange(n, dtype=np.int32)
        res["sizes"][str(n)] = per_size = {}
        for label, m in (("1_slot", 1), ("25_percent", n // 4)):
            slots = np.sort(np.random.RandomState(n + m).choice(n, size=m, replace=False)).astype(np.int64)
            runs = {k: [] for k in ("global", "global_build", "global_set_tracks", "partial", "parts_build",
                                    "parts_patch", "parts_reset")}
            n_reset = None
            for rep in range(a.reps + 1):  # round 0 warms every route up
                draw = lambda g: spawn_same_points(7, g, [len(cps_all[k]) for k in slots])  # noqa: E731
                # (a) the global route
                cps, ws = draw(3 * rep)
                for k, c, w in zip(slots, cps, ws):
                    cps_all[k], ws_all[k] = c, float(w)
                v.step_device(act)
                sync()
                t0 = now()
                table = DeviceTrackTable.build(cps_all, ws_all, device=dev)
                sync()
                t1 = now()
                v.set_tracks(table, toe)
                sync()
                t2 = now()
                # (b) the partial route, one call
                cps, ws = draw(3 * rep + 1)
                for k, c, w in zip(slots, cps, ws):
                    cps_all[k], ws_all[k] = c, float(w)
                v.step_device(act)
                sync()
                t3 = now()
                _, mask = v.replace_tracks(slots, cps, ws)
                sync()
                t4 = now()
                n_reset = int(mask.sum().item())
                # (b) again with its parts apart
                cps, ws = draw(3 * rep + 2)
                for k, c, w in zip(slots, cps, ws):
                    cps_all[k], ws_all[k] = c, float(w)
                v.step_device(act)
                sync()
                t5 = now()
                source = v._table.replacement(slots, cps, ws)
                sync()
                t6 = now()
                p, keep = v._table.patch(source)
                _lib.check(v.L.rx_replace_tracks_device(v._h, ctypes.byref(p), _lib.stream_ptr()),
                           "rx_replace_tracks_device")
                v._table.apply(source)
                sync()
                t7 = now()
                flag = torch.zeros(n, dtype=torch.uint8, device=dev)
                flag[torch.from_numpy(slots).to(dev)] = 1
                v.reset_device(flag[v._st["track"].long()])
                sync()
                t8 = now()
                if rep:
                    for k, x in (("global", t2 - t0), ("global_build", t1 - t0), ("global_set_tracks", t2 - t1),
                                 ("partial", t4 - t3), ("parts_build", t6 - t5), ("parts_patch", t7 - t6),
                                 ("parts_reset", t8 - t7)):
                        runs[k].append(x)
            w_rows = int(sum(v._table.wp_off[k + 1] - v._table.wp_off[k] for k in slots))
            per_size[label] = {"slots_replaced": int(m), "envs_reset_partial": n_reset, "envs_reset_global": n,
                               "table_bytes_replaced": w_rows * 12 * 8 + 64 * int(m),
                               "table_bytes_pool": int(v._table.wp_off[-1]) * 12 * 8 + 64 * n,
                               **{k: stats(x) for k, x in runs.items()}}
            g, p_ = per_size[label]["global"], per_size[label]["partial"]
            print(f"n={n} {label}: global {g['median_ms']:.3f} ms [{g['min_ms']:.3f}, {g['max_ms']:.3f}]  partial "
                  f"{p_['median_ms']:.3f} ms [{p_['min_ms']:.3f}, {p_['max_ms']:.3f}]  (build "
                  f"{per_size[label]['parts_build']['median_ms']:.3f}, patch "
                  f"{per_size[label]['parts_patch']['median_ms']:.3f}, reset "
                  f"{per_size[label]['parts_reset']['median_ms']:.3f}); envs reset {n_reset} of {n}", flush=True)
        v.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
