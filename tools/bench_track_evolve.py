"""Track evolution: what filling the retired slots costs, on the host and on the device.

    python tools/bench_track_evolve.py [--repeats 9] [--out profiles/track_evolve/bench_track_evolve.json]

One resample's worth of new tracks at 1,024 and 65,536 slots with a quarter of them
retired (scattered slots), from the retired slots to a built ``DeviceTrackTable``:

host    what ``CurriculumPPO`` does: ``gen_tracks(seed=None, rng=...)`` and one
        ``randint(6, 10)`` width per retired slot in a Python loop, the host list of
        control points updated, then ``DeviceTrackTable.build`` (every slot's control
        points concatenated and uploaded, one rx_build_tracks launch);
device  what ``EvolvingCurriculumPPO`` does: ``TrackEvolver.spawn``, i.e.
        rx_track_evolve_plan, the plan's download, the new offsets, rx_track_evolve
        and ``DeviceTrackTable.build_from_device`` (the same rx_build_tracks launch).

Each leg runs between two device synchronises on the wall clock, two warm-up rounds,
then --repeats rounds, interleaved (drift hits both alike); every round replaces
another generation's slots of the pool the round before left.  Reported per leg:
every run, min, median, max, spread = (max - min) / median; and the ratio of the
medians.  No threshold: nobody has measured either leg before.

It needs a HIP device and fails without one.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]


def summary(ms):
    med = statistics.median(ms)
    return {"runs_ms": [round(x, 3) for x in ms], "min": round(min(ms), 3), "median": round(med, 3),
            "max": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def resample(n, repeats, edit_frac):
    import numpy as np
    import torch
    from rx.track import gen_tracks
    from rx.track_device import DeviceTrackTable
    from rx.track_evolve import TrackEvolver
    rng = np.random.RandomState(5)
    cps = gen_tracks(n, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(n)]
    host_cps, host_widths = list(cps), list(widths)
    ev = TrackEvolver.from_tracks(cps, widths, seed=1, edit_frac=edit_frac)
    # an inclusive integer rank table as rx_track_learn_tables leaves it: random weights below 2^32
    cdf = torch.from_numpy(np.cumsum(rng.randint(1, 1 << 32, size=n, dtype=np.int64))).cuda()
    ms = {"host": [], "device": []}
    kinds = np.zeros(2, dtype=np.int64)
    for r in range(2 + repeats):
        g = r + 1
        slots = np.sort(np.random.RandomState(100 + r).choice(n, size=n // 4, replace=False))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        draw = np.random.RandomState(7919 * g)
        new_cps = gen_tracks(len(slots), seed=None, rng=draw)
        new_widths = [int(draw.randint(6, 10)) for _ in range(len(slots))]
        for k, c, w in zip(slots, new_cps, new_widths):
            host_cps[k], host_widths[k] = c, w
        table = DeviceTrackTable.build(host_cps, host_widths, device="cuda")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        table_d, plan = ev.spawn(slots, g, cdf)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if not bool(torch.isfinite(table_d.meta).all()) or not bool(torch.isfinite(table.meta).all()):
            raise SystemExit(f"bench_track_evolve: a built table carries a bad track (round {r})")
        if r >= 2:
            ms["host"].append((t1 - t0) * 1e3)
            ms["device"].append((t2 - t1) * 1e3)
            kinds += np.bincount(plan[:, 0], minlength=2)
    res = {"slots": n, "retired": n // 4, "edit_frac": edit_frac, "host": summary(ms["host"]),
           "device": summary(ms["device"]), "spawned_fresh": int(kinds[0]), "spawned_edits": int(kinds[1]),
           "plan_bytes_down": 16 * (n // 4), "control_points_at_the_end": int(ev.cp_off_host[-1])}
    res["host_over_device"] = round(res["host"]["median"] / res["device"]["median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--slots", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--edit-frac", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_evolve", "bench_track_evolve.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_evolve measures on the GPU: no device found")
    res = {"command": "python tools/bench_track_evolve.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0),
           "protocol": "wall clock between device synchronises, 2 warm-up rounds then --repeats rounds, interleaved",
           "resample": []}
    for n in args.slots:
        res["resample"].append(resample(n, args.repeats, args.edit_frac))
        print(json.dumps(res["resample"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # after every size: a later failure keeps what was measured
            json.dump(res, f, indent=1)
    print("->", args.out)


if __name__ == "__main__":
    main()
