"""Time the track-table builders on distinct-track pools.

    python tools/bench_track_build.py [--sizes 4096 65536] [--reps 3] [--out profiles/track_build/mi355x.json]

Pools: np.random.seed(5); gen_tracks(N, seed=None), one track per env (the
stress pool).  Two things are recorded, each the best of --reps:

1. geometry alone
   * scipy : TrackSet.build(pool, widths) with its default workers -- the
             spawn pool of scipy splines, the only path before ABI v24 (the
             call has no smaller geometry-only part: the pool hands back
             packed rows);
   * native: rx_build_tracks_host over the flattened pool (rx.track.build_table);
   * device: rx_build_tracks -- upload of the control points, kernel span
             (device events around the launch), download of the table, each
             by itself, and their sum.
2. the whole TrackSet.build call for each backend, which adds the dedup pass
   and the per-slot Python loop the backends share.

It needs a HIP device and fails without one.  The device and native tables are
compared byte for byte at every timed size.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]


def _best(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts), ts


def _device_parts(pool, widths, factor):
    """One device build with its three parts timed apart; -> (upload s, kernel s, download s, table bytes, flat)."""
    import numpy as np
    import torch
    from rx import _lib
    L = _lib.load()
    n = len(pool)
    cp_off = np.concatenate([[0], np.cumsum([len(c) for c in pool])]).astype(np.int32)
    cp = np.ascontiguousarray(np.concatenate(pool), dtype=np.float64)
    w = np.asarray(widths, dtype=np.float64)
    wt = int(cp_off[-1]) * factor
    cuts = np.concatenate([[0], np.cumsum([2 * wt, 2 * wt, 8 * wt, 8 * n])])
    wp_off = np.zeros(n + 1, np.int32)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cp_d, w_d = torch.from_numpy(cp).cuda(), torch.from_numpy(w).cuda()
    flat_d = torch.empty(int(cuts[-1]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    parts = [flat_d[cuts[i]:cuts[i + 1]] for i in range(4)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(L.rx_build_tracks(n, factor, _lib.ptr(cp_off), _lib.ptr(cp_d), _lib.ptr(w_d), _lib.ptr(wp_off),
                                 *[_lib.ptr(x) for x in parts], _lib.stream_ptr()), "rx_build_tracks")
    e1.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    flat = flat_d.cpu().numpy()
    t3 = time.perf_counter()
    return t1 - t0, e0.elapsed_time(e1) * 1e-3, t3 - t2, flat.nbytes, flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--factor", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_build", "mi355x.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from rx.track import TrackSet, build_table, gen_tracks
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_build needs a HIP device")
    res = {"device": torch.cuda.get_device_name(0), "cpus": len(os.sched_getaffinity(0)), "reps": a.reps,
           "factor": a.factor, "sizes": {}}
    _device_parts([np.array([[0.0, 0], [8, 0], [8, 8], [0, 8]])], [1.0], a.factor)  # load the code object
    for n in a.sizes:
        np.random.seed(5)
        pool = gen_tracks(n, seed=None)
        widths = [float(np.random.randint(6, 10)) for _ in range(n)]
        r = {"n_tracks": n, "waypoints": int(sum(len(c) for c in pool)) * a.factor}
        # 1. geometry alone
        r["native_geometry_s"], _ = _best(lambda: build_table(pool, widths, a.factor, "native"), a.reps)
        dev, flat_dev = [], None
        for i in range(a.reps + 1):  # the first run at this size is the warm-up
            *times, flat_dev = _device_parts(pool, widths, a.factor)
            if i:
                dev.append(times)
        r["device_upload_s"] = min(d[0] for d in dev)
        r["device_kernel_s"] = min(d[1] for d in dev)
        r["device_download_s"] = min(d[2] for d in dev)
        r["device_geometry_s"] = min(d[0] + d[1] + d[2] for d in dev)
        r["table_bytes"] = dev[0][3]
        r["device_kernel_GBps"] = r["table_bytes"] / r["device_kernel_s"] / 1e9
        nat = build_table(pool, widths, a.factor, "native")
        flat_nat = np.concatenate([nat[k].ravel() for k in ("wp", "nrm", "seg")])
        r["device_equals_native"] = bool(flat_dev[:flat_nat.size].tobytes() == flat_nat.tobytes())
        del flat_dev, flat_nat, nat
        # 2. the whole call
        built = {}
        for backend in ("native", "device", "scipy"):
            def run(b=backend):
                built[b] = TrackSet.build(pool, widths, factor=a.factor, backend=b)
            r[f"{backend}_build_s"], r[f"{backend}_build_all_s"] = _best(run, a.reps)
        r["scipy_geometry_s"] = r["scipy_build_s"]  # the parent path has no smaller geometry-only part
        an, ad, asc = (built[b].arrays() for b in ("native", "device", "scipy"))
        r["python_tables_identical"] = all(an[k].tobytes() == ad[k].tobytes() for k in an)
        r["max_abs_waypoint_dev_vs_scipy"] = float(np.abs(an["wp"] - asc["wp"]).max())
        res["sizes"][str(n)] = r
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
