"""Lane-varying track slots for two-car envs (rx_set_lane_cars): the grouped schedule against the
lane-varying one, in one session on one build.

    python tools/bench_lane_cars.py [--pools 7,64,512,2048,8192] [--out profiles/lane_cars/bench.json]
    python tools/bench_lane_cars.py --build-minw 5 6 7      (no GPU: builds the A/B libraries)
    python tools/bench_lane_cars.py --minw 5 6 7            (one fresh process per library, 8,192-slot pool)

8,192 two-car envs (BASELINE.json configs[3]'s size) over pools of 7 slots (the seed-1 pool), 64,
512, 2,048 and 8,192 distinct slots (env i on slot i % slots), the tables built by the device
backend.  Per pool two envs on one TrackSet with one seed, one per schedule; each steps a window of
--window = 20 steps (fixed U(-1, 1)^2 actions per car, the same for both) captured in a HIP graph.
After 5 warm-up windows the two graphs are replayed in turn, --repeats = 7 times each, between
device events: ms per step = window time / 20; median, min and max per side.  Both envs have then
taken the same steps, and their last outputs (obs, reward, done) and state must be equal bit for
bit ("outputs_equal"): a schedule that computes something else is no schedule.  "auto" is what
rx_set_lane_cars(h, 0) resolves on that pool; the rule is held to the measurement: wherever it
switches the schedule on, lane-varying ms/step must be at or below grouped's ("auto_rule_holds").

--minw: RX_STEP2_MINW_2LV (k_step2<2, 1, 1, true>'s waves per SIMD) A/B.  --build-minw compiles
rx/lib/ab/librx_minw<K>.so with -DRX_STEP2_MINW_2LV=<K>; --minw runs this tool once per library in a
fresh process (RX_LIB_PATH) on the largest pool and gathers the lane-varying medians.

Kernel times: run the tool under ``rocprofv3 --kernel-trace --stats -- python tools/bench_lane_cars.py
--pools 8192 --repeats 2 --out <dir>/prof_run.json`` (a run of its own: the trace slows the windows).
It needs a HIP device and fails without one.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]
AB_DIR = os.path.join(ROOT, "self-play-racing_amd", "rx", "lib", "ab")


def ab_lib(k):
    return os.path.join(AB_DIR, f"librx_minw{k}.so")


def summary(ms):
    return {"runs": [round(x, 5) for x in ms], "median": round(statistics.median(ms), 5), "min": round(min(ms), 5),
            "max": round(max(ms), 5)}


def pool_of(envs, slots):
    """(control points, widths) per env: 7 = the reference's seed-1 pool, else `slots` distinct tracks."""
    import numpy as np
    from rx.track import gen_tracks
    if slots == 7:
        random.seed(1)
        np.random.seed(1)
        pool = gen_tracks(num_tracks=envs, seed=1)
        return pool, [int(np.random.randint(6, 10)) for _ in range(envs)]
    rng = np.random.RandomState(slots)
    pool = gen_tracks(slots, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(slots)]
    return [pool[i % slots] for i in range(envs)], [widths[i % slots] for i in range(envs)]


def one_pool(envs, slots, window, warmup, repeats):
    import numpy as np
    import torch
    from rx import _lib
    from rx.track import TrackSet
    from rx.vector_env import RacingVectorEnv
    cps, widths = pool_of(envs, slots)
    ts = TrackSet.build(cps, widths, backend="device", device=torch.device("cuda:0"))
    g = torch.Generator(device="cuda").manual_seed(slots)
    acts = torch.rand((window, envs, 2, 2), device="cuda", generator=g) * 2 - 1
    side = {}
    for name, mode in (("grouped", -1), ("lane_varying", 1)):
        v = RacingVectorEnv(cps, widths, n_agents=2, device="cuda", seed=9, track_set=ts, lane_cars=mode)
        v.reset_device()

        def body(v=v):
            for t in range(window):
                v.step_device(acts[t])
        body()  # eager once: every lazy allocation happens outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            body()
        side[name] = (v, graph)
    for _ in range(warmup):
        for v, graph in side.values():
            graph.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in side}
    for _ in range(repeats):
        for name, (v, graph) in side.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / window)
    (va, _), (vb, _) = side["grouped"], side["lane_varying"]
    va._launched()
    vb._launched()
    sa, sb = va.get_state(), vb.get_state()
    equal = all(torch.equal(va.buf[k], vb.buf[k]) for k in ("obs", "reward", "done_f32")) and \
        all(np.array_equal(sa[k], sb[k]) for k in sa)
    plan = _lib.assign_plan(va._cfg, ts.arrays()["wp_off"], va.track_of_env, lane_cars=0)
    res = {"envs": envs, "slots": int(len(np.unique(va.track_of_env))), "window": window,
           "dyn_waves": {k: v.schedule()["dyn_waves"] for k, (v, _) in side.items()},
           "ray_waves": {k: v.schedule()["ray_waves"] for k, (v, _) in side.items()},
           "unit": "ms per step, device events around a captured window",
           "grouped": summary(ms["grouped"]), "lane_varying": summary(ms["lane_varying"]),
           "outputs_equal": bool(equal), "auto": int(plan["schedule"]["lane_tracks"])}
    res["lane_varying_over_grouped"] = round(res["lane_varying"]["median"] / res["grouped"]["median"], 4)
    res["m_env_steps_per_s"] = {k: round(envs / res[k]["median"] / 1e3, 1) for k in ("grouped", "lane_varying")}
    for v, graph in side.values():
        del graph
        v.close()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--pools", default="7,64,512,2048,8192")
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane_cars", "bench.json"))
    ap.add_argument("--build-minw", type=int, nargs="+", metavar="K")
    ap.add_argument("--minw", type=int, nargs="+", metavar="K")
    a = ap.parse_args()

    def save(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if a.build_minw:
        from rx import _build
        os.makedirs(AB_DIR, exist_ok=True)
        for k in a.build_minw:
            print(_build.build(out=ab_lib(k), defines=[f"RX_STEP2_MINW_2LV={k}"], verbose=False), flush=True)
        return
    if a.minw:  # a fresh process per library: librx is loaded once per process
        slots = max(int(s) for s in a.pools.split(","))
        res = {"command": "python tools/bench_lane_cars.py " + " ".join(sys.argv[1:]), "slots": slots, "builds": {}}
        for k in a.minw:
            if not os.path.exists(ab_lib(k)):
                raise SystemExit(f"{ab_lib(k)} is missing: python tools/bench_lane_cars.py --build-minw {k}")
            part = os.path.splitext(a.out)[0] + f"_minw{k}.json"
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--envs", str(a.envs), "--pools", str(slots),
                                   "--window", str(a.window), "--warmup", str(a.warmup), "--repeats", str(a.repeats),
                                   "--out", part], env=dict(os.environ, RX_LIB_PATH=ab_lib(k)))
            with open(part) as f:
                r = json.load(f)["pools"][0]
            res["builds"][f"RX_STEP2_MINW_2LV={k}"] = {"lane_varying": r["lane_varying"], "grouped": r["grouped"],
                                                      "outputs_equal": r["outputs_equal"]}
            save(res)
        res["fastest"] = min(res["builds"], key=lambda k: res["builds"][k]["lane_varying"]["median"])
        save(res)
        print(json.dumps(res))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lane_cars measures on the GPU: no device found")
    res = {"command": "python tools/bench_lane_cars.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(os.environ.get("RX_LIB_PATH") or os.path.join(ROOT, "self-play-racing_amd", "rx",
                                                                                     "lib", "librx.so"),
                                      os.path.join(ROOT, "self-play-racing_amd")), "pools": []}
    for slots in (int(s) for s in a.pools.split(",")):
        r = one_pool(a.envs, slots, a.window, a.warmup, a.repeats)
        res["pools"].append(r)
        print(json.dumps(r), flush=True)
        save(res)  # after every pool: a later failure keeps what was measured
    on = [r for r in res["pools"] if r["auto"]]
    res["auto_rule_holds"] = all(r["lane_varying"]["median"] <= r["grouped"]["median"] for r in on)
    res["outputs_equal"] = all(r["outputs_equal"] for r in res["pools"])
    save(res)
    print("wrote", a.out)
    if not res["outputs_equal"]:
        raise SystemExit("the two schedules' outputs differ")


if __name__ == "__main__":
    main()
