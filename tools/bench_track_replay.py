"""Replay scores of the track curriculum: what the advantage tally, the rank and the
tables cost, and what they cost an update.

    python tools/bench_track_replay.py [--repeats 12] [--out profiles/track_replay/bench_track_replay.json]

(1) Device time of rx_track_learn_tally at 4,096 envs x 128 steps and 65,536 x 16,
    with 512 slots and with as many slots as envs (env i on slot i % slots), against
    a torch restatement of the same reduction (the quantised int64 magnitudes and a
    column of ones, ``index_add_`` by slot; the slot index of every value is built
    outside the timed window).  Device events around --launches back-to-back calls,
    --repeats windows after a warm-up window; the two sides alternate.  The sums of
    the two sides are compared once, bit for bit.

(2) Device time of rx_track_learn_tables (k_track_rank + k_track_learn_tables) at
    1,024 and 65,536 slots against torch: a stable descending ``argsort`` of the
    keys, the scatter of the ranks, the two weights and two ``cumsum``.  The ranks
    of the two sides are compared once.

(3) ms per update of ``rx.track_replay.ReplayCurriculumPPO`` against
    ``rx.curriculum.CurriculumPPO`` (the parent path: its rollout, GAE and update
    are untouched by the replay scores), same config, one process, the two
    ``train_iter`` generators advanced in turn, each update on the host clock between
    two device synchronises.  Updates that begin with a resample are summarised
    apart.  The difference is one tally and one fold launch per update and, at a
    resample, the rank, tables and draw launches in place of scores and draw.

No threshold: the file records both sides and their ratio.  It needs a HIP device
and fails without one.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]


def summary(xs, digits=3):
    med = statistics.median(xs)
    return {"runs": [round(x, digits) for x in xs], "min": round(min(xs), digits), "median": round(med, digits),
            "max": round(max(xs), digits), "spread": round((max(xs) - min(xs)) / med, 4)}


def device_us(sides, launches, repeats):
    """{name: fn} -> {name: summary of microseconds per call}: device events around `launches` calls,
    one warm-up window, then `repeats` windows per side in turn."""
    import torch
    us = {k: [] for k in sides}
    for r in range(1 + repeats):
        for name, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                us[name].append(a.elapsed_time(b) * 1e3 / launches)
    return {k: summary(v, 2) for k, v in us.items()}


def tally(envs, T, slots, launches, repeats):
    import torch
    from rx import _lib
    L = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(envs + slots)
    adv = torch.randn((T, envs), device="cuda", generator=g) * 2.0
    track = (torch.arange(envs, device="cuda") % slots).to(torch.int32)
    learn = torch.zeros((slots, 2), dtype=torch.int64, device="cuda")
    lt = _lib.RxTrackLearnIO(slots, 0, _lib.ptr(track), _lib.ptr(learn), None, None, None, None, None, None, 0)
    stream = _lib.stream_ptr()

    def kernel():
        _lib.check(L.rx_track_learn_tally(ctypes.byref(lt), T, envs, _lib.ptr(adv), stream), "rx_track_learn_tally")

    idx = track.long().expand(T, envs).reshape(-1).contiguous()
    ones = torch.ones_like(idx)
    mag, samples = torch.zeros(slots, dtype=torch.int64, device="cuda"), torch.zeros(slots, dtype=torch.int64,
                                                                                     device="cuda")

    def restated():
        q = (adv.abs().clamp(max=1048576.0).double() * 1048576.0).long().reshape(-1)
        mag.index_add_(0, idx, q)
        samples.index_add_(0, idx, ones)

    kernel()
    restated()
    same = bool(torch.equal(learn, torch.stack([samples, mag], 1)))
    res = {"envs": envs, "num_steps": T, "slots": slots, "values": envs * T, "launches_per_window": launches,
           "sums_equal_bit_for_bit": same}
    res.update(device_us({"rx_track_learn_tally_us": kernel, "torch_index_add_us": restated}, launches, repeats))
    res["torch_over_kernel"] = round(res["torch_index_add_us"]["median"] / res["rx_track_learn_tally_us"]["median"], 2)
    res["kernel_GB_per_s"] = round(envs * T * 4 / res["rx_track_learn_tally_us"]["median"] / 1e3, 1)
    return res


def tables(slots, launches, repeats):
    import numpy as np
    import torch
    from rx import _lib
    L = _lib.load()
    rs = np.random.RandomState(slots)
    # scores as a run leaves them: many distinct values, some ties, a tenth of the slots never scored
    score = torch.from_numpy(np.where(rs.rand(slots) < 0.2, 0.25, rs.rand(slots))).cuda()
    seen = torch.from_numpy(np.where(rs.rand(slots) < 0.1, -1, rs.randint(0, 40, size=slots)).astype(np.int32)).cuda()
    rank = torch.zeros(slots, dtype=torch.int32, device="cuda")
    cs, ct = torch.zeros(slots, dtype=torch.int64, device="cuda"), torch.zeros(slots, dtype=torch.int64, device="cuda")
    lt = _lib.RxTrackLearnIO(slots, 0, None, None, _lib.ptr(score), _lib.ptr(seen), _lib.ptr(rank), _lib.ptr(cs),
                             _lib.ptr(ct), None, 0)
    stream = _lib.stream_ptr()

    def kernel():
        _lib.check(L.rx_track_learn_tables(ctypes.byref(lt), 4, 40, stream), "rx_track_learn_tables")

    inf = torch.full_like(score, float("inf"))
    ar = torch.arange(1, slots + 1, device="cuda")
    out = {}

    def restated():
        key = torch.where(seen < 0, inf, score)
        order = torch.argsort(key, descending=True, stable=True)
        r = torch.empty_like(ar)
        r[order] = ar
        h = 1.0 / r.double()
        w = (h * h * h * h * 4294967296.0).long()
        s = torch.where(seen < 0, 0, 40 - seen.long())
        out["rank"], out["cdf_score"], out["cdf_stale"] = r, torch.cumsum(w, 0), torch.cumsum(s, 0)

    kernel()
    restated()
    res = {"slots": slots, "power": 4, "launches_per_window": launches,
           "ranks_equal": bool(torch.equal(rank.long(), out["rank"])),
           "tables_equal": bool(torch.equal(cs, out["cdf_score"]) and torch.equal(ct, out["cdf_stale"])),
           "rank_comparisons": slots * slots}
    res.update(device_us({"rx_track_learn_tables_us": kernel, "torch_argsort_cumsum_us": restated}, launches, repeats))
    res["torch_over_kernel"] = round(res["torch_argsort_cumsum_us"]["median"] /
                                     res["rx_track_learn_tables_us"]["median"], 2)
    return res


def update_pair(envs, T, tracks, repeats, resample_every):
    import numpy as np
    import torch
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.track import gen_tracks
    from rx.track_replay import ReplayCurriculumPPO
    rng = np.random.RandomState(1)
    pool = gen_tracks(tracks, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(tracks)]
    warm = resample_every  # up to the first resample: every path has run once
    side = {}
    for name, cls in (("curriculum", CurriculumPPO), ("replay", ReplayCurriculumPPO)):
        cfg = base_config(num_envs=envs, num_steps=T, seed=1, shuffle="device", kl_target=1e9,
                          track_resample_every=resample_every)
        cfg["total_timesteps"] = (warm + 1 + repeats) * cfg["batch_size"]
        random.seed(1)
        np.random.seed(1)
        torch.manual_seed(1)
        t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % tracks,
                                    track_width=widths[i % tracks]), cfg, device="cuda")
        side[name] = (t, t.train_iter())
    ms = {k: {"plain": [], "resample": []} for k in side}
    for u in range(warm + 1 + repeats):
        for name, (t, it) in side.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            next(it)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if u > warm:
                ms[name]["resample" if u % resample_every == 0 else "plain"].append(dt)
    res = {"envs": envs, "num_steps": T, "tracks": tracks, "track_resample_every": resample_every,
           "unit": "ms per update on the host clock between device synchronises"}
    for kind in ("plain", "resample"):
        if ms["replay"][kind]:
            res[kind] = {k: summary(v[kind]) for k, v in ms.items()}
            a, b = res[kind]["replay"], res[kind]["curriculum"]
            res[kind]["replay_over_curriculum"] = round(a["median"] / b["median"], 4)
            res[kind]["within_spread"] = bool(abs(a["median"] / b["median"] - 1.0) <= max(a["spread"], b["spread"]))
    for t, _ in side.values():
        t.envs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x128,65536x16")
    ap.add_argument("--slots", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--tracks", type=int, default=512)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--resample-every", type=int, default=4)
    ap.add_argument("--skip-updates", action="store_true", help="parts (1) and (2) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_replay", "bench_track_replay.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_replay measures on the GPU: no device found")
    res = {"command": "python tools/bench_track_replay.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "tally": [], "tables": [], "update": []}

    def save(part, row):
        res[part].append(row)
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # after every part: a later failure keeps what was measured
            json.dump(res, f, indent=1)
            f.write("\n")

    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    for envs, T in shapes:
        for slots in (a.tracks, envs):
            save("tally", tally(envs, T, slots, a.launches, a.repeats))
    for n in a.slots:
        save("tables", tables(n, a.launches if n <= 4096 else max(a.launches // 10, 2), a.repeats))
    if not a.skip_updates:
        for envs, T in shapes:
            save("update", update_pair(envs, T, a.tracks, a.repeats, a.resample_every))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
