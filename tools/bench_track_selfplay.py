"""Track curriculum for self-play: what the per-step tally costs a two-car rollout, what the
tally kernel costs alone, and what the boundary costs.

    python tools/bench_track_selfplay.py [--repeats 10] [--out profiles/track_selfplay/bench.json]

(a) Rollout ms per update at 8,192 two-car envs x 128 steps (BASELINE.json configs[3]) on a
    512-slot pool of distinct tracks: ``SelfPlayPPO`` against ``SelfPlayCurriculumPPO`` and
    ``LeagueSelfPlayPPO`` against ``LeagueCurriculumPPO``, every trainer with one snapshot in
    its pool so the rollout is the one library call.  All sides live in one process and are
    timed in turn (interleaved: drift hits them alike): ``collect_rollout`` on the wall clock
    between two device synchronises, two warm-ups each, then --repeats rounds; the policy is
    the untrained one (no update runs between rollouts).  A third self-play side,
    ``selfplay_info``, is the parent made to write the info rows: it splits the tally launch
    from the info writes.  The league parent writes the info rows already (its draw reads the
    placement), so there the whole difference is the tally launch.  Per side: every run, min,
    median, max, spread = (max - min) / median.  The parents are the yardstick.

(b) k_track_tally2 alone at 8,192 envs on 512 slots, by device events over 100 launches: no
    env ended; every env ended on one slot; every env ended on its own slot (env i on slot
    i % 512: 64 distinct slots in every wave).

(c) The boundary at the same shape, each between device synchronises: ``reset_device()``
    alone (the parent's rebuild), ``reassign_tracks`` (with the scores, the draw and the
    download of the ids before it, timed apart), and ``set_tracks`` with a quarter of the
    slots retired (the device build of the pool's table timed apart).

The single-agent figures of profiles/curriculum/bench_curriculum.json are copied beside the
results when that file is present.  It needs a HIP device and fails without one.
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


def summary(ms):
    med = statistics.median(ms)
    return {"runs_ms": [round(x, 3) for x in ms], "min": round(min(ms), 3), "median": round(med, 3),
            "max": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 4)}


def pool_of(slots, seed=1):
    import numpy as np
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    return gen_tracks(slots, seed=None, rng=rng), [int(rng.randint(6, 10)) for _ in range(slots)]


def rollouts(envs, T, slots, repeats):
    import numpy as np
    import torch
    from rx import _lib
    from rx.configs import self_play_config
    from rx.envs import MultiRacingEnv
    from rx.league_train import LeagueSelfPlayPPO
    from rx.selfplay import SelfPlayPPO
    from rx.track_selfplay import LeagueCurriculumPPO, SelfPlayCurriculumPPO
    pool, widths = pool_of(slots)
    side = {}
    for name, cls in (("selfplay", SelfPlayPPO), ("selfplay_info", SelfPlayPPO),
                      ("selfplay_curriculum", SelfPlayCurriculumPPO), ("league", LeagueSelfPlayPPO),
                      ("league_curriculum", LeagueCurriculumPPO)):
        cfg = self_play_config(num_envs=envs, num_steps=T, snapshot_freq=1, pool_size=5, checkpoint=False,
                               kl_target=1e9, track_backend="device")
        random.seed(1)
        np.random.seed(1)
        torch.manual_seed(1)
        t = cls(lambda i: MultiRacingEnv(2, 11, pool, i % slots, widths), cfg, device="cuda")
        t.advance_pool(1)  # one snapshot: the frozen / bank opponent, so the rollout is the library call
        t.update_opponent()
        if name == "selfplay_info":  # every step io of this trainer also carries the info rows
            v = t.envs.venv
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
    res = {"envs": envs, "num_steps": T, "slots": int(side["selfplay_curriculum"][0].curriculum.n_tracks)}
    res.update({k: summary(v) for k, v in ms.items()})
    res["library_call"] = {k: t.__dict__.get("_td_steps_rollout") is not None or
                           t.__dict__.get("_sp_steps_rollout") is not None or
                           t.__dict__.get("_lg_steps_rollout") is not None for k, (t, _) in side.items()}
    res["episodes_ended_per_step"] = {k: round(v / (repeats * T), 1) for k, v in episodes.items()}
    for k in ("selfplay_curriculum", "league_curriculum"):
        res[k + "_tallied"] = int(side[k][0].curriculum.tally[:, 0].sum())
    med = lambda k: res[k]["median"]  # noqa: E731
    res["selfplay_curriculum_over_selfplay"] = round(med("selfplay_curriculum") / med("selfplay"), 4)
    res["selfplay_info_over_selfplay"] = round(med("selfplay_info") / med("selfplay"), 4)
    res["league_curriculum_over_league"] = round(med("league_curriculum") / med("league"), 4)
    res["selfplay_tally_us_per_step"] = round((med("selfplay_curriculum") - med("selfplay_info")) * 1e3 / T, 2)
    res["selfplay_info_us_per_step"] = round((med("selfplay_info") - med("selfplay")) * 1e3 / T, 2)
    res["league_tally_us_per_step"] = round((med("league_curriculum") - med("league")) * 1e3 / T, 2)
    for t, _ in side.values():
        t.envs.close()
    del side
    torch.cuda.empty_cache()
    return res


def tally_alone(envs, slots, launches=100):
    import numpy as np
    import torch
    from rx import _lib
    L = _lib.load()
    rng = np.random.RandomState(3)
    info = np.zeros((envs, 2, _lib.RX_INFO_W))
    info[:, :, _lib.RX_INFO_PROGRESS] = rng.rand(envs, 2)
    info[:, 0, _lib.RX_INFO_PLACEMENT], info[:, 1, _lib.RX_INFO_PLACEMENT] = 1.0, 2.0
    d_info = torch.from_numpy(info).cuda()
    d_term = torch.from_numpy((rng.rand(envs) < 0.5).astype(np.uint8)).cuda()
    tally = torch.zeros((slots, 4), dtype=torch.int64, device="cuda")
    duel = torch.zeros((slots, 4), dtype=torch.int64, device="cuda")
    cases = {"none_ended": (np.arange(envs) % slots, 0.0), "all_on_one_slot": (np.full(envs, slots // 2), 1.0),
             "all_on_own_slot": (np.arange(envs) % slots, 1.0)}
    out = {"envs": envs, "slots": slots, "launches": launches, "unit": "us per launch, device events"}
    for name, (track, done) in cases.items():
        d_track = torch.from_numpy(track.astype(np.int32)).cuda()
        d_done = torch.full((envs,), done, dtype=torch.float32, device="cuda")
        tc = _lib.RxTrackIO(slots, 0, _lib.ptr(d_track), _lib.ptr(tally), None, None, None, 0)
        td = _lib.RxTrackDuelIO(0, _lib.ptr(duel))
        s = _lib.stream_ptr(None)

        def launch():
            _lib.check(L.rx_track_tally2(ctypes.byref(tc), ctypes.byref(td), envs, _lib.ptr(d_done), _lib.ptr(d_term),
                                         _lib.ptr(d_info), s), "rx_track_tally2")
        for _ in range(10):
            launch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        torch.cuda.synchronize()
        out[name] = round(a.elapsed_time(b) * 1e3 / launches, 3)
    return out


def boundary(envs, slots, repeats):
    import numpy as np
    import torch
    from rx.curriculum import host_fresh_tracks
    from rx.track_device import DeviceTrackTable
    from rx.track_selfplay import DuelTrackCurriculum
    from rx.vector_env import RacingVectorEnv
    pool, widths = pool_of(slots)
    cps = [np.asarray(pool[k], dtype=np.float64) for k in range(slots)]
    ws = [float(w) for w in widths]
    v = RacingVectorEnv([cps[i % slots] for i in range(envs)], [ws[i % slots] for i in range(envs)], n_agents=2,
                        device="cuda", track_backend="device")
    v.reset_device()
    cur = DuelTrackCurriculum(v, 0, seed=1)
    rng = np.random.RandomState(5)
    t = np.zeros((slots, 4), dtype=np.int64)
    t[:, 0] = rng.randint(1, 60, size=slots)
    d = np.zeros((slots, 4), dtype=np.int64)
    d[:, 0] = (rng.rand(slots) * (t[:, 0] + 1)).astype(np.int64).clip(0, t[:, 0])
    cur.tally.copy_(torch.from_numpy(t))
    cur.duel.copy_(torch.from_numpy(d))
    sync, now = torch.cuda.synchronize, time.perf_counter
    parts = {k: [] for k in ("reset_device_ms", "scores_draw_download_ms", "reassign_tracks_ms", "table_build_ms",
                             "set_tracks_ms")}
    for r in range(1 + repeats):
        sync()
        t0 = now()
        v.reset_device()
        sync()
        t1 = now()
        cur.scores()
        toe = cur.draw(2 * r + 1).cpu().numpy()
        t2 = now()
        v.reassign_tracks(toe)
        sync()
        t3 = now()
        retired = rng.choice(slots, size=slots // 4, replace=False)
        new_cps, new_ws = host_fresh_tracks(1, 2 * r + 2, len(retired))
        for k, cp, w in zip(retired, new_cps, new_ws):
            cps[k], ws[k] = np.asarray(cp, dtype=np.float64), float(w)
        toe = cur.draw(2 * r + 2).cpu().numpy()
        sync()
        t4 = now()
        table = DeviceTrackTable.build(cps, ws, device="cuda")
        sync()
        t5 = now()
        v.set_tracks(table, toe)
        sync()
        t6 = now()
        if r:
            for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t5 - t4, t6 - t5)):
                parts[k].append(dt * 1e3)
    out = {"envs": envs, "slots": slots, "retired_per_set_tracks": slots // 4}
    out.update({k: summary(x) for k, x in parts.items()})
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_selfplay", "bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_selfplay measures on the GPU: no device found")
    res = {"command": "python tools/bench_track_selfplay.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "unit": "ms on the host clock between device synchronises unless stated"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    single = os.path.join(ROOT, "profiles", "curriculum", "bench_curriculum.json")
    if os.path.exists(single):
        with open(single) as f:
            s = json.load(f)
        res["single_agent_for_comparison"] = {
            "source": "profiles/curriculum/bench_curriculum.json",
            "rollout": [{k: (r[k]["median"] if isinstance(r[k], dict) else r[k])
                         for k in ("envs", "num_steps", "slots", "ppo", "ppo_info", "curriculum", "curriculum_over_ppo",
                                   "tally_us_per_step", "info_us_per_step")} for r in s["rollout"]],
            "resample": [{k: (r[k]["median"] if isinstance(r[k], dict) else r[k])
                          for k in ("slots", "envs", "scores_ms", "draw_and_download_ms", "reassign_ms")}
                         for r in s["resample"]]}
    for name, fn in (("rollout", lambda: rollouts(a.envs, a.steps, a.slots, a.repeats)),
                     ("tally_alone", lambda: tally_alone(a.envs, a.slots)),
                     ("boundary", lambda: boundary(a.envs, a.slots, a.repeats))):
        res[name] = fn()
        print(json.dumps(res[name]), flush=True)
        save()  # after every part: a later failure keeps what was measured
    print("wrote", a.out)


if __name__ == "__main__":
    main()
