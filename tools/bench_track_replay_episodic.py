"""Replay scores on episodic draws: what the replay draw costs the rollout, and the tally by per-step slot.

    python tools/bench_track_replay_episodic.py [--repeats 15]
        [--out profiles/track_replay_episodic/bench_track_replay_episodic.json]

(1) Rollout ms per update, tools/bench_track_episodic.py's protocol (trainers in one
    process timed in turn, ``collect_rollout`` on the wall clock between two device
    synchronises, two warm-up rollouts each, then --repeats interleaved rounds,
    untrained policy): ``rx.track_episodic.EpisodicCurriculumPPO`` with
    ``episodic_slots=True`` (the baseline) against
    ``rx.track_replay_episodic.EpisodicReplayCurriculumPPO``, at 4,096 envs x 128
    steps on 512 slots and 65,536 x 16 on 4,096 slots.  The two differ only in the
    draw of the envs that ended.  ``gate``: the new median lies within max(3 %, the
    baseline's own (max - min) / median) of the baseline's median (DESIGN.md §5,
    the league-training rule).  Both trainers collect without an update in between,
    so the replay scores stay unseen and the rank table is the initial one.

(2) The tally: rx_track_learn_tally_slots against rx_track_learn_tally on the same
    [T][N] advantages, device events around --launches back-to-back launches, the
    variants interleaved, median of --repeats rounds: the old kernel (one array),
    the new one with constant columns and dones null (two arrays), with constant
    columns and a zero dones (three), and on the slots and dones of the replay
    trainer's last rollout (slot changes inside the chunks; ``slot_changes`` counts
    them).

It needs a HIP device and fails without one.
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


def trainers(envs, T, slots):
    """-> {name: (trainer, rollout buffers)} on one pool of ``slots`` tracks."""
    import numpy as np
    import torch
    from rx.configs import base_config
    from rx.envs import RacingEnv
    from rx.track import gen_tracks
    from rx.track_episodic import EpisodicCurriculumPPO
    from rx.track_replay_episodic import EpisodicReplayCurriculumPPO
    rng = np.random.RandomState(5)
    pool = gen_tracks(slots, seed=None, rng=rng)
    widths = [int(rng.randint(6, 10)) for _ in range(slots)]
    side = {}
    for name, cls in (("episodic", EpisodicCurriculumPPO), ("episodic_replay", EpisodicReplayCurriculumPPO)):
        cfg = base_config(num_envs=envs, num_steps=T, kl_target=1e9, track_backend="device", curriculum_refresh=0.0,
                          episodic_slots=True)
        random.seed(1)
        np.random.seed(1)
        torch.manual_seed(1)
        t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % slots,
                                    track_width=widths[i % slots]), cfg, device="cuda")
        assert t.envs.schedule()["lane_tracks"] == 1
        bufs = list(t._buffers()) + [t.envs.buf["obs"].clone(), torch.zeros(envs, device="cuda")]
        side[name] = (t, bufs)
    return side


def tally(t, bufs, repeats, launches):
    """(2) on the replay trainer ``t``: its own slots and dones of the last rollout, random advantages."""
    import torch
    from rx import _lib
    rep, L = t.replay, t.replay.L
    slots, dones = t.slots(), bufs[3]
    T, N = slots.shape
    g = torch.Generator(device="cuda").manual_seed(3)
    adv = torch.randn((T, N), device="cuda", generator=g)
    const = rep.venv._st["track"][None, :].expand(T, N).contiguous()
    zero = torch.zeros((T, N), device="cuda")
    q, lt, s = _lib.ptr, ctypes.byref(rep.lt), _lib.stream_ptr()
    calls = {
        "tally": lambda: L.rx_track_learn_tally(lt, T, N, q(adv), s),
        "slots_const": lambda: L.rx_track_learn_tally_slots(lt, T, N, q(adv), q(const), None, s),
        "slots_const_dones": lambda: L.rx_track_learn_tally_slots(lt, T, N, q(adv), q(const), q(zero), s),
        "slots_rollout": lambda: L.rx_track_learn_tally_slots(lt, T, N, q(adv), q(slots), q(dones), s),
    }
    us = {k: [] for k in calls}
    for r in range(2 + repeats):
        for name, call in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                assert call() == 0, L.rx_last_error()
            b.record()
            b.synchronize()
            if r >= 2:
                us[name].append(a.elapsed_time(b) * 1e3 / launches)
    rep.learn.zero_()
    res = {k: summary(v) for k, v in us.items()}
    res["unit"] = "us per launch, device events"
    res["launches_per_round"] = launches
    for k in ("slots_const", "slots_const_dones", "slots_rollout"):
        res[k + "_over_tally"] = round(res[k]["median"] / res["tally"]["median"], 3)
    res["bytes_over_tally"] = {"slots_const": 2.0, "slots_const_dones": 3.0, "slots_rollout": 3.0}
    res["slot_changes"] = int((slots[1:] != slots[:-1]).sum().item())
    res["autoreset_rows"] = int((dones != 0).sum().item())
    res["elements"] = T * N
    return res


def shape(envs, T, slots, repeats, launches):
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
           "unit": "ms on the host clock between device synchronises",
           "episodes_ended_per_step": {k: round(v / (repeats * T), 1) for k, v in episodes.items()}}
    base, new = res["episodic"], res["episodic_replay"]
    res["replay_over_episodic"] = round(new["median"] / base["median"], 4)
    res["replay_minus_episodic_us_per_step"] = round((new["median"] - base["median"]) * 1e3 / T, 2)
    res["gate_bound"] = round(max(0.03, base["spread"]), 4)
    res["gate"] = bool(abs(res["replay_over_episodic"] - 1.0) <= res["gate_bound"])
    res["tally"] = tally(*side["episodic_replay"], repeats, launches)
    for t, _ in side.values():
        t.envs.close()
    del side
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x128x512,65536x16x4096", help="envs x steps x slots, comma-separated")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--launches", type=int, default=100, help="back-to-back tally launches per timed round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_replay_episodic",
                                                  "bench_track_replay_episodic.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_track_replay_episodic measures on the GPU: no device found")
    res = {"command": "python tools/bench_track_replay_episodic.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "shapes": []}
    for s in a.shapes.split(","):
        envs, T, slots = (int(x) for x in s.split("x"))
        res["shapes"].append(shape(envs, T, slots, a.repeats, a.launches))
        print(json.dumps(res["shapes"][-1]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # after every shape: a later failure keeps what was measured
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
