"""Dump what rx_assign builds, for comparing two builds of librx (profiles/assign_plan/).

    python tools/dump_assign.py --out new.json [--lib path/to/librx.so]
    python tools/dump_assign.py --compare parent.json new.json

For some forty configurations -- the project's real shapes (65,536 single-agent envs on 7
slots, 4,096 envs on 128 slots, 65,536 envs with a slot each (lane-varying), 2,048 envs on the
wide schedule, 8,192 two-car envs, ...) and a sample of tests/test_assign_plan_cpu.py's grid --
a handle is created, given a table of circular tracks (only the waypoint counts matter here)
and assigned; rx_schedule (the dynamics-launch counter masked), the raw rx_ray_waves table
and rx_env_order are recorded: the schedule and the sort bins in full, the tables as their
length, a SHA-256 of their int32 bytes and their first records.  Nothing is launched.  The
library is loaded with ctypes alone (--lib: any build with ABI v25, e.g. one of the parent
commit), so the tool does not depend on what rx._lib binds.  Where the library has
rx_assign_plan, its outputs for the same inputs are compared with the handle's
("plan_equals_handle").  --compare exits non-zero unless the two dumps' configurations are
identical entry for entry (that key aside).  Needs a HIP device (rx_create).
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "self-play-racing_amd")]

MIXES = {"single": [130], "full": [64], "one_each": [1] * 70, "ragged": [63, 1, 65, 130, 64],
         "holes": [65, 0, 0, 64, 0, 1, 130]}


LONG_SLOTS = 40  # a table of this many slots gets 2,048 waypoints each: more than 65,536 sort bins at shift 0


def configs():
    """(name, A, R, ray_order, sort_interval, envs per slot, schedule overrides)"""
    def even(n, k):
        return [n // k + (i < n % k) for i in range(k)]
    out = [("65536x1_7slots", 1, 11, 2, 8, even(65536, 7), {}),
           ("4096x1_128slots", 1, 11, 2, 16, even(4096, 128), {}),
           ("65536x1_slot_each_lane_varying", 1, 11, 2, 8, [1] * 65536, {}),
           ("2048x1_wide", 1, 11, 2, 16, even(2048, 7), {}),
           ("8192x2_two_car", 2, 11, 2, 16, even(8192, 7), {}),
           ("16384x1_7slots", 1, 11, 2, 16, even(16384, 7), {}),
           ("4096x1_7slots", 1, 11, 2, 16, even(4096, 7), {}),
           ("65536x2_two_car", 2, 11, 2, 16, even(65536, 7), {}),
           ("65536x1_tail", 1, 11, 2, 8, even(65536, 7), dict(ray_tail=3, ray_tail_lpr=4)),
           ("65536x1_dispatch1", 1, 11, 2, 8, even(65536, 7), dict(ray_dispatch=1)),
           ("65536x1_octet_major", 1, 11, 2, 8, even(65536, 7), dict(ray_dispatch=-1)),
           ("65536x1_ray_major_17", 1, 17, 1, 8, even(65536, 7), {}),
           ("8256x1_env_major", 1, 11, 0, 16, even(8256, 7), {}),
           ("6000x1_mixed_slots", 1, 11, 2, 16, even(4500, 7) + [1] * 1500, {}),
           ("4096x1_long_tracks_sort_shift", 1, 11, 2, 16, even(4096, LONG_SLOTS), {})]
    sample = [dict(dyn_lpe=1, ray_lpr=1, lane_tracks=-1, ray_dispatch=3, ray_tail=3, ray_tail_lpr=4),
              dict(dyn_lpe=1, ray_lpr=2, lane_tracks=-1, ray_dispatch=1),
              dict(dyn_lpe=1, lane_tracks=1),
              dict(dyn_lpe=4, ray_lpr=4, ray_dispatch=2, reward_lpe=4, task_sort=3),
              dict(dyn_lpe=64, split=-1, argmin_window=32),
              dict(dyn_lpe=2, ray_lpr=1, ray_dispatch=-1, ray_tail=16)]
    i = 0
    for A, R, order in ((1, 11, 2), (1, 3, 2), (1, 16, 2), (1, 17, 1), (1, 1, 0), (2, 11, 2), (2, 16, 1), (2, 17, 0)):
        for mix in ("ragged", "holes", "one_each", "single"):
            s = dict(sample[i % len(sample)])
            if A == 2:
                s.update(dyn_lpe=0, reward_lpe=min(s.get("reward_lpe", 0), 2))
            out.append((f"grid_A{A}_R{R}_order{order}_{mix}_{i % len(sample)}", A, R, order, (0, 8)[i % 2], MIXES[mix], s))
            i += 1
    return out


SCHED_FIELDS = ("split", "wide_n", "dyn_lpe", "ray_lpr", "reward_lpe", "argmin_window", "seg_filter", "box_quadrants",
                "ray_dispatch", "ray_tail", "ray_tail_lpr", "task_sort", "lane_tracks")


def tracks(np, counts):
    """Circular tracks, slot k with 300 + 37 k % 200 waypoints (more than 1,024 slots: 20 + k % 13, to keep
    the table small; LONG_SLOTS slots: 2,048 each): rx_upload_tracks' arrays."""
    few = len(counts) <= 1024
    W = np.array([300 + (37 * k) % 200 if few else 20 + k % 13 for k in range(len(counts))], np.int64)
    if len(counts) == LONG_SLOTS:
        W[:] = 2048
    wp_off = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    ang = np.concatenate([np.arange(w) * (2 * np.pi / w) for w in W])
    nrm = np.stack([np.cos(ang), np.sin(ang)], 1)
    rad = np.repeat(40.0 + W / 10.0, W)[:, None]
    wp = nrm * rad
    seg, meta = [], np.zeros((len(W), 8))
    for k, w in enumerate(W):
        sl = slice(wp_off[k], wp_off[k + 1])
        for side in (4.0, -4.0):
            b = wp[sl] + side * nrm[sl]
            seg.append(np.concatenate([b, np.roll(b, -1, 0) - b], 1))
        meta[k] = [wp[sl][0, 0], wp[sl][0, 1], np.pi / 2, 8.0, 2 * np.pi * rad[wp_off[k], 0], 1.0, 0.0, 0.0]
    c = np.ascontiguousarray
    return wp_off, c(wp), c(nrm), c(np.concatenate(seg)), c(meta)


def digest(a):
    return {"n": int(len(a)), "sha256": hashlib.sha256(a.tobytes()).hexdigest(), "head": a[:8].tolist()}


def dump(a):
    import numpy as np
    import torch  # noqa: F401  (first: librx shares torch's HIP runtime)
    from rx import _build
    from rx._lib import RxConfig
    P, I = ctypes.c_void_p, ctypes.c_int32
    L = ctypes.CDLL(a.lib or _build.LIB)
    L.rx_last_error.restype = ctypes.c_char_p
    L.rx_create.argtypes = [ctypes.POINTER(RxConfig), ctypes.POINTER(P)]
    L.rx_destroy.argtypes = [P]
    L.rx_upload_tracks.argtypes = [P, I, P, P, P, P, P]
    L.rx_assign.argtypes = [P, P]
    L.rx_schedule.argtypes = [P, P]
    L.rx_ray_waves.argtypes = [P, P, I, P]
    L.rx_env_order.argtypes = [P, P, P, P]
    has_plan = hasattr(L, "rx_assign_plan")

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed ({rc}): {L.rx_last_error().decode()}")

    res = {"abi": L.rx_abi_version(), "has_rx_assign_plan": has_plan, "configs": {}}
    for name, A, R, order, si, counts, sched in configs():
        toe = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
        np.random.RandomState(len(toe)).shuffle(toe)
        N = len(toe)
        cfg = RxConfig(N, A, R, 3000, 0, 0, 0, 1.0, 8.0, 8, si, order, 8, *[int(sched.get(k, 0)) for k in SCHED_FIELDS], 0)
        wp_off, wp, nrm, seg, meta = tracks(np, counts)
        h = P()
        ok(L.rx_create(ctypes.byref(cfg), ctypes.byref(h)), "rx_create")
        ok(L.rx_upload_tracks(h, len(counts), wp_off.ctypes.data, wp.ctypes.data, nrm.ctypes.data, seg.ctypes.data,
                              meta.ctypes.data), "rx_upload_tracks")
        ok(L.rx_assign(h, toe.ctypes.data), "rx_assign")
        sch = np.zeros(18, np.int32)
        ok(L.rx_schedule(h, sch.ctypes.data), "rx_schedule")
        sch[16] = 0  # dynamics launches so far
        n = I(0)
        ok(L.rx_ray_waves(h, None, 0, ctypes.byref(n)), "rx_ray_waves")
        ray = np.zeros((n.value, 4), np.int32)
        ok(L.rx_ray_waves(h, ray.ctypes.data, n.value, ctypes.byref(n)), "rx_ray_waves")
        perm, bins, shift = np.zeros(N, np.int32), I(0), I(0)
        ok(L.rx_env_order(h, perm.ctypes.data, ctypes.byref(bins), ctypes.byref(shift)), "rx_env_order")
        L.rx_destroy(h)
        r = {"n_envs": N, "n_agents": A, "n_sensors": R, "ray_order": order, "sort_interval": si, "n_slots": len(counts),
             "sched": sched, "schedule": sch.tolist(), "ray_waves": digest(ray), "env_order": digest(perm),
             "sort_bins": bins.value, "sort_shift": shift.value}
        if has_plan:
            from rx import _lib
            p = _lib.assign_plan(cfg, wp_off, toe)
            r["plan_equals_handle"] = bool(
                list(p["schedule"].values()) == sch.tolist() and np.array_equal(p["ray_waves"], ray) and
                np.array_equal(p["perm"], perm) and (p["sort_bins"], p["sort_shift"]) == (bins.value, shift.value))
        res["configs"][name] = r
        print(name, r["schedule"], r["ray_waves"]["n"], r.get("plan_equals_handle"), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out, len(res["configs"]), "configurations")
    if has_plan and not all(r["plan_equals_handle"] for r in res["configs"].values()):
        raise SystemExit("rx_assign_plan differs from the handle")


def compare(pa, pb):
    ca, cb = (json.load(open(p))["configs"] for p in (pa, pb))
    bad = [k for k in sorted(set(ca) | set(cb))
           if {x: v for x, v in ca.get(k, {}).items() if x != "plan_equals_handle"} !=
              {x: v for x, v in cb.get(k, {}).items() if x != "plan_equals_handle"}]
    print(json.dumps({"a": pa, "b": pb, "configurations": len(ca), "identical": not bad, "differing": bad}))
    if bad:
        raise SystemExit(1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_plan", "dump.json"))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    compare(*a.compare) if a.compare else dump(a)
