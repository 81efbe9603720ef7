"""League play: what the policy-bank launch costs, and what a table costs.

Table size P = 6 policies on the 40 x 5 protocol: 30 ordered pairs, 6,000
two-car envs, 12,000 policy rows per step.  Three comparisons, one JSON:

 (a) device time of ONE rx_policy_act_bank launch over the 12,000 rows against
     ONE rx_policy_act launch over the same rows with one policy (the floor: the
     same tiles, every row on the same weights) -- with the league's seating
     (pairings contiguous, tile_cars = 2), with every row on policy 0 (the
     loop's overhead alone) and with six policies in tile-aligned blocks (the
     bank's footprint without a mixed tile);
 (b) the same bank launch against the alternative design, per-policy strided
     rx_policy_act launches: 12 launches of 1,000 strided rows (6 policies x 2
     cars: the same work, a floor -- no env layout puts BOTH cars' rows of every
     policy in one range) and the 36 launches the pairing-major layout needs (car
     0: 6 ranges of 1,000 envs; car 1: 30 ranges of 200);
 (c) wall time of one league table (League.play) against 30 MultiEvaluator(backend=
     "fused") runs of 200 episodes each -- what could be run before, both cars on
     ONE policy, so it answers another question and is the cost yardstick only.

(a), (b): ``--launches`` back-to-back launches between two device events, the
variants interleaved, ``--rounds`` rounds, the median per-launch time; every
variant is warmed first.  (c): host clock around work that ends in a device
synchronise; set-up (env construction) is reported apart from the runs.

    python tools/bench_league.py --out profiles/league/bench_league.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P, EPISODES, D = 6, 200, 19


def launch_times(variants, launches, rounds):
    """Median device microseconds per call of each variant: {name: fn}, fn() enqueues one call."""
    for fn in variants.values():  # warm-up: code objects, first-use allocations
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / launches)
    return {k: round(statistics.median(v), 3) for k, v in out.items()}, \
        {k: [round(min(v), 3), round(max(v), 3)] for k, v in out.items()}


def policy_launches(prec, launches, rounds):
    from league import random_agents
    from rx import _lib
    from rx.league import PolicyBank, all_pairs, seating
    L = _lib.load()
    dev = "cuda"
    agents = random_agents(P)
    bank = PolicyBank(agents, device=dev)
    pairs = all_pairs(P)
    seat = seating(pairs, EPISODES, P)
    N = seat.shape[0]
    g = torch.Generator(device=dev).manual_seed(3)
    obs = torch.rand((N, 2, D), device=dev, generator=g) * 2.0 - 1.0
    eps = torch.empty((N, 2, 2), device=dev).normal_(generator=g)
    act = torch.zeros((N, 2, 2), device=dev)
    lp, val = torch.zeros(2 * N, device=dev), torch.zeros(2 * N, device=dev)
    pr = _lib.PRECISION[prec]
    s = _lib.stream_ptr(None)
    keep = []

    def single(params, log_std, n, obs_t, eps_t, act_t, lp_t, val_t, obs_stride=0, act_stride=0):
        io = _lib.RxPolicyIO(D, n, _lib.view_ptr(obs_t), _lib.view_ptr(eps_t), _lib.view_ptr(params),
                             _lib.view_ptr(log_std), _lib.view_ptr(act_t), _lib.view_ptr(lp_t), _lib.view_ptr(val_t),
                             obs_stride, act_stride, pr, None, 0)
        keep.append(io)
        return lambda: _lib.check(L.rx_policy_act(ctypes.byref(io), s), "rx_policy_act")

    def banked(ids, tile_cars):
        idt = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(dev)
        io = _lib.RxPolicyIO(D, 2 * N, _lib.ptr(obs), _lib.ptr(eps), _lib.ptr(bank.params), _lib.ptr(bank.log_std),
                             _lib.ptr(act), _lib.ptr(lp), _lib.ptr(val), 0, 0, pr, None, 0)
        b = _lib.RxPolicyBankIO(io, P, tile_cars, bank.stride, _lib.ptr(idt))
        keep.extend((idt, b))
        return lambda: _lib.check(L.rx_policy_act_bank(ctypes.byref(b), s), "rx_policy_act_bank")

    # per-policy strided launches: car q of the env range [lo, hi) on policy p
    eps_car = [eps[:, q].contiguous() for q in (0, 1)]  # rx_policy_act reads eps rows back to back
    lpc, valc = [torch.zeros(N, device=dev) for _ in (0, 1)], [torch.zeros(N, device=dev) for _ in (0, 1)]

    def strided(p, q, lo, hi):
        return single(bank.params[p], bank.log_std[p], hi - lo, obs[lo:hi, q], eps_car[q][lo:hi], act[lo:hi, q],
                      lpc[q][lo:hi], valc[q][lo:hi], 2 * D, 4)
    runs36 = []
    for k, (i, j) in enumerate(pairs):
        runs36.append(strided(j, 1, k * EPISODES, (k + 1) * EPISODES))
    for p in range(P):  # car 0 of pairs (p, *): one range of (P - 1) * EPISODES envs
        runs36.append(strided(p, 0, p * (P - 1) * EPISODES, (p + 1) * (P - 1) * EPISODES))
    assert len(runs36) == P * (P - 1) + P
    runs12 = [strided(p, q, p * (P - 1) * EPISODES, (p + 1) * (P - 1) * EPISODES) for p in range(P) for q in (0, 1)]
    blk = np.arange(N) // 16
    aligned = np.stack([blk % P, (blk + 1) % P], axis=1).astype(np.int32)
    mixed = sum(int(len(np.unique(seat[16 * t:16 * t + 16, q])) > 1) for q in (0, 1) for t in range((N + 15) // 16))
    variants = {
        "single_policy": single(bank.params[0], bank.log_std[0], 2 * N, obs, eps, act, lp, val),
        "bank_one_policy": banked(np.zeros(2 * N, np.int32), 2),
        "bank_league_seating": banked(seat.reshape(-1), 2),
        # six policies, none sharing a tile (16-env blocks round robin): the bank's cache footprint without mixed tiles
        "bank_six_policies_uniform_tiles": banked(aligned.reshape(-1), 2),
        "bank_league_seating_interleaved_tiles": banked(seat.reshape(-1), 1),
        "per_policy_12_launches": lambda: [f() for f in runs12],
        "per_policy_36_launches": lambda: [f() for f in runs36],
    }
    med, span = launch_times(variants, launches, rounds)
    return {"us_per_step": med, "min_max_us": span, "tiles": 2 * ((N + 15) // 16), "tiles_with_two_policies": mixed,
            "bank_over_single": round(med["bank_league_seating"] / med["single_policy"], 3),
            "bank_one_policy_over_single": round(med["bank_one_policy"] / med["single_policy"], 3),
            "per_policy_12_over_bank": round(med["per_policy_12_launches"] / med["bank_league_seating"], 3),
            "per_policy_36_over_bank": round(med["per_policy_36_launches"] / med["bank_league_seating"], 3)}


def table_wall(max_steps, runs):
    from league import random_agents
    from rx.evaluate import MultiEvaluator
    from rx.league import League, PolicyBank
    agents = random_agents(P)
    bank = PolicyBank(agents, device="cuda")
    pairs = [(i, j) for i in range(P) for j in range(P) if i != j]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    t_lg_setup, lg = clock(lambda: League(max_steps=max_steps, device="cuda"))
    t_first, res = clock(lambda: lg.play(bank))  # builds the 6,000-env match env: set-up, and the warm-up
    t_ev_setup, ev = clock(lambda: MultiEvaluator(max_steps=max_steps, device="cuda", backend="fused"))
    clock(lambda: ev.run(agents[0]))  # warm-up
    lg_s, lg_steps, ev_s, ev_steps = [], [], [], []
    torch.manual_seed(99)
    for _ in range(runs):  # interleaved
        dt, res = clock(lambda: lg.play(bank))
        lg_s.append(dt)
        lg_steps.append(int(res.record[:, :, 2].max()))
        steps = []

        def thirty():
            for i, _j in pairs:  # what could be run before: policy i in BOTH cars, once per pairing
                r = ev.run(agents[i])
                steps.append(max(e["steps"] for e in r["all_episodes"]))
        dt, _ = clock(thirty)
        ev_s.append(dt)
        ev_steps.append(int(sum(-(-s // 50) * 50 for s in steps)))
    out = {"max_steps": max_steps, "runs": runs,
           "league_play_median_s": round(statistics.median(lg_s), 4), "league_play_s": [round(x, 4) for x in lg_s],
           "league_steps": lg_steps, "league_first_play_with_env_build_s": round(t_first + t_lg_setup, 4),
           "thirty_fused_evals_median_s": round(statistics.median(ev_s), 4),
           "thirty_fused_evals_s": [round(x, 4) for x in ev_s], "thirty_fused_evals_steps_total": ev_steps,
           "evaluator_setup_s": round(t_ev_setup, 4),
           "ratio_evals_over_league": round(statistics.median(ev_s) / statistics.median(lg_s), 3),
           "draws": int(np.triu(res.draws).sum()), "episodes": int(res.seat.shape[0])}
    lg.close()
    ev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip-table", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_league.py measures on the GPU: no device found")
    out = {"command": "python tools/bench_league.py " + " ".join(sys.argv[1:]),
           "shape": {"policies": P, "pairs": P * (P - 1), "envs": P * (P - 1) * EPISODES,
                     "rows": 2 * P * (P - 1) * EPISODES, "obs_dim": D},
           "launches_per_window": args.launches, "rounds": args.rounds,
           "policy_launch": {prec: policy_launches(prec, args.launches, args.rounds) for prec in ("fp32", "bf16")}}
    if not args.skip_table:
        out["league_table"] = table_wall(args.max_steps, args.runs)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
