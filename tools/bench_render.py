"""Device time of a rendered step: k_raster_trail + k_raster_frame for the 200
episodes of the evaluate.py protocol at 800 x 800, against a plain device fill
of the same output bytes (the write ceiling) in the same run.

The envs are stepped with seeded random actions so that paths grow and cars
move; only the two render launches are timed, with stream events around them,
per step, over ``--steps`` steps after ``--warmup`` steps.  The fill of the same
buffer is timed in the same loop, alternating with the render.  Prints one JSON
line: the medians, their ratio and the achieved rates.

    python tools/bench_render.py --out profiles/render/bench_render.json

Bytes per step, from the shapes: the frame kernel writes 3 B and reads 2 B per
pixel (static class, trail bits); the trail kernel touches a few dozen pixels
per car and is counted in the time, not in the bytes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render needs a HIP device"
    from rx.evaluate import eval_pool
    from rx.render import Renderer
    from rx.vector_env import RacingVectorEnv
    cps, ws, _ = eval_pool()
    v = RacingVectorEnv(cps, ws, n_agents=1, device="cuda", autoreset="disabled")
    N, S = v.num_envs, args.size
    r = Renderer(v, size=S)
    v.reset_device()
    r.begin()
    out = torch.empty((N, S, S, 3), dtype=torch.uint8, device=v.device)
    rng = np.random.default_rng(0)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]
    for t in range(args.warmup + args.steps):
        act = np.empty((N, 1, 2), dtype=np.float32)
        act[..., 0] = rng.uniform(-0.3, 0.3, (N, 1))
        act[..., 1] = rng.uniform(0.5, 1.0, (N, 1))
        v.step_device(torch.from_numpy(act).cuda())
        st = v.state  # rx_state_export, before the timed region
        e = ev[t - args.warmup] if t >= args.warmup else None
        if e:
            e[0].record()
        r.canvas.add_points(st["x"], st["y"])
        if e:
            e[1].record()
        r.canvas.compose(st["x"], st["y"], st["angle"], out)
        if e:
            e[2].record()
        out.fill_(255)
        if e:
            e[3].record()
    torch.cuda.synchronize()
    trail = [e[0].elapsed_time(e[1]) for e in ev]
    frame = [e[1].elapsed_time(e[2]) for e in ev]
    fill = [e[2].elapsed_time(e[3]) for e in ev]
    both = [a + b for a, b in zip(trail, frame)]
    med = statistics.median
    px = N * S * S
    res = {"metric": "device time of one rendered step (ms): k_raster_trail + k_raster_frame", "images": N, "size": S,
           "steps": args.steps, "warmup": args.warmup, "bytes_written": 3 * px, "bytes_read": 2 * px,
           "trail_ms_median": round(med(trail), 4), "frame_ms_median": round(med(frame), 4),
           "render_ms_median": round(med(both), 4), "render_ms_min": round(min(both), 4),
           "render_ms_max": round(max(both), 4), "fill_ms_median": round(med(fill), 4),
           "fill_ms_min": round(min(fill), 4), "fill_ms_max": round(max(fill), 4),
           "ratio_render_over_fill": round(med(both) / med(fill), 3),
           "frame_written_GBps": round(3 * px / med(frame) / 1e6, 1),
           "frame_read_plus_written_GBps": round(5 * px / med(frame) / 1e6, 1),
           "fill_GBps": round(3 * px / med(fill) / 1e6, 1), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    v.close()


if __name__ == "__main__":
    main()
