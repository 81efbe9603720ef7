"""Render chosen episodes of the evaluation pool (rx.evaluate.Evaluator: 40
tracks x 5 runs, all stepped side by side on the device) to a frame stack.

    python tools/render_eval.py --episodes 0 7 64 199 --out runs.npy
    python tools/render_eval.py --episodes 0 7 64 199 --mosaic --out grid.npy --size 400 --every 4

Without ``--mosaic`` the output is uint8 [frames, episodes, size, size, 3];
with it (exactly four episodes) the 2 x 2 grid of visualization_grid,
uint8 [frames, H, W, 3], composed in place on the device.  ``--checkpoint`` is
an Agent state_dict (torch.save); without it a freshly initialised agent
drives, which shows the pipeline and little else.  Only the chosen episodes
are drawn; all 200 are stepped.  An episode that has ended keeps its last
frame.  Frames are held on the host until the end: ``--size``, ``--every`` and
``--max-steps`` bound the memory.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "self-play-racing_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--mosaic", action="store_true")
    ap.add_argument("--padding", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.mosaic and len(args.episodes) != 4:
        ap.error("--mosaic lays out exactly four episodes")
    from rx.agent import Agent
    from rx.evaluate import Evaluator
    from rx.render import Renderer
    torch.manual_seed(args.seed)
    ev = Evaluator(max_steps=args.max_steps, device="cuda")
    v = ev.venv
    agent = Agent(v.single_observation_space, v.single_action_space).to(v.device)
    if args.checkpoint:
        agent.load_state_dict(torch.load(args.checkpoint, map_location=v.device))
    r = Renderer(v, env_ids=args.episodes, size=args.size)
    obs = v.reset_device()
    r.begin()
    active = torch.ones(v.num_envs, dtype=torch.bool, device=v.device)
    frames = []
    with torch.no_grad():
        for t in range(args.max_steps):
            obs, _, done = v.step_device(agent.get_action_and_value(obs)[0])
            r.step()
            active &= ~done.bool()
            last = not bool(active[torch.as_tensor(args.episodes, device=v.device)].any())
            if t % args.every == 0 or last:
                f = r.mosaic(2, 2, args.padding) if args.mosaic else r.frame()
                frames.append(f.cpu().numpy())
            if last:
                break
    np.save(args.out, np.stack(frames))
    print(f"{len(frames)} frames of episodes {args.episodes} -> {args.out}")
    ev.close()


if __name__ == "__main__":
    main()
