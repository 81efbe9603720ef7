"""Drop-ins for utils/visualization.py: ``visualize_single_agent``,
``visualize_multi_agent`` and ``visualization_grid`` with the reference's
arguments and result dicts, drawn by rx.render on the device instead of pygame.

What differs from the reference, on purpose:

* the pixels follow rx.render's exact raster rules, not pygame's, and there is
  no HUD text and no model-name label (no font here); the numbers are in the
  returned dict and in ``info``;
* no window, no 60 Hz clock and no end-of-episode wait;
* frames go to ``video_path``: a ``.npy`` path gets one uint8 array
  [frames, size, size, 3] (RGB).  Frames are held in host memory until the
  episode ends -- 1.9 MB each at 800 x 800 -- so ``size=`` and ``every=`` (keep
  one frame in ``every``) bound it.  Any other suffix is written with OpenCV as
  the reference does (mp4v, 60 fps) and needs ``cv2``; without it the call
  fails with ImportError before the episode runs.  That branch has never been
  run: cv2 is not installed where this project is developed and tested.
"""
import os

import numpy as np
import torch

from .render import Renderer, mosaic_shape


class _Sink:
    """Frames -> ``path``: a .npy stack, or a video through cv2."""

    def __init__(self, path, width, height, fps=60):
        self.path = path
        self.npy = os.path.splitext(path)[1].lower() == ".npy"
        self.shape = (height, width, 3)
        self.frames = []
        self.writer = None
        if not self.npy:
            try:
                import cv2
            except ImportError as e:
                raise ImportError(f"writing {path!r} needs OpenCV (cv2), which is not installed; "
                                  f"use a .npy path for a raw frame stack") from e
            self.cv2 = cv2
            self.writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), fps, (width, height))

    def write(self, rgb):
        if self.npy:
            self.frames.append(np.ascontiguousarray(rgb))
        else:
            self.writer.write(self.cv2.cvtColor(rgb, self.cv2.COLOR_RGB2BGR))

    def close(self):
        if self.npy:
            stack = np.stack(self.frames) if self.frames else np.zeros((0,) + self.shape, dtype=np.uint8)
            np.save(self.path, stack)
        else:
            self.writer.release()


def _act(agent, obs, device):
    with torch.no_grad():
        t = torch.as_tensor(np.asarray(obs), dtype=torch.float32).unsqueeze(0).to(device)
        return agent.get_action_and_value(t)[0].cpu().numpy()[0]


def visualize_single_agent(env, agent, device, video_path, max_steps=2000, size=800, every=1):
    """visualization.py:62-161 for an rx.envs.RacingEnv."""
    sink = _Sink(video_path, size, size)
    obs, _ = env.reset()
    r = Renderer(env._vec(), size=size)
    r.begin()
    total_reward = 0
    step = 0
    info = {}
    for step in range(max_steps):
        obs, reward, terminated, truncated, info = env.step(_act(agent, obs, device))
        total_reward += reward
        r.step()
        if step % every == 0 or terminated or truncated:
            sink.write(r.frame()[0].cpu().numpy())
        if terminated or truncated:
            reason = "Finished" if info["finished"] else "Crashed" if info["crashed"] else "Time limit"
            print(f"{reason} | Steps: {step} | Reward: {total_reward:.1f} | Progress: {info['progress']:.1%}")
            break
    sink.close()
    return {"total_reward": total_reward, "steps": step + 1, "progress": info["progress"],
            "finished": info["finished"], "crashed": info["crashed"], "speed": info["speed"]}


def visualize_multi_agent(env, agent, device, video_path, max_steps=3000, size=800, every=1):
    """visualization.py:164-313 for an rx.envs.MultiRacingEnv: both cars driven by ``agent``."""
    sink = _Sink(video_path, size, size)
    obs_dict, _ = env.reset()
    r = Renderer(env._vec(), size=size)
    r.begin()
    total = [0, 0]
    step = 0
    info_dict = {}
    for step in range(max_steps):
        actions = {k: _act(agent, obs_dict[k], device) for k in ("0", "1")}
        obs_dict, reward_dict, done_dict, truncated, info_dict = env.step(actions)
        total[0] += reward_dict["0"]
        total[1] += reward_dict["1"]
        r.step()
        if step % every == 0 or done_dict["__all__"]:
            sink.write(r.frame()[0].cpu().numpy())
        if done_dict["__all__"]:
            if "placement" in info_dict["0"]:
                winner = "Car 0 (Red)" if info_dict["0"]["placement"] == 1 else "Car 1 (Blue)"
            else:
                winner = "Unknown"
            fin = [info_dict[k]["finished"] for k in ("0", "1")]
            crash = [info_dict[k]["crashed"] for k in ("0", "1")]
            reason = "Finished" if any(fin) else "All crashed" if all(crash) else "Time limit"
            print(f"\n{reason}")
            print(f"  Car 0 (Red):  Reward: {total[0]:.1f} | Progress: {info_dict['0']['progress']:.1%}")
            print(f"  Car 1 (Blue): Reward: {total[1]:.1f} | Progress: {info_dict['1']['progress']:.1%}")
            print(f"  Winner: {winner}")
            break
    sink.close()
    chosen = "1" if (not info_dict["0"]["finished"] and info_dict["1"]["finished"]) else "0"
    d = info_dict[chosen]
    return {"total_reward": total[int(chosen)], "progress": d["progress"], "finished": d["finished"],
            "crashed": d["crashed"], "speed": d["speed"], "placement": d.get("placement", None), "steps": step + 1}


def visualization_grid(video_paths, model_names, output_path="racing_grid.npy", padding=10):
    """visualization.py:413-471 over saved ``.npy`` frame stacks: four stacks into
    one 2 x 2 grid on white, a finished stack frozen on its last frame.
    ``model_names`` is accepted for the signature; no label is drawn."""
    if len(video_paths) != 4:
        raise ValueError("visualization_grid lays out exactly four stacks (2 x 2)")
    stacks = [np.load(p, mmap_mode="r") for p in video_paths]
    h, w = stacks[0].shape[1:3]
    for p, s in zip(video_paths, stacks):
        if s.ndim != 4 or s.shape[1:] != (h, w, 3) or s.dtype != np.uint8 or len(s) == 0:
            raise ValueError(f"{p}: need a non-empty uint8 [frames, {h}, {w}, 3] stack")
    total = max(len(s) for s in stacks)
    H, W = mosaic_shape(h, 2, 2, padding) if h == w else (h * 2 + padding * 3, w * 2 + padding * 3)
    sink = _Sink(output_path, W, H)
    for t in range(total):
        grid = np.full((H, W, 3), 255, dtype=np.uint8)
        for k, s in enumerate(stacks):
            top, left = padding + (k // 2) * (h + padding), padding + (k % 2) * (w + padding)
            grid[top:top + h, left:left + w] = s[min(t, len(s) - 1)]
        sink.write(grid)
    sink.close()
