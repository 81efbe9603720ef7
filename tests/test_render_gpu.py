"""The three raster kernels (csrc/rx_render.hip) against their host twins, byte
for byte, and the Python layer above them on a real device.  The host twins
are themselves checked against an independent NumPy restatement in
tests/test_render_cpu.py.

Sizes 128 (rows of whole dwords: the frame kernel's three-dword stores) and 99
(not a multiple of 4 nor of the 16-pixel tile: the byte path and the row tail).
Mosaics: padding 4 at size 128 keeps every row 4-byte aligned (the dword path
through out_off / out_pitch); padding 10 and 3 do not (the byte path)."""
import numpy as np
import pytest
import torch

from rx import render
from rx.envs import MultiRacingEnv, RacingEnv
from rx.vector_env import RacingVectorEnv
from tests import raster_ref as R

pytestmark = pytest.mark.gpu

geoms = R.sample_geoms


def _pool():
    g = geoms()
    return [x.control_points for x in g], [x.track_width for x in g]


def _host_state(v):
    st = v.state
    return tuple(np.ascontiguousarray(st[k].cpu().numpy()) for k in ("x", "y", "angle"))


def _actions(rng, n, a):
    act = np.empty((n, a, 2), dtype=np.float32)
    act[..., 0] = rng.uniform(-1.0, 1.0, (n, a))
    act[..., 1] = rng.uniform(0.5, 1.0, (n, a))
    return act


# ---------------------------------------------------------------- 1. static layers
@pytest.mark.parametrize("size", (128, 99))
def test_device_static_layers_equal_host(size):
    dev = render.Canvas(list(geoms()), size, 2, backend="device", device="cuda")
    host = render.Canvas(list(geoms()), size, 2, backend="host")
    got = dev.layer.cpu().numpy()
    assert got.shape == (3, size, size)
    for k in range(3):
        assert np.array_equal(got[k], host.layer[k]), k
        assert (np.bincount(got[k].ravel(), minlength=4) >= 40).all()


# ---------------------------------------------------------------- 2., 3. episodes
def _run_episode(n_agents, n_envs, env_ids, size, steps, same_actions, min_trail=10):
    cps, widths = _pool()
    slot = [i % (2 if n_agents == 1 else 3) for i in range(n_envs)]  # single-agent: 2 tracks
    v = RacingVectorEnv([cps[s] for s in slot], [widths[s] for s in slot], n_agents=n_agents, device="cuda",
                        autoreset="disabled", seed=5)
    try:
        r = render.Renderer(v, env_ids=env_ids, size=size)
        host = render.Canvas([v.tracks.geoms[v.track_of_env[e]] for e in r.env_ids], size, n_agents, backend="host",
                             env_ids=r.env_ids)
        v.reset_device()
        r.begin()
        rng = np.random.default_rng(11)
        moved = 0
        for t in range(steps):
            act = _actions(rng, n_envs, 1 if same_actions else n_agents)
            if same_actions:
                act = np.repeat(act, n_agents, axis=1)
            v.step_device(torch.from_numpy(act).cuda())
            r.step()
            frames = r.frame()
            x, y, a = _host_state(v)
            host.add_points(x, y)
            want = host.compose(x, y, a)
            assert frames.shape == (len(r.env_ids), size, size, 3) and frames.dtype == torch.uint8
            assert np.array_equal(frames.cpu().numpy(), want), t
            moved = int(host.trail.astype(bool).sum())
        assert np.array_equal(r.canvas.trail.cpu().numpy(), host.trail)
        assert np.array_equal(r.canvas.last.cpu().numpy(), host.last)
        assert moved >= min_trail * len(r.env_ids)  # the cars drew paths: the comparison was not of empty layers
        return v, r, host
    except BaseException:
        v.close()
        raise


def test_single_agent_episode_equals_host():
    v, r, host = _run_episode(1, 8, [0, 3, 7], 128, 40, False)
    v.close()


def test_two_car_episode_equals_host():
    v, r, host = _run_episode(2, 4, None, 99, 60, True)
    try:
        assert (host.trail & 0x20).any() and (host.trail & 0x10).any()
    finally:
        v.close()


# ---------------------------------------------------------------- 4. mosaics; 6. begin()
@pytest.mark.parametrize("size,padding", ((99, 10), (99, 3), (128, 4)))
def test_device_mosaic_equals_pasted_frames(size, padding):
    v, r, host = _run_episode(2, 4, None, size, 12, False, min_trail=1)
    try:
        frames = r.frame().cpu().numpy()
        got = r.mosaic(2, 2, padding)
        H = W = 2 * size + 3 * padding
        assert tuple(got.shape) == (H, W, 3) and got.dtype == torch.uint8
        want = np.full((H, W, 3), 255, dtype=np.uint8)
        for k in range(4):
            top, left = padding + (k // 2) * (size + padding), padding + (k % 2) * (size + padding)
            want[top:top + size, left:left + size] = frames[k]
        assert np.array_equal(got.cpu().numpy(), want)
        x, y, a = _host_state(v)
        assert np.array_equal(host.mosaic(x, y, a, 2, 2, padding), want)
        # begin() after a reset clears the paths
        assert r.canvas.trail.any()
        v.reset_device()
        r.begin()
        assert not r.canvas.trail.any() and not r.canvas.last.any()
        host.begin()
        x, y, a = _host_state(v)
        assert np.array_equal(r.frame().cpu().numpy(), host.compose(x, y, a))
    finally:
        v.close()


# ---------------------------------------------------------------- 5. the Gymnasium surface
@pytest.mark.parametrize("two", (False, True))
def test_env_render_rgb_array(two):
    env = MultiRacingEnv(render_mode="rgb_array") if two else RacingEnv(render_mode="rgb_array")
    try:
        env.reset()
        S = 800
        host = render.Canvas([env._vec().tracks.geoms[0]], S, 2 if two else 1, backend="host")
        assert env.render().shape == (S, S, 3)
        for t in range(5):
            env.step({"0": np.array([0.3, 1.0]), "1": np.array([-0.2, 0.8])} if two else np.array([0.3, 1.0]))
            x, y, a = _host_state(env._vec())
            host.add_points(x, y)
        f = env.render()
        assert f.shape == (S, S, 3) and f.dtype == np.uint8
        want = host.compose(x, y, a)[0]
        v = host.views[0]
        ci, cj = render.convert_coords(x[0], y[0], v["offset_x"], v["offset_y"], v["scale"], S)
        i0, j0 = min(max(ci - 49, 0), S - 99), min(max(cj - 49, 0), S - 99)
        win = (slice(j0, j0 + 99), slice(i0, i0 + 99))
        assert (255, 0, 0) in {tuple(p) for p in f[win].reshape(-1, 3)}  # the window holds the car
        assert np.array_equal(f[win], want[win])
        assert np.array_equal(f, want)
        env.reset()  # a new path
        assert not env._renderer.canvas.trail.any()
    finally:
        env.close()


# ---------------------------------------------------------------- 7. what a Renderer refuses
def test_renderer_refuses_autoreset_envs_and_too_many_images():
    cps, widths = _pool()
    v = RacingVectorEnv(cps[:2], widths[:2], device="cuda", autoreset="next_step")
    try:
        with pytest.raises(ValueError, match="autoreset"):
            render.Renderer(v)
    finally:
        v.close()
    v = RacingVectorEnv(cps[:2], widths[:2], device="cuda", autoreset="disabled")
    try:
        with pytest.raises(ValueError, match="env_ids"):
            render.Renderer(v, env_ids=[0, 2])
        with pytest.raises(ValueError, match="1024"):
            render.Renderer(v, env_ids=[0, 1] * 513)
    finally:
        v.close()


# ---------------------------------------------------------------- the drop-ins of utils/visualization.py
def test_visualize_drop_ins_write_npy_stacks(tmp_path):
    from rx.agent import Agent
    from rx.visualize import visualize_multi_agent, visualize_single_agent
    torch.manual_seed(3)
    env = RacingEnv(num_sensors=7)
    agent = Agent(env.observation_space, env.action_space).to("cuda")
    try:
        path = str(tmp_path / "single.npy")
        res = visualize_single_agent(env, agent, "cuda", path, max_steps=9, size=64, every=4)
        assert set(res) == {"total_reward", "steps", "progress", "finished", "crashed", "speed"}
        frames = np.load(path)
        assert frames.shape == (3, 64, 64, 3) and frames.dtype == np.uint8 and res["steps"] == 9  # steps 0, 4, 8
        colours = {tuple(p) for p in frames[-1].reshape(-1, 3)}
        assert (255, 0, 0) in colours or (150, 0, 0) in colours  # at 64 pixels a car can be all outline
    finally:
        env.close()
    env = MultiRacingEnv(num_sensors=7)
    agent = Agent(env.observation_space["0"], env.action_space["0"]).to("cuda")
    try:
        path = str(tmp_path / "multi.npy")
        res = visualize_multi_agent(env, agent, "cuda", path, max_steps=6, size=64, every=2)
        assert set(res) == {"total_reward", "progress", "finished", "crashed", "speed", "placement", "steps"}
        frames = np.load(path)
        assert frames.shape == (3, 64, 64, 3)
        colours = {tuple(p) for p in frames[-1].reshape(-1, 3)}
        assert (255, 0, 0) in colours or (150, 0, 0) in colours
        assert (0, 0, 255) in colours or (0, 0, 150) in colours
    finally:
        env.close()
