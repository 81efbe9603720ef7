"""The track table built on the device (rx_build_tracks, csrc/rx_track.hip;
TrackSet backend="device") against its host twin (rx_build_tracks_host): the
same rx_spline.h code compiled for gfx950 and for the host, so wp / nrm / seg /
meta agree byte for byte -- except meta[:, 2], the platform's atan2 (ocml /
libm), held to 1e-14 rad of np.arctan2 (~20 ulp of pi: above any libm's error,
far below anything that moves a start pose).  Then the engine on such a table
against the oracle fed the same table, bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle.orc import multi_state, sensor_angles
from rx.track import DEFAULT_CONTROL_POINTS, DEFAULT_WIDTH, TrackSet, gen_tracks

pytestmark = pytest.mark.gpu

GUARD = 12345.0
KEYS = ("wp", "nrm", "seg", "meta")


def _pool193():
    np.random.seed(11)
    pool = gen_tracks(192, seed=None) + [DEFAULT_CONTROL_POINTS]  # 193: the last workgroup is partly empty
    return pool, [float(4 + k % 6) for k in range(193)]


def _circle(P, r=40.0):
    a = np.linspace(0, 2 * np.pi, P, endpoint=False)
    return np.column_stack([r * np.cos(a) + 3.0, r * np.sin(a) - 1.0])


def _flatten(cps, widths):
    cp_off = np.concatenate([[0], np.cumsum([len(c) for c in cps])]).astype(np.int32)
    cp = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64) for c in cps]))
    return cp_off, cp, np.asarray(widths, dtype=np.float64)


def _sizes(cp_off, factor):
    wt, n = int(cp_off[-1]) * factor, len(cp_off) - 1
    return dict(wp=2 * wt, nrm=2 * wt, seg=8 * wt, meta=8 * n)


def _host(cps, widths, factor):
    from rx import _lib
    L = _lib.load()
    cp_off, cp, w = _flatten(cps, widths)
    out = {k: np.full(s + 1, GUARD) for k, s in _sizes(cp_off, factor).items()}
    wp_off = np.zeros(len(cps) + 1, np.int32)
    _lib.check(L.rx_build_tracks_host(len(cps), factor, _lib.ptr(cp_off), _lib.ptr(cp), _lib.ptr(w), _lib.ptr(wp_off),
                                      *[_lib.ptr(out[k]) for k in KEYS], None), "rx_build_tracks_host")
    return wp_off, out


def _enqueue(cps, widths, factor):
    """Upload and enqueue one device build on torch's current stream; no host sync after the launch."""
    from rx import _lib
    L = _lib.load()
    cp_off, cp, w = _flatten(cps, widths)
    cp_d, w_d = torch.from_numpy(cp).cuda(), torch.from_numpy(w).cuda()
    out = {k: torch.full((s + 1,), GUARD, dtype=torch.float64, device="cuda") for k, s in _sizes(cp_off, factor).items()}
    wp_off = np.zeros(len(cps) + 1, np.int32)
    _lib.check(L.rx_build_tracks(len(cps), factor, _lib.ptr(cp_off), _lib.ptr(cp_d), _lib.ptr(w_d), _lib.ptr(wp_off),
                                 *[_lib.ptr(out[k]) for k in KEYS], _lib.stream_ptr()), "rx_build_tracks")
    return wp_off, out, (cp_d, w_d)


def _device(cps, widths, factor):
    wp_off, out, _ = _enqueue(cps, widths, factor)
    torch.cuda.synchronize()
    return wp_off, {k: v.cpu().numpy() for k, v in out.items()}


CASES = {
    "pool193": lambda: (*_pool193(), 30),
    "one": lambda: ([_pool193()[0][5]], [7.0], 30),
    "P3_factor1": lambda: ([_circle(3)], [5.0], 1),       # fewer waypoints than lanes
    "P64_factor2": lambda: ([_circle(64)], [5.0], 2),     # exactly two passes of the 64 lanes
    "mixed": lambda: ([_circle(3), _circle(64), _circle(11), _circle(5), _circle(7)], [1.0, 2.0, 0.0, 4.0, 9.5], 3),
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_host_twin(case):
    cps, widths, factor = CASES[case]()
    h_off, h = _host(cps, widths, factor)
    d_off, d = _device(cps, widths, factor)
    assert np.array_equal(h_off, d_off)
    n = len(cps)
    for k in KEYS:
        assert d[k][-1] == GUARD and h[k][-1] == GUARD, f"{k}: the element past the table was written"
        assert not np.any(d[k][:-1] == GUARD), f"{k}: an element of the table was not written"
    for k in ("wp", "nrm", "seg"):
        assert d[k].tobytes() == h[k].tobytes(), k
    dm, hm = d["meta"][:-1].reshape(n, 8), h["meta"][:-1].reshape(n, 8)
    cols = [0, 1, 3, 4, 5, 6, 7]
    assert dm[:, cols].tobytes() == hm[:, cols].tobytes()
    wp = d["wp"][:-1].reshape(-1, 2)
    s = d_off[:-1]
    want = np.arctan2(wp[s + 1, 1] - wp[s, 1], wp[s + 1, 0] - wp[s, 0])
    err_d, err_h = np.abs(dm[:, 2] - want).max(), np.abs(hm[:, 2] - want).max()
    print(f"{case}: max |meta[:, 2] - np.arctan2| device {err_d:.3e}, host {err_h:.3e}")
    assert err_d <= 1e-14 and err_h <= 1e-14
    assert np.array_equal(dm[:, 3], np.asarray(widths, dtype=np.float64)) and np.all(dm[:, 7] == 0.0)


def test_python_tables_are_byte_identical():
    pool, widths = _pool193()
    pool, widths = pool + pool[:9] + [None], widths + widths[:9] + [None]  # duplicates dedup the same way
    dev = TrackSet.build(pool, widths, backend="device")
    nat = TrackSet.build(pool, widths, backend="native")
    assert len(dev) == len(nat) == 194 and dev._index == nat._index
    assert dev.geoms[193].track_width == DEFAULT_WIDTH
    for k in ("wp_off", "wp", "nrm", "seg", "meta"):
        assert dev.arrays()[k].dtype == nat.arrays()[k].dtype and dev.arrays()[k].tobytes() == nat.arrays()[k].tobytes(), k
    # a slot added later comes from the host twin: still one table
    extra = _circle(9)
    assert dev.slot(extra, 5.0) == nat.slot(extra, 5.0) == 194
    assert dev.arrays()["wp"].tobytes() == nat.arrays()["wp"].tobytes()
    assert dev.arrays()["meta"].tobytes() == nat.arrays()["meta"].tobytes()


def test_device_marks_what_only_device_memory_shows():
    """A repeated control point cannot be seen by the host before the launch: the
    kernel marks the track (meta[4] = NaN, which rx_upload_tracks refuses) and
    the Python layer raises the host twin's message."""
    from rx import _lib
    good, rep = _circle(10), _circle(10)
    rep[4] = rep[3]
    _, d = _device([good, rep, good], [6.0, 6.0, -1.0], 30)
    m = d["meta"][:-1].reshape(3, 8)
    assert np.isfinite(m[0]).all() and np.isnan(m[1, 4]) and np.isnan(m[2, 4])
    with pytest.raises(_lib.RxError, match="track 1.*chord 3"):
        TrackSet.build([good, rep], [6.0, 6.0], backend="device")


def test_single_env_runs_on_a_device_built_table(oracle_dev):
    """128 envs on 128 distinct device-built tracks == the oracle fed the same
    table, bit for bit, 60 steps with next-step autoreset."""
    from rx.vector_env import RacingVectorEnv
    from tests.test_fullsize_gpu import _single_run
    np.random.seed(5)
    pool = gen_tracks(128, seed=None)
    widths = [np.random.randint(6, 10) for _ in range(128)]
    v = RacingVectorEnv(pool, widths, device="cuda", autoreset="next_step", track_backend="device")
    assert v.tracks.backend == "device" and len(v.tracks) == 128
    nat = TrackSet.build(pool, widths, backend="native").arrays()
    for k, a in v.tracks.arrays().items():
        assert a.tobytes() == nat[k].tobytes(), k
    _single_run(v, np.arange(128), oracle_dev, 60, seed=31, state_every=20)
    v.close()


def test_two_car_env_runs_on_a_device_built_table(oracle_dev):
    """32 two-car envs on 4 device-built tracks == the oracle, bit for bit, 30 steps
    (the start-slot order of a reset is drawn on the device: the oracle takes the
    order the device chose, as tests/test_fullsize_gpu.py does)."""
    from rx.vector_env import RacingVectorEnv
    from tests.test_fullsize_gpu import _actions, _oracle_table
    rel = sensor_angles(11, np.pi / 2)
    np.random.seed(6)
    four = gen_tracks(4, seed=None)
    N = 32
    pool, widths = [four[i % 4] for i in range(N)], [float(6 + i % 4) for i in range(N)]
    ts = TrackSet.build(pool, widths, backend="device")
    assert len(ts) == 4
    v = RacingVectorEnv(pool, widths, n_agents=2, device="cuda", autoreset="next_step", seed=9, track_set=ts)
    tab = _oracle_table(v)
    st = multi_state(N)
    st["track"][:] = v.track_of_env

    def oracle_reset(mask):
        dx = v.get_state()["x"].reshape(N, 2)
        keep = {k: val.copy() for k, val in st.items()}
        outs = []
        for first in (0, 1):
            for k in st:
                st[k][...] = keep[k]
            o = oracle_dev.multi_reset(tab, st, first, rel, mask=mask)
            outs.append((o, {k: val.copy() for k, val in st.items()}))
        pick = np.where(np.all(outs[0][1]["x"] == dx, axis=1), 0, 1)
        assert (np.all(outs[1][1]["x"] == dx, axis=1) | (pick == 0))[mask].all(), "start slots are neither order"
        for k in st:
            v0, v1 = outs[0][1][k], outs[1][1][k]
            st[k][...] = np.where(pick.reshape((-1,) + (1,) * (v0.ndim - 1)) == 0, v0, v1)
        return np.where(pick[:, None, None] == 0, outs[0][0], outs[1][0])

    obs = v.reset_device().cpu().numpy()
    assert np.array_equal(obs, oracle_reset(np.ones(N, bool)))
    rng = np.random.default_rng(13)
    pending = np.zeros(N, bool)
    for t in range(30):
        a = _actions(rng, N, 2)
        obs, rew, done = v.step_device(torch.from_numpy(a).cuda())
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool)
        o_obs, o_rew, _, o_done, _, _, _ = oracle_dev.multi_step(tab, st, a, rel)
        if pending.any():
            r_obs = oracle_reset(pending)
            o_obs[pending], o_rew[pending], o_done[pending] = r_obs[pending], 0.0, False
        assert np.array_equal(obs, o_obs), t
        assert np.array_equal(rew, o_rew.astype(np.float32)), t
        assert np.array_equal(done, o_done), t
        pending = o_done.copy()
    g = v.get_state()
    for k in ("x", "y", "angle", "vx", "vy", "progress", "flags", "finished_step"):
        assert np.array_equal(g[k].reshape(N, 2), st[k]), k
    v.close()


def test_two_builds_back_to_back_on_a_side_stream():
    """No host synchronisation between two builds enqueued on a non-default
    stream: the same bytes as two separate, synchronised builds."""
    pool, widths = _pool193()
    a, b = (pool[:96], widths[:96], 30), (pool[96:], widths[96:], 30)
    ref_a, ref_b = _device(*a), _device(*b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off_a, out_a, keep_a = _enqueue(*a)
        off_b, out_b, keep_b = _enqueue(*b)
        s.synchronize()
        got_a = {k: t.cpu().numpy() for k, t in out_a.items()}
        got_b = {k: t.cpu().numpy() for k, t in out_b.items()}
    assert np.array_equal(off_a, ref_a[0]) and np.array_equal(off_b, ref_b[0])
    for k in KEYS:
        assert got_a[k].tobytes() == ref_a[1][k].tobytes(), k
        assert got_b[k].tobytes() == ref_b[1][k].tobytes(), k
