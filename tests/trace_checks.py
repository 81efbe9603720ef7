"""What the trace tests share (tests/test_lap_events_gpu.py, tests/test_lattice_gpu.py): a case
(tests/lap_cases.py Case: state0, actions and the oracle's trace) run on a RacingVectorEnv step by
step, and its rows, last rows and final state compared with the trace BIT FOR BIT.  A failure
names the first step, env and field that differ.  The sum of the episode returns is compared to
1e-9 relative: a re-sort orders the envs of one bin by the arrival of the REWARD waves' atomics,
so the f64 partial sums are taken over other env sets (tests/test_steps_cross_gpu.py RET_REL).
"""
import numpy as np
import pytest
import torch

RET_REL = 1e-9
STATE = ("x", "y", "angle", "vx", "vy", "progress", "last_progress", "last_steering", "flags", "steps")


def inject(v, case):
    """The case's state into a freshly reset env, its episode tallies cleared."""
    st = case.state0
    v.set_state(**{k: st[k] for k in STATE})
    if "finished_step" in st:
        v.set_state(finished_step=st["finished_step"])
    v.set_state(env_flags=np.zeros(case.n, np.uint8), ep_return=np.zeros(case.n), ep_length=np.zeros(case.n, np.int32))
    v.episode_stats()


def _acts(case, lo=0, hi=None):
    return torch.from_numpy(case.trace["actions"][lo:hi]).cuda().contiguous()


def _rows(v, T):
    z = lambda name: torch.zeros((T,) + tuple(v.buf[name].shape), dtype=v.buf[name].dtype, device="cuda")  # noqa: E731
    return {k: z(n) for k, n in (("obs", "obs"), ("reward", "reward"), ("done", "done_f32"))}


def _per_step(v, case, hook=None):
    """K x step_device(full_info): step k's outputs, masks and info rows in row k."""
    acts = _acts(case)
    out = _rows(v, case.T)
    full = {k: torch.zeros((case.T,) + tuple(v.buf[k].shape), dtype=v.buf[k].dtype, device="cuda")
            for k in ("reward64", "terminated", "truncated", "info", "ep_done")}
    for k in range(case.T):
        if hook is not None:
            hook(k)
        v.step_device(acts[k], obs_out=out["obs"][k], reward_out=out["reward"][k], done_out=out["done"][k],
                      full_info=True)
        for name, t in full.items():
            t[k].copy_(v.buf[name])
    out.update(full)
    return out


def _first_diff(dev, ref):
    """(step, env, rows that differ) of the first row of dev [T, N, ...] that is not ref's, or None."""
    dev = dev.cpu().numpy() if isinstance(dev, torch.Tensor) else np.asarray(dev)
    assert dev.shape == ref.shape and dev.dtype == ref.dtype, (dev.shape, dev.dtype, ref.shape, ref.dtype)
    if np.array_equal(dev, ref):
        return None
    bad = (dev != ref).reshape(dev.shape[0], dev.shape[1], -1).any(2)
    k, e = (int(i) for i in np.argwhere(bad)[0])
    return k, e, int(bad.sum()), dev[k, e].tolist(), ref[k, e].tolist()


def _differs(fields, lo=0):
    """fields: (name, device rows, oracle rows).  Fail naming the FIRST step at which any of them
    differs, the env and the field (of the fields that differ at that step, the first listed)."""
    found = [(d[0], i, name, d) for i, (name, dev, ref) in enumerate(fields) if (d := _first_diff(dev, ref))]
    if found:
        _, _, name, (k, e, n_bad, dev_row, ref_row) = min(found, key=lambda f: f[:2])
        pytest.fail(f"{name}: step {lo + k}, env {e}: device {dev_row} != oracle {ref_row} ({n_bad} (step, env) "
                    f"rows of {name} differ; fields that differ: {[f[2] for f in found]})")


def _want(case, lo=0, hi=None):
    tr = case.trace
    sl = slice(lo, hi)
    info = tr["info"][sl]
    return dict(obs=tr["obs"][sl], reward=tr["reward64"][sl].astype(np.float32), done=tr["done"][sl].astype(np.float32),
                reward64=tr["reward64"][sl], terminated=tr["terminated"][sl].astype(np.uint8),
                truncated=tr["truncated"][sl].astype(np.uint8), ep_done=tr["done"][sl].astype(np.uint8),
                info=info[:, :, None, :] if case.n_agents == 1 else info)


def _check_rows(case, out):
    want = _want(case)
    names = ("terminated", "truncated", "done", "ep_done", "reward64", "reward", "info", "obs")
    _differs([(name, out[name], want[name]) for name in names if name in out])


def _check_last_rows(case, v, outputs=False):
    """The env's own rows, written at stride 0, hold the trace's last step: the info and mask rows,
    and with `outputs` (a call without row buffers) obs / reward / done too."""
    want = _want(case, case.T - 1, case.T)
    rows = (("reward64", "reward64"), ("terminated", "terminated"), ("truncated", "truncated"), ("ep_done", "ep_done"),
            ("info", "info"))
    if outputs:
        rows += (("obs", "obs"), ("reward", "reward"), ("done", "done_f32"))
    _differs([("last " + name, v.buf[buf][None], want[name]) for name, buf in rows], case.T - 1)


def _check_end(case, v):
    """The whole state, the episode counts and lengths (exact) and the return sum (RET_REL)."""
    g = v.get_state()
    for k, ref in case.final.items():
        if k == "track":  # slot ids: the env's own numbering (checked in _start)
            continue
        dev = g[k].reshape(ref.shape)
        if not np.array_equal(dev, ref):
            e = int(np.argwhere((dev != ref).reshape(case.n, -1).any(1))[0, 0])
            pytest.fail(f"state {k} after step {case.T - 1}: env {e}: device {dev[e].tolist()} != oracle "
                        f"{ref[e].tolist()}")
    ret, length, count = v.episode_stats()
    assert (length, count) == (case.stats[1], case.stats[2]), ((ret, length, count), case.stats)
    assert abs(ret - case.stats[0]) <= RET_REL * max(1.0, abs(case.stats[0])), (ret, case.stats[0])
