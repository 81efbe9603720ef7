"""The refusals of the step-loop entry points that need a real handle: rx_rollout,
rx_rollout_steps, rx_track_rollout_steps, rx_selfplay_rollout_steps,
rx_league_rollout_steps, rx_eval_steps and rx_match_steps on a single-agent handle, a
two-car handle and a handle that was created but never assigned.  Per row: the return
code (RX_ESTATE / RX_EINVAL differ between the entry points; they are ABI) and a word
of rx_last_error.  Every row returns before any HIP call; all the same every pointer
in every struct is a real device buffer of the right size.  A valid rx_rollout_steps
on the same handle afterwards shows that the refusals left no state behind."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N, T, DEV = 8, 2, "cuda"
ROLLOUT_BUFS = ("params", "log_std", "eps", "obs", "actions", "logprobs", "values", "rewards", "dones", "next_obs",
                "next_done")
SELFPLAY_BUFS = ("opp_params", "opp_log_std", "opp_eps", "env_actions", "env_obs", "env_reward", "sink")


class Ctx:
    def __init__(self):
        from rx import _lib
        from rx.evaluate import eval_pool
        from rx.vector_env import RacingVectorEnv
        self.lib, self.L = _lib, _lib.load()
        cps, ws, _ = eval_pool(num_tracks=N, num_runs=1)  # 8 envs on 8 tracks
        self.one = RacingVectorEnv(cps, ws, n_agents=1, device=DEV, seed=3)
        self.two = RacingVectorEnv(cps, ws, n_agents=2, device=DEV, seed=3)
        cfg = _lib.RxConfig(N, 1, 11, 3000, 0, 0, 3, 3.141592653589793 / 3, 8.0, 8, 16, 2, 8)
        self.raw = _lib._P()
        _lib.check(self.L.rx_create(cfg, self.raw), "rx_create")
        self.handles = {"one": self.one._h, "two": self.two._h, "raw": self.raw}
        self.keep = []  # the tensors behind the structs' pointers
        z = self.z
        self.rollout = {D: self.rollout_io(D) for D in (15, 19)}
        stride = (int(self.L.rx_ppo_n_params(19)) + 63) // 64 * 64
        p = _lib.ptr
        self.act2 = z(N, 2, 2)
        b = self.two.buf
        self.sp = _lib.RxSelfplayIO(p(z(stride)), p(z(2)), p(z(T, N, 2)), p(self.act2), p(b["obs"]), p(b["reward"]),
                                    p(z(2 * N)), 0, 0)
        self.lg = _lib.RxLeagueIO(3, 0, p(z(3, stride)), p(z(3, 2)), stride, p(z(N, dtype=torch.int32)),
                                  p(z(N, dtype=torch.int32)), p(z(3, 3, dtype=torch.int64)),
                                  p(z(3, dtype=torch.float64).fill_(1.0)), 5, 0)
        self.tc = _lib.RxTrackIO(N, 0, p(self.one._st["track"]), p(z(N, 4, dtype=torch.int64)),
                                 p(z(N, dtype=torch.int64)), p(z(N, dtype=torch.float64)), p(z(N, dtype=torch.int32)),
                                 5)
        rec = (p(z(T, N, 2)), p(z(T, N, 1, 2)), p(z(N)), p(z(N)), p(z(N, 1, _lib.RX_EVAL_W, dtype=torch.float64)),
               p(z(N, dtype=torch.uint8)), p(z(1, dtype=torch.int32)))
        self.ev = _lib.RxEvalIO(15, 0, p(z(stride)), p(z(2)), *rec)
        self.m = _lib.RxMatchIO(15, 0, p(z(3, stride)), p(z(3, 2)), *rec, 3, 0, stride, p(z(N, 1, dtype=torch.int32)))

    def z(self, *shape, dtype=torch.float32):
        t = torch.zeros(shape, dtype=dtype, device=DEV)
        self.keep.append(t)
        return t

    def rollout_io(self, D):
        z, p = self.z, self.lib.ptr
        t = {"params": z(int(self.L.rx_ppo_n_params(D))), "log_std": z(2), "eps": z(T, N, 2), "obs": z(T, N, D),
             "actions": z(T, N, 2), "logprobs": z(T, N), "values": z(T, N), "rewards": z(T, N), "dones": z(T, N),
             "next_obs": z(N, D), "next_done": z(N)}
        return self.lib.RxRolloutIO(T, D, *(p(t[k]) for k in ROLLOUT_BUFS)), t

    def io(self, venv, full=False, info=False):
        base = venv._io(full=full)
        io = self.lib.RxIO(*(getattr(base, k) for k in self.lib.IO_FIELDS))
        if info:
            io.info = self.lib.ptr(venv.buf["info"])
        return io

    def call(self, fn, handle, changes):
        """``fn`` on ``handle`` with valid arguments for the handle the entry point wants, then
        ``changes``: ((struct.field or "precision", value), ...)."""
        copy = lambda s: type(s).from_buffer_copy(s)  # noqa: E731
        two_car = fn in ("rx_selfplay_rollout_steps", "rx_league_rollout_steps")
        venv = self.two if two_car else self.one
        a = {"io": self.io(venv, full=fn in ("rx_eval_steps", "rx_match_steps"),
                           info=fn in ("rx_track_rollout_steps", "rx_league_rollout_steps")),
             "r": copy(self.rollout[19 if two_car else 15][0]), "sp": copy(self.sp), "lg": copy(self.lg),
             "tc": copy(self.tc), "ev": copy(self.ev), "m": copy(self.m), "precision": 0}
        for path, value in changes:
            if "." in path:
                s, field = path.split(".")
                setattr(a[s], field, value)
            else:
                a[path] = value
        h, s, ref = self.handles[handle], self.lib.stream_ptr(None), ctypes.byref
        order = {"rx_rollout": ("io", "r"), "rx_rollout_steps": ("io", "r", "precision"),
                 "rx_track_rollout_steps": ("io", "r", "tc", "precision"),
                 "rx_selfplay_rollout_steps": ("io", "r", "sp", "precision"),
                 "rx_league_rollout_steps": ("io", "r", "sp", "lg", "precision"),
                 "rx_eval_steps": ("io", "ev", "n_steps"), "rx_match_steps": ("io", "m", "n_steps")}[fn]
        a["n_steps"] = T
        args = [a[k] if isinstance(a[k], int) else ref(a[k]) for k in order]
        return getattr(self.L, fn)(h, *args, s)

    def close(self):
        self.one.close()
        self.two.close()
        self.L.rx_destroy(self.raw)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def _rows():
    """(entry point, handle, changes, return code, word of rx_last_error); the codes are those of the
    entry points before their loops were merged."""
    E, S = "RX_EINVAL", "RX_ESTATE"
    rows = []
    add = lambda *r: rows.append(r)  # noqa: E731
    # a handle that was never assigned: RX_ESTATE, but RX_EINVAL from the track and league entry points
    for fn, code in (("rx_rollout", S), ("rx_rollout_steps", S), ("rx_track_rollout_steps", E),
                     ("rx_selfplay_rollout_steps", S), ("rx_league_rollout_steps", E), ("rx_eval_steps", S),
                     ("rx_match_steps", S)):
        add(fn, "raw", (), code, "assigned")
    # the wrong number of cars
    add("rx_rollout", "two", (), S, "single-agent")
    add("rx_rollout_steps", "two", (), E, "single-agent")
    add("rx_track_rollout_steps", "two", (), E, "single-agent")
    add("rx_selfplay_rollout_steps", "one", (), E, "two-car")
    add("rx_league_rollout_steps", "one", (), E, "two-car")
    # the rollout io
    for fn, h in (("rx_rollout", "one"), ("rx_rollout_steps", "one"), ("rx_track_rollout_steps", "one"),
                  ("rx_selfplay_rollout_steps", "two"), ("rx_league_rollout_steps", "two")):
        for bad in (0, -1):
            add(fn, h, (("r.T", bad),), E, "T=")
        add(fn, h, (("r.obs_dim", 17),), E, "obs_dim")
        for k in ROLLOUT_BUFS if fn == "rx_rollout_steps" else ("eps", "next_done"):
            add(fn, h, ((f"r.{k}", None),), E, "null")
        if fn != "rx_rollout":
            add(fn, h, (("precision", 7),), E, "precision")
    # the self-play io
    for k in SELFPLAY_BUFS:
        add("rx_selfplay_rollout_steps", "two", ((f"sp.{k}", None),), E, "null")
    for k in SELFPLAY_BUFS[2:]:  # the league form takes the opponents' parameters from the bank
        add("rx_league_rollout_steps", "two", ((f"sp.{k}", None),), E, k)
    for bad in (-1, 2):
        add("rx_selfplay_rollout_steps", "two", (("sp.agent", bad),), E, "agent")
    add("rx_selfplay_rollout_steps", "two", (("sp.opp_precision", 7),), E, "precision")
    add("rx_league_rollout_steps", "two", (("sp.agent", 1),), E, "agent")
    add("rx_league_rollout_steps", "two", (("sp.agent", 1), ("r.eps", None)), E, "agent")  # the earlier check wins
    add("rx_selfplay_rollout_steps", "two", (("sp.agent", 2), ("r.eps", None)), E, "agent")
    add("rx_selfplay_rollout_steps", "two", (("r.T", 0), ("sp.agent", 2)), E, "T=")
    # the io rows a tally reads
    add("rx_track_rollout_steps", "one", (("io.info", None),), E, "info")
    add("rx_track_rollout_steps", "one", (("io.terminated", None),), E, "terminated")
    add("rx_league_rollout_steps", "two", (("io.info", None),), E, "info")
    # the evaluation loops: the width is compared with the handle's
    add("rx_eval_steps", "one", (("ev.obs_dim", 19),), E, "obs_dim")
    add("rx_match_steps", "one", (("m.obs_dim", 19),), E, "obs_dim")
    return rows


ROWS = _rows()


def test_every_refusal_has_its_code_and_names_the_function_and_the_field(ctx):
    assert ctx.L.rx_rollout_supported(ctx.one._h) == 1  # or rx_rollout's rows below would all be RX_ESTATE
    for fn, handle, changes, code, word in ROWS:
        rc = ctx.call(fn, handle, changes)
        err = ctx.L.rx_last_error().decode()
        print(f"{fn} [{handle}] {changes}: rc={rc} {err!r}")
        assert rc == getattr(ctx.lib, code), (fn, handle, changes, rc, err)
        assert fn in err and word in err, (fn, handle, changes, word, err)
    # nothing was enqueued and nothing was left behind: a valid rollout on the same handle
    _, t = ctx.rollout[15]
    t["obs"][0].copy_(ctx.one.reset_device())
    for k in ("actions", "logprobs", "values", "rewards", "next_obs", "next_done"):
        t[k].fill_(float("nan"))
    t["eps"].normal_()
    ctx.lib.check(ctx.call("rx_rollout_steps", "one", ()), "rx_rollout_steps")
    ctx.one._launched(None)
    torch.cuda.synchronize()
    for k in ("actions", "logprobs", "values", "rewards", "next_obs", "next_done"):
        assert torch.isfinite(t[k]).all(), k
