"""Positions regrouped by slot on the GPU: rx_regroup_plan against its host twin byte for byte;
a regrouped env against its untouched twin env through the episodic rollout, steps_device and
captured graphs; the handle refusals; and the episodic trainers with episodic_regroup_every 1
against 0.  Everything compared is an integer or a bit pattern, and the reference of the env
tests is the path without a regroup, which tests/test_track_episodic_gpu.py pins to the oracle.

Every device output buffer of the kernel test carries a guard element past its end.
"""
import random

import numpy as np
import pytest
import torch

from tests.test_track_episodic_gpu import GUARD, LANE, LANE_SMALL, NAMES, _agent, _bufs, _dev, _guarded, _pool
from tests.test_track_regroup_cpu import OUTS, PATTERNS, SIZES, TRACKS, case, host_plan, py_regroup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


# ---------------------------------------------------------------- 1. kernel == host twin
def _kernel_case(L, n, n_tracks, name):
    from rx import _lib
    perm, pos_slot = case(name, n, n_tracks)
    rc, want = host_plan(L, n, n_tracks, perm, pos_slot)
    assert rc == 0, L.rx_last_error()
    d_in = {"perm": _guarded(perm), "pos_slot": _guarded(pos_slot)}
    d_out = {k: _guarded(np.full(n, -5, dtype=np.int32)) for k in OUTS}
    need = L.rx_regroup_scratch_bytes(n, n_tracks)
    assert need > 0 and need % 4 == 0
    scratch = torch.full((need // 4 + 1,), GUARD, dtype=torch.int32, device="cuda")
    rc = L.rx_regroup_plan(n, n_tracks, _lib.ptr(d_in["perm"]), _lib.ptr(d_in["pos_slot"]),
                           *(_lib.ptr(d_out[k]) for k in OUTS), _lib.ptr(scratch), need, _lib.stream_ptr())
    assert rc == 0, L.rx_last_error()
    torch.cuda.synchronize()
    for k in OUTS:
        got = d_out[k].cpu().numpy()
        assert got[n] == GUARD, f"guard of {k} ({n}, {n_tracks}, {name})"
        assert got[:n].tobytes() == want[k].tobytes(), (n, n_tracks, name, k)
    assert int(scratch[-1].item()) == GUARD, "guard of the scratch"
    for k, host in (("perm", perm), ("pos_slot", pos_slot)):
        assert np.array_equal(d_in[k].cpu().numpy(), np.append(host, GUARD)), f"input {k} was written"
    return want


@pytest.mark.parametrize("n_tracks", TRACKS)
def test_plan_kernel_equals_host_twin(L, n_tracks):
    """The grid of the CPU test: 9 sizes x 6 key patterns at this slot count (1 slot: no pass; up to 256:
    one digit; 257: two; 65,537: three)."""
    for n in SIZES:
        for name in PATTERNS:
            _kernel_case(L, n, n_tracks, name)


@pytest.mark.parametrize("n_tracks", [65537, 1])
def test_plan_kernel_equals_host_twin_at_70001_positions(L, n_tracks):
    """274 tiles: a count table of 70,144 entries, more than one entry per scanning thread; with 65,537
    slots the third digit decides, with one slot the order stays."""
    n = 70001
    for name in ("random", "sparse", "reversed"):
        want = _kernel_case(L, n, n_tracks, name)
        perm, pos_slot = case(name, n, n_tracks)
        ref = py_regroup(perm, pos_slot)
        for k in OUTS:
            assert want[k].tobytes() == ref[k].tobytes(), k
    if n_tracks == 1:
        assert np.array_equal(want["src"], np.arange(n))
    else:
        assert case("sparse", n, n_tracks)[1].max() == 65536


# ---------------------------------------------------------------- 2-4. the regroup is invisible
N_SLOTS = 16


class _Run:
    """One env on a 16-slot pool with max_steps = 3 (every env ends episodes), a TrackCurriculum whose
    table is not uniform, and an EpisodicStepRollout of T steps on the given noise."""

    def __init__(self, N, sched, T=8, seed=13):
        from rx.curriculum import TrackCurriculum
        from rx.track_episodic import EpisodicStepRollout
        from rx.vector_env import RacingVectorEnv
        pool, widths = _pool(N_SLOTS, 5)
        cps, ws = [pool[i % N_SLOTS] for i in range(N)], [widths[i % N_SLOTS] for i in range(N)]
        self.ag, self.fl = _agent()
        self.venv = RacingVectorEnv(cps, ws, device="cuda", max_steps=3, seed=seed, sched=sched)
        assert self.venv.schedule()["lane_tracks"] == 1
        self.cur = TrackCurriculum(self.venv, seed=3, mix=0.3)
        self.cur.tally[:, 1] = torch.arange(N_SLOTS, device="cuda") % 5
        self.cur.tally[:, 0] = 6
        self.cur.scores()
        self.bufs = _bufs(self.venv, T)
        self.sr = EpisodicStepRollout(self.ag, self.fl, self.venv, T, self.cur, record_slots=True)

    def rollout(self, eps):
        self.bufs[0][0].copy_(self.bufs[6])  # the carried next_obs / next_done open the next rollout
        self.bufs[3][0].copy_(self.bufs[7])
        self.sr(*self.bufs, eps=eps)

    def snapshot(self):
        torch.cuda.synchronize()
        out = {k: x.clone() for k, x in zip(NAMES, self.bufs)}
        out.update(tally=self.cur.tally.clone(), track=self.venv._st["track"].clone(), draws=self.cur.draws.clone(),
                   slots=self.sr.slots.clone())
        for k, v in self.venv.get_state().items():
            out["state_" + k] = torch.from_numpy(v.copy())
        out["ep_stats"] = torch.tensor(self.venv.episode_stats(reset=False), dtype=torch.float64)
        return out

    def close(self):
        self.venv.close()


def _noise(T, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((T, N, 2), device="cuda", generator=g) * 1.5


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _sorted(pos_slot):
    return bool((np.diff(pos_slot) >= 0).all())


@pytest.mark.parametrize("N,sched", [(4160, LANE), (200, LANE_SMALL)])
def test_a_regrouped_env_runs_as_its_untouched_twin(L, N, sched):
    """Two envs from the same seed run EpisodicStepRollout for 8 steps on the same noise, one is regrouped,
    both run 8 more: every rollout buffer, tally, track, draws, the recorded slots, get_state() and
    episode_stats() are equal bit for bit.  On the regrouped env lane_layout() is the host twin applied to
    the layout downloaded just before, pos_slot is non-decreasing and is track_ids()[perm], and env_pos is
    the inverse of perm.  Not vacuous: the draws of the first 8 steps left the layout out of slot order."""
    a, b = _Run(N, sched), _Run(N, sched)
    e0, e1 = _noise(8, N, 6), _noise(8, N, 7)
    for r in (a, b):
        r.rollout(e0)
    _same(a.snapshot(), b.snapshot())
    perm0, slot0, pos0 = b.venv.lane_layout()
    assert not _sorted(slot0), "the episodic draws moved envs off their slots' positions"
    assert np.array_equal(slot0, b.venv.track_ids()[perm0]) and np.array_equal(pos0[perm0], np.arange(N))
    assert b.venv.regroups == 0
    b.venv.regroup_slots()
    assert b.venv.regroups == 1 and a.venv.regroups == 0
    rc, want = host_plan(L, N, N_SLOTS, perm0, slot0)
    assert rc == 0
    perm1, slot1, pos1 = b.venv.lane_layout()
    assert perm1.tobytes() == want["perm"].tobytes() and slot1.tobytes() == want["pos_slot"].tobytes()
    assert pos1.tobytes() == want["env_pos"].tobytes()
    assert _sorted(slot1) and np.array_equal(slot1, b.venv.track_ids()[perm1])
    assert np.array_equal(pos1[perm1], np.arange(N)) and not np.array_equal(perm1, perm0)
    for x, y in zip(a.venv.lane_layout(), (perm0, slot0, pos0)):
        assert np.array_equal(x, y), "the twin env's layout stays"
    _same(a.snapshot(), b.snapshot())  # the move itself changed nothing in env order
    for r in (a, b):
        r.rollout(e1)
    sa, sb = a.snapshot(), b.snapshot()
    _same(sa, sb)
    ends = int(sa["dones"].sum().item() + sa["next_done"].sum().item())
    assert ends >= N, "episodes ended after the regroup as well"
    perm2, slot2, pos2 = b.venv.lane_layout()
    assert np.array_equal(perm2, perm1) and np.array_equal(pos2, pos1), "only a regroup moves positions"
    assert np.array_equal(slot2, b.venv.track_ids()[perm2]) and not _sorted(slot2)
    a.close()
    b.close()


def test_steps_device_after_a_regroup(L):
    """After a regroup, 24 steps of steps_device (the paired lane-varying launches and their snapshots, which
    are indexed by position) from a device action bank equal the same steps on the untouched twin env."""
    N, K = 4160, 24
    a, b = _Run(N, LANE), _Run(N, LANE)
    e0 = _noise(8, N, 6)
    for r in (a, b):
        r.rollout(e0)
    b.venv.regroup_slots()
    assert _sorted(b.venv.lane_layout()[1]) and not _sorted(a.venv.lane_layout()[1])
    g = torch.Generator(device="cuda").manual_seed(11)
    act = torch.rand((K, N, 2), device="cuda", generator=g) * torch.tensor([2.0, 0.7], device="cuda") + \
        torch.tensor([-1.0, 0.3], device="cuda")
    act = act.contiguous()
    outs = []
    for r in (a, b):
        obs = torch.zeros((K, N, 15), device="cuda")
        rew, done = torch.zeros((K, N), device="cuda"), torch.zeros((K, N), device="cuda")
        r.venv.steps_device(act, obs_out=obs, reward_out=rew, done_out=done, full_info=True)
        torch.cuda.synchronize()
        st = {k: torch.from_numpy(v.copy()) for k, v in r.venv.get_state().items()}
        outs.append(dict(obs=obs, rew=rew, done=done, info=r.venv.buf["info"].clone(),
                         terminated=r.venv.buf["terminated"].clone(), **st))
    _same(*outs)
    assert outs[0]["done"].sum().item() >= N, "episodes ended (max_steps = 3)"
    a.close()
    b.close()


def test_graphs_across_and_around_a_regroup(L):
    """(1) A rollout graph captured before a regroup and replayed after it equals the eager call: no buffer
    the graph reads moved.  (2) A captured graph of [rollout, regroup] replayed twice equals two eager rounds,
    the layouts included (the plan's order is a function of its input, not of arrival)."""
    N, T = 200, 4
    eps = _noise(T, N, 2)
    snaps, layouts = {}, {}
    for mode in ("eager", "rollout_graph", "round_graph"):
        r = _Run(N, LANE_SMALL, T=T)

        def body(r=r, mode=mode):
            r.rollout(eps)
            if mode == "round_graph":
                r.venv.regroup_slots()
        if mode != "eager":
            torch.cuda.synchronize()
            cg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cg, capture_error_mode="thread_local"):
                body()
            assert not r.cur.draws.any(), "the capture records, it runs nothing"
        for _ in range(2):
            if mode == "eager":
                body()
                r.venv.regroup_slots()
            elif mode == "rollout_graph":
                cg.replay()
                r.venv._launched()
                r.venv.regroup_slots()
            else:
                cg.replay()
                r.venv._launched()
        snaps[mode] = r.snapshot()
        layouts[mode] = r.venv.lane_layout()
        r.close()
    for mode in ("rollout_graph", "round_graph"):
        _same(snaps["eager"], snaps[mode])
        for x, y in zip(layouts["eager"], layouts[mode]):
            assert np.array_equal(x, y), mode
    assert _sorted(layouts["eager"][1])
    assert int(snaps["eager"]["draws"].sum().item()) >= N


# ---------------------------------------------------------------- 5. handle refusals
def test_refusals_that_need_a_handle(L):
    from rx import _lib
    from rx.vector_env import RacingVectorEnv
    pool, widths = _pool(4, 2)
    cps, ws = [pool[i % 4] for i in range(130)], [widths[i % 4] for i in range(130)]
    out = [np.zeros(130, np.int32) for _ in range(3)]
    seen = []
    # a grouped single-agent handle
    v = RacingVectorEnv(cps, ws, device="cuda", sched=dict(wide_n=-1, dyn_lpe=1, lane_tracks=-1))
    assert v.schedule()["lane_tracks"] == 0
    with pytest.raises(_lib.RxError, match="rx_regroup_slots.*not lane-varying"):
        v.regroup_slots()
    with pytest.raises(_lib.RxError, match="rx_lane_layout.*not lane-varying"):
        v.lane_layout()
    assert L.rx_regroup_slots(v._h, None) == _lib.RX_EINVAL
    seen.append(L.rx_last_error().decode())
    assert v.regroups == 0
    v.close()
    # a two-car handle
    v2 = RacingVectorEnv(cps, ws, n_agents=2, device="cuda")
    assert L.rx_regroup_slots(v2._h, None) == _lib.RX_EINVAL and b"two-car" in L.rx_last_error()
    seen.append(L.rx_last_error().decode())
    assert L.rx_lane_layout(v2._h, *(o.ctypes.data for o in out)) == _lib.RX_EINVAL and b"two-car" in L.rx_last_error()
    v2.close()
    # a handle whose assignment a new track table has voided: before rx_assign
    v = RacingVectorEnv(cps, ws, device="cuda", sched=LANE_SMALL)
    assert v.schedule()["lane_tracks"] == 1
    v.regroup_slots()  # accepted as it stands
    assert L.rx_lane_layout(v._h, None, out[1].ctypes.data, out[2].ctypes.data) == _lib.RX_EINVAL
    assert b"null perm_out" in L.rx_last_error()
    torch.cuda.synchronize()
    v._upload_tracks()
    assert L.rx_regroup_slots(v._h, None) == _lib.RX_ESTATE and b"rx_assign" in L.rx_last_error()
    seen.append(L.rx_last_error().decode())
    assert L.rx_lane_layout(v._h, *(o.ctypes.data for o in out)) == _lib.RX_ESTATE
    v.close()
    assert len(set(seen)) == 3


# ---------------------------------------------------------------- 6. trainers
def _train(monkeypatch, cls_name, regroup_every):
    from rx import track_episodic
    from rx.configs import base_config
    from rx.envs import RacingEnv
    if cls_name == "EpisodicCurriculumPPO":
        cls, extra = track_episodic.EpisodicCurriculumPPO, dict(episodic_slots=True)
    else:
        from rx.track_replay_episodic import EpisodicReplayCurriculumPPO as cls
        extra = dict(replay_alpha=0.5, replay_power=2)
    config = base_config(num_envs=4160, num_steps=16, kl_target=1e9, update_epochs=1, track_resample_every=1,
                         curriculum_refresh=0.0, episodic_regroup_every=regroup_every, **extra)
    config["total_timesteps"] = 3 * config["batch_size"]
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    pool, widths = _pool(64, 21)
    t = cls(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 64, track_width=widths[i % 64]), config,
            device="cuda")
    assert t.envs.schedule()["lane_tracks"] == 1 and t.regroup_every == regroup_every
    starts, collect, slots = [], t.collect_rollout, []

    def recording(*a):
        pre = t.envs.regroups
        out = collect(*a)
        slots.append(t.slots().clone())
        starts.append(t.envs.regroups - pre)
        return out
    regroup, after = t.envs.regroup_slots, []

    def regrouping(*a, **kw):
        before = t.envs.lane_layout()[1]
        regroup(*a, **kw)
        after.append((_sorted(before), _sorted(t.envs.lane_layout()[1])))
    monkeypatch.setattr(t.envs, "regroup_slots", regrouping)
    t.collect_rollout = recording
    assert [u for u, _, _, _ in t.train_iter()] == [0, 1, 2]
    torch.cuda.synchronize()
    res = dict(params=[p.detach().clone() for p in t.agent.parameters()], tally=t.curriculum.tally.clone(),
               draws=t.curriculum.draws.clone(), slots=slots, track=t.envs._st["track"].clone(),
               regroups=t.envs.regroups, starts=starts, after=after, grouped_at_end=_sorted(t.envs.lane_layout()[1]))
    if hasattr(t, "replay"):
        res["score"], res["seen"] = t.replay.score.clone(), t.replay.seen.clone()
    t.envs.close()
    return res


@pytest.mark.parametrize("cls_name", ["EpisodicCurriculumPPO", "EpisodicReplayCurriculumPPO"])
def test_trainer_with_regroups_equals_the_trainer_without(L, monkeypatch, cls_name):
    """3 updates at 4,160 envs x 16 steps on a 64-slot pool, max_steps = 12, episodic_regroup_every 1 against 0:
    parameters, tallies, draws and the slots of every rollout are equal bit for bit.  The regroup ran before
    the rollouts of updates 1 and 2 and of no other (venv.regroups == 2), found the layout out of slot order
    and left pos_slot non-decreasing for the rollout."""
    from rx import track_episodic
    build = track_episodic.build_vector_env
    monkeypatch.setattr(track_episodic, "build_vector_env", lambda *a, **kw: build(*a, max_steps=12, **kw))
    off, on = _train(monkeypatch, cls_name, 0), _train(monkeypatch, cls_name, 1)
    assert off["regroups"] == 0 and off["starts"] == [0, 0, 0] and off["after"] == []
    assert on["regroups"] == 2 and on["starts"] == [0, 1, 1]
    assert on["after"] == [(False, True), (False, True)]
    assert not off["grouped_at_end"]
    for k in ("tally", "draws", "track") + (("score", "seen") if "score" in on else ()):
        assert torch.equal(off[k], on[k]), k
    for u, (x, y) in enumerate(zip(off["slots"], on["slots"])):
        assert torch.equal(x, y), f"slots of update {u}"
    for i, (x, y) in enumerate(zip(off["params"], on["params"])):
        assert torch.equal(x, y), f"parameter {i}"
    assert int(on["draws"].sum().item()) >= 2 * 4160
