"""The curriculum's replay scores on the GPU: each kernel (csrc/rx_track_replay.hip)
against its host twin bit for bit, and ReplayCurriculumPPO against a torch
restatement of its scores, against CurriculumPPO before the first redraw, and
against itself.

Every device output buffer carries a guard element past its end.
"""
import ctypes
import random

import numpy as np
import pytest
import torch

from tests.test_track_replay_cpu import adv_case, host_draw, host_tables, learn_io, score_case

pytestmark = pytest.mark.gpu

GUARD = -77


@pytest.fixture(scope="module")
def L():
    from rx import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- 1. the tally
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("mode", ["one_slot", "distinct", "none", "random"])
@pytest.mark.parametrize("T,n", [(1, 1), (3, 63), (2, 64), (5, 65), (7, 257), (129, 4097)])
def test_tally_kernel_equals_host_twin(L, T, n, mode, kind):
    """One lane, a partial wave, an exact wave, a wave plus a lane, a workgroup plus a lane, and several
    row chunks x 17 env blocks.  one_slot: every lane of every wave adds to ONE row (the sums must be exact);
    distinct: every lane of a wave on another slot (67 slots); none: nothing is inside the table."""
    from rx import _lib
    n_tracks = 67
    track, adv = adv_case(T, n, n_tracks, 100 + n, mode)
    start = np.random.RandomState(n).randint(0, 1000, size=(n_tracks + 1, 2)).astype(np.int64)
    want = start.copy()
    lt = learn_io(_lib, n_tracks, kind, track=track, learn=want)
    assert L.rx_track_learn_tally_host(ctypes.byref(lt), T, n, _lib.ptr(adv), None) == 0
    d = {k: _dev(v) for k, v in dict(track=track, learn=start).items()}
    adv_d = torch.full((T * n + 1,), float("nan"), device="cuda")  # a value past the end would not even count
    adv_d[:T * n] = _dev(adv).reshape(-1)
    ltd = learn_io(_lib, n_tracks, kind, track=d["track"], learn=d["learn"])
    _lib.check(L.rx_track_learn_tally(ctypes.byref(ltd), T, n, _lib.ptr(adv_d), _lib.stream_ptr()),
               "rx_track_learn_tally")
    got = d["learn"].cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got[n_tracks], start[n_tracks]), "guard row"
    if mode == "none":
        assert np.array_equal(got, start)
    if mode == "one_slot":
        k = n_tracks // 2
        assert got[k, 0] - start[k, 0] == int(np.isfinite(adv).sum())
        assert np.array_equal(np.delete(got, k, 0), np.delete(start, k, 0))


# ---------------------------------------------------------------- 2. fold, rank, tables
@pytest.mark.parametrize("size", ["1", "2", "63", "64", "65", "C-1", "C", "C+1", "70001"])
def test_fold_and_tables_kernels_equal_host_twins(L, size):
    """k_track_learn_fold, k_track_rank and k_track_learn_tables at one lane, around a wave, around the
    scan chunk C (= the rank tile: asserted) and over 69 chunks plus a remainder; scores all equal,
    three values, ties with never-scored slots mixed in, and nothing scored yet; powers 0, 1, 4, 10."""
    from rx import _lib
    C = _lib.RX_TRACK_LEARN_CHUNK
    assert C == _lib.RX_TRACK_RANK_TILE, "were they to differ, the sizes around both belong in the list"
    n = {"C-1": C - 1, "C": C, "C+1": C + 1}.get(size) or int(size)
    now = 9
    for kind in ("equal", "three", "mixed", "unseen"):
        score, seen = score_case(kind, n, now=now)
        # the fold: a third of the slots without samples
        rs = np.random.RandomState(n)
        samples = rs.randint(1, 200, size=n) * (rs.rand(n) < 0.67)
        learn = np.ascontiguousarray(np.stack([samples, rs.randint(0, 1 << 40, size=n) * (samples > 0)], 1),
                                     dtype=np.int64)
        for alpha in (1.0, 0.5):
            l_h, s_h, n_h = learn.copy(), score.copy(), seen.copy()
            lt = learn_io(_lib, n, learn=l_h, score=s_h, seen=n_h)
            assert L.rx_track_learn_fold_host(ctypes.byref(lt), now, alpha, None) == 0
            l_d = torch.full((n + 1, 2), GUARD, dtype=torch.int64, device="cuda")
            s_d = torch.full((n + 1,), float(GUARD), dtype=torch.float64, device="cuda")
            n_d = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
            l_d[:n], s_d[:n], n_d[:n] = _dev(learn), _dev(score), _dev(seen)
            ltd = learn_io(_lib, n, learn=l_d, score=s_d, seen=n_d)
            _lib.check(L.rx_track_learn_fold(ctypes.byref(ltd), now, alpha, _lib.stream_ptr()), "rx_track_learn_fold")
            assert np.array_equal(l_d.cpu().numpy()[:n], l_h) and not l_h.any(), (kind, alpha)
            assert np.array_equal(s_d.cpu().numpy()[:n], s_h) and np.array_equal(n_d.cpu().numpy()[:n], n_h)
            assert (l_d[n] == GUARD).all() and s_d[n] == GUARD and n_d[n] == GUARD
            assert (n_h[learn[:, 0] == 0] == seen[learn[:, 0] == 0]).all()
        # rank + tables on the scores as given and on the folded ones
        for sc, sn in ((score, seen), (s_h, n_h)):
            sc_d, sn_d = _dev(sc), _dev(sn)
            for power in (0, 1, 4, 10):
                rank, cs, ct = host_tables(L, sc, sn, power, now)
                r_d = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
                cs_d = torch.full((n + 1,), GUARD, dtype=torch.int64, device="cuda")
                ct_d = torch.full((n + 1,), GUARD, dtype=torch.int64, device="cuda")
                ltd = learn_io(_lib, n, score=sc_d, seen=sn_d, rank=r_d, cdf_score=cs_d, cdf_stale=ct_d)
                _lib.check(L.rx_track_learn_tables(ctypes.byref(ltd), power, now, _lib.stream_ptr()),
                           "rx_track_learn_tables")
                got_r, got_cs, got_ct = r_d.cpu().numpy(), cs_d.cpu().numpy(), ct_d.cpu().numpy()
                assert np.array_equal(got_r[:n], rank), (kind, power)
                assert np.array_equal(got_cs[:n], cs) and np.array_equal(got_ct[:n], ct), (kind, power)
                assert got_r[n] == GUARD and got_cs[n] == GUARD and got_ct[n] == GUARD
                assert np.array_equal(np.sort(rank), np.arange(1, n + 1))
                if power == 0:
                    assert cs[-1] == n << 32


# ---------------------------------------------------------------- 3. the draw
@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_draw_kernel_equals_host_twin(L, n):
    from rx import _lib
    seed, now = 0xC0FFEE1234567, 9
    tables = []
    for n_tracks, kind in ((37, "mixed"), (1025, "mixed"), (37, "three"), (1, "equal")):
        score, seen = score_case(kind, n_tracks, now=now)
        if kind == "three":
            seen[:] = now  # F_stale == 0
        _, cs, ct = host_tables(L, score, seen, 4, now)
        assert (ct[-1] == 0) == (kind == "three" or bool((seen == now).all()))
        tables.append((cs.copy(), ct.copy()))
    for cs, ct in tables:
        n_tracks = len(cs)
        cs_d, ct_d = _dev(cs), _dev(ct)
        for mix, stale_mix in ((0.0, 0.0), (0.1, 0.1), (1.0, 0.0), (0.0, 1.0), (0.3, 0.7)):
            want = host_draw(L, cs, ct, n, seed, 3, mix, stale_mix)
            out = torch.full((n + 1,), GUARD, dtype=torch.int32, device="cuda")
            ltd = learn_io(_lib, n_tracks, seed=seed, cdf_score=cs_d, cdf_stale=ct_d, track_of_env=out)
            _lib.check(L.rx_track_learn_draw(ctypes.byref(ltd), n, 3, mix, stale_mix, _lib.stream_ptr()),
                       "rx_track_learn_draw")
            got = out.cpu().numpy()
            assert np.array_equal(got[:n], want), (n_tracks, mix, stale_mix)
            assert got[n] == GUARD and want.min() >= 0 and want.max() < n_tracks


# ---------------------------------------------------------------- 4. ReplayCurriculumPPO
def _pool(n_tracks, seed):
    from rx.track import gen_tracks
    rng = np.random.RandomState(seed)
    return gen_tracks(n_tracks, seed=None, rng=rng), [int(rng.randint(6, 10)) for _ in range(n_tracks)]


def _train(replay, updates=4, **over):
    """64 envs x 32 steps on a pool of 8 tracks, max_steps = 12, a resample every 2 updates that retires
    two slots -> (trainer, np.random state after, the parameters after every update, what every update
    left: (advantages, bound track array, score, seen, learn after a second tally of the same advantages),
    what every resample left: (generation, bound track array, score, seen, retired))."""
    from rx.configs import base_config
    from rx.curriculum import CurriculumPPO
    from rx.envs import RacingEnv
    from rx.ppo import build_vector_env
    from rx.track_replay import ReplayCurriculumPPO

    class ShortEpisodes(ReplayCurriculumPPO if replay else CurriculumPPO):
        def _make_envs(self, env_fn):
            c = self.config
            return build_vector_env(env_fn, c["num_envs"], c["seed"], self.device, max_steps=12)

    config = base_config(num_envs=64, num_steps=32, kl_target=1e9, track_resample_every=2, curriculum_mastery=0.0,
                         curriculum_min_episodes=1, **over)
    config["total_timesteps"] = updates * config["batch_size"]
    random.seed(config["seed"])
    np.random.seed(config["seed"])
    torch.manual_seed(config["seed"])
    pool, widths = _pool(8, 21)
    t = ShortEpisodes(lambda i: RacingEnv(num_sensors=11, track_pool=pool, track_id=i % 8, track_width=widths[i % 8]),
                      config, device="cuda")
    folds, swaps, params = [], [], []
    advantages, resample = t.compute_advantages, t.resample_tracks

    def recording(*a):
        adv, ret = advantages(*a)
        if replay:
            r = t.replay
            assert not r.learn.any(), "the fold starts the learn rows again"
            r.tally(adv)  # the same advantages once more: the sums the fold consumed
            folds.append((adv.clone(), t.envs._st["track"].clone(), r.score.clone(), r.seen.clone(), r.learn.clone()))
            r.learn.zero_()
        return adv, ret

    def swapping(*a):
        out = resample(*a)
        if replay:
            r = t.replay
            swaps.append((t.envs.track_generation, t.envs._st["track"].cpu().numpy(), r.score.cpu().numpy(),
                          r.seen.cpu().numpy(), list(t.retired[-1])))
        return out

    t.compute_advantages, t.resample_tracks = recording, swapping
    for u, _, _, _ in t.train_iter():
        params.append([p.detach().clone() for p in t.agent.parameters()])
    assert len(params) == updates
    return t, np.random.get_state(), params, folds, swaps


@pytest.fixture(scope="module")
def trained():
    return _train(True)


def test_trainer_scores_equal_a_torch_restatement(trained):
    t, _, _, folds, _ = trained
    assert len(folds) == 4 and t.replay_updates == 4
    adv, track, score, seen, learn = folds[0]
    assert adv.shape == (32, 64) and torch.isfinite(adv).all() and track.min() >= 0 and track.max() < 8
    q = (adv.abs().clamp(max=1048576.0).double() * 1048576.0).long()  # truncation
    idx = track.long().expand(32, 64).reshape(-1)
    mag = torch.zeros(8, dtype=torch.int64, device="cuda").index_add_(0, idx, q.reshape(-1))
    samples = torch.zeros(8, dtype=torch.int64, device="cuda").index_add_(0, idx, torch.ones_like(idx))
    assert torch.equal(learn, torch.stack([samples, mag], 1)) and samples.sum().item() == 32 * 64
    assert (samples > 0).all(), "env i starts on slot i % 8"
    assert torch.equal(score, (mag.double() / 1048576.0) / samples.double())  # never seen: the mean itself
    assert (seen == 0).all() and (score > 0).all()
    assert (folds[1][3] == 1).all() and not torch.equal(folds[1][2], score)


def test_trainer_redraws_from_the_replay_tables(L, trained):
    t, _, _, folds, swaps = trained
    assert t.envs.track_generation == 1 and len(swaps) == 1 and t.replay.n_tracks == 8
    g, bound, score, seen, retired = swaps[0]
    assert g == 1 and len(retired) == 2
    assert (seen[retired] == -1).all() and not score[retired].any(), "a retired slot starts again as never scored"
    keep = np.setdiff1d(np.arange(8), retired)
    assert (seen[keep] == 1).all() and np.array_equal(score[keep], folds[1][2].cpu().numpy()[keep])
    rank, cs, ct = host_tables(L, np.ascontiguousarray(score), np.ascontiguousarray(seen), 4, 2)
    assert sorted(rank[retired].tolist()) == [1, 2]
    want = host_draw(L, cs, ct, 64, t.config["seed"], 1, 0.1, 0.1)
    assert np.array_equal(bound, want)
    assert np.array_equal(folds[2][1].cpu().numpy(), want), "the tally after the redraw reads the new slots"
    tab = t.track_table()
    assert np.array_equal(np.sort(tab["rank"]), np.arange(1, 9)) and abs(tab["prob"].sum() - 1.0) < 1e-12
    assert np.array_equal(tab["seen"], t.replay.seen.cpu().numpy()) and "episodes" in tab and "prob_finishes" in tab
    assert np.array_equal(tab["staleness"], np.where(tab["seen"] < 0, 0, 4 - tab["seen"]))


def test_trainer_equals_curriculum_ppo_until_the_first_redraw(trained):
    t, state, params, _, _ = trained
    tc, state_c, params_c, _, _ = _train(False)
    assert tc.envs.track_generation == 1
    for u in (0, 1):
        for a, b in zip(params[u], params_c[u]):
            assert torch.equal(a, b), u
    assert state[0] == state_c[0] and np.array_equal(state[1], state_c[1]) and state[2:] == state_c[2:], \
        "the replay scores moved the global numpy stream"
    assert t.retired == tc.retired, "retirement still comes from the finish tallies"
    assert not np.array_equal(t.envs._st["track"].cpu().numpy(), tc.envs._st["track"].cpu().numpy())


def test_trainer_is_deterministic(trained):
    t, state, params, folds, swaps = trained
    t2, state2, params2, folds2, swaps2 = _train(True)
    assert state[0] == state2[0] and np.array_equal(state[1], state2[1]) and state[2:] == state2[2:]
    for a, b in zip(params[-1], params2[-1]):
        assert torch.equal(a, b)
    for a, b in zip(folds, folds2):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(swaps[0][1], swaps2[0][1]) and torch.equal(t.replay.score, t2.replay.score)
    assert torch.equal(t.curriculum.tally, t2.curriculum.tally)
