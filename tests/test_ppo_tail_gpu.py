"""The fused minibatch gradient and the advantage statistics at minibatch sizes
with a tail: mb that is no multiple of a workgroup pass (dead rows), smaller
than one pass (one partial workgroup), and large enough for a second pass that
is mostly dead.  ppo_fused.supported() accepts every such mb (num_envs = 100,
num_steps = 32, num_minibatches = 4 trains at mb = 800).  Reference:
tests/update_ref.py in float64; tests/test_update_ref_cpu.py shows float32
autograd uses under 0.02 of the gradient tolerance on these inputs."""
import numpy as np
import pytest
import torch

from tests import update_ref as ur

pytestmark = pytest.mark.gpu

CASES = [(mb, D) for mb in ur.PPO_MB for D in ur.PPO_D]
BF16_CASES = [(mb, D) for mb in ur.PPO_MB[:-1] for D in ur.PPO_D]  # 16400: the tiles of 800, only slower


class _Fused:
    """FusedMinibatchGrad over ur.ppo_case(mb, D) with tests/test_ppo_fused_gpu.py's Agent set-up."""

    def __init__(self, mb, D, dtype="fp32", perm=None, kl_target=ur.PPO_KL_TARGET):
        from rx.configs import base_config
        from rx.optim import FlatAdam
        from rx.ppo_fused import FusedMinibatchGrad, supported
        self.mb = mb
        self.host, self.perm_host, self.refs = ur.ppo_case(mb, D)
        self.agent = ur.tail_agent(D).cuda()
        self.flat = FlatAdam(self.agent, torch.optim.Adam(self.agent.parameters(), lr=1e-3, eps=1e-5), 0.5)
        self.b = tuple(torch.from_numpy(x).cuda() for x in self.host)
        self.perm = torch.from_numpy(self.perm_host if perm is None else perm).cuda()
        assert supported(self.agent, self.b, mb)
        cfg = base_config(clip_coef=ur.PPO_CLIP, ent_coef=ur.PPO_ENT, vf_coef=ur.PPO_VF, kl_target=kl_target,
                          update_epochs=1, policy_dtype=dtype)
        self.fg = FusedMinibatchGrad(self.agent, self.flat, self.b, mb, self.perm, cfg)
        self.fg.adv_stats()
        self.stop = torch.zeros(1, dtype=torch.bool, device="cuda")
        self.kl_at_stop = torch.zeros(1, device="cuda")

    def grad(self, m):
        """-> (flat gradient, KL partials per workgroup, stop) of minibatch m."""
        self.stop.zero_()
        self.fg.grad(m, self.stop, self.kl_at_stop)
        return self.flat.flat_grad.clone(), self.fg.ws_d.clone(), bool(self.stop)


def _check_tail(mb):
    """The shapes are tails in the library as built (not a hard-coded 64)."""
    from rx import _lib
    L = _lib.load()
    n_wg = L.rx_ppo_n_wg(mb)
    assert mb % 64 != 0 and n_wg == L.rx_ppo_workspace_doubles(mb)
    if mb >= 100:
        assert n_wg > 1
    if mb == 16400:  # workgroups of several passes; the last one's live rows end at least a whole 64-row pass early
        rows_per_wg = -(-(-(-mb // n_wg)) // 64) * 64
        assert rows_per_wg >= 128 and 0 < mb - (n_wg - 1) * rows_per_wg <= rows_per_wg - 64
    return n_wg


@pytest.mark.parametrize("mb,D", CASES)
def test_tail_grad_fp32_matches_float64(mb, D):
    n_wg = _check_tail(mb)
    f = _Fused(mb, D)
    worst = 0.0
    for m in range(2):
        g64, kl64 = f.refs[m]
        got, klp, stop = f.grad(m)
        assert klp.numel() == n_wg
        ratio = ur.tol_ratio(got.cpu().numpy(), g64, ur.GRAD_RTOL, ur.GRAD_ATOL_REL * np.abs(g64).max())
        kl = float(klp.sum()) / mb
        kl_ratio = abs(kl - kl64) / (1e-5 + 1e-4 * abs(kl64))
        worst = max(worst, ratio)
        print(f"\ntail grad fp32 mb={mb} D={D} m={m}: error / tolerance {ratio:.4f}, KL {kl_ratio:.4f}")
        assert ratio <= 1.0 and kl_ratio <= 1.0
        assert stop == (kl64 > ur.PPO_KL_TARGET)
        if stop:
            assert abs(float(f.kl_at_stop) - kl64) <= 1e-5 + 1e-4 * abs(kl64)
    # the other side of the KL check: no stop under a target above every KL
    f2 = _Fused(mb, D, kl_target=1e9)
    assert not f2.grad(0)[2]


@pytest.mark.parametrize("mb,D", BF16_CASES)
def test_tail_grad_bf16_close_to_float64(mb, D):
    """tests/test_bf16_gpu.py's bounds (4e-2 max|g| per element, cosine > 0.999),
    against float64; test_update_ref_cpu.py shows the bounds are fair at every one
    of these shapes, mb = 2 included."""
    _check_tail(mb)
    f = _Fused(mb, D, dtype="bf16")
    for m in range(2):
        g64 = f.refs[m][0]
        got = f.grad(m)[0].double().cpu().numpy()
        err = np.abs(got - g64).max() / np.abs(g64).max()
        cos = float(got @ g64 / np.sqrt((got @ got) * (g64 @ g64)))
        print(f"\ntail grad bf16 mb={mb} D={D} m={m}: err {err / 4e-2:.4f} of 4e-2 max|g|, 1 - cos {1 - cos:.2e}")
        assert np.isfinite(got).all() and err > 0  # really the bf16 path
        assert err <= 4e-2 and cos > 0.999


@pytest.mark.parametrize("dtype,mb,D", [("fp32", mb, D) for mb, D in CASES] + [("bf16", mb, D) for mb, D in BF16_CASES])
def test_dead_rows_contribute_nothing(dtype, mb, D):
    """No tolerance: with every row of the OTHER minibatch overwritten by NaN (the
    statistics kept), minibatch m's gradient and KL partials keep their bits.  A
    tail that gathered past row_end into the next minibatch's perm slice, or let a
    dead row's [X | 1] column through, would turn them NaN."""
    f = _Fused(mb, D, dtype=dtype)
    for m in range(2):
        clean_g, clean_kl, clean_stop = f.grad(m)
        assert torch.isfinite(clean_g).all() and torch.isfinite(clean_kl).all()
        other = f.perm[(1 - m) * mb:(2 - m) * mb]
        for t in f.b:
            t[other] = float("nan")
        g, kl, stop = f.grad(m)
        for t, h in zip(f.b, f.host):
            t.copy_(torch.from_numpy(h))
        assert torch.equal(g, clean_g) and torch.equal(kl, clean_kl) and stop == clean_stop, m


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("D", ur.PPO_D)
def test_tail_equals_explicit_absent_rows(dtype, D):
    """mb = 100 of B = 200: minibatch 0 with the next minibatch's perm slice
    replaced by out-of-range entries (-1 and >= n_rows, which the kernels treat as
    absent rows: include/rx.h) gives the same bits; and a minibatch of absent rows
    only has an exactly zero gradient and KL sum."""
    mb = 100
    a = _Fused(mb, D, dtype=dtype)
    perm = a.perm_host.copy()
    perm[mb::2] = -1
    perm[mb + 1::2] = 2 * mb + 5
    b = _Fused(mb, D, dtype=dtype, perm=perm)
    ga, kla, sa = a.grad(0)
    gb, klb, sb = b.grad(0)
    assert torch.equal(a.fg.stats[:2], b.fg.stats[:2])
    assert torch.equal(ga, gb) and torch.equal(kla, klb) and sa == sb
    assert not b.fg.stats[2:].any()  # no rows: mean 0, std 0
    g1, kl1, s1 = b.grad(1)
    assert not g1.any() and not kl1.any() and not s1


# ------------------------------------------------------------ advantage statistics
def _adv_batch(adv, perm, mb):
    from rx import _lib
    L = _lib.load()
    D, B = 15, adv.size
    t = dict(obs=torch.zeros(B, D), act=torch.zeros(B, 2), logp=torch.zeros(B), adv=torch.from_numpy(adv),
             ret=torch.zeros(B), val=torch.zeros(B), perm=torch.from_numpy(perm),
             params=torch.zeros(L.rx_ppo_n_params(D)), log_std=torch.zeros(2), stats=torch.zeros(2 * ur.ADV_N_MB))
    t = {k: x.cuda() for k, x in t.items()}
    return t, _lib.RxPPOBatch(D, mb, B, *[_lib.ptr(x) for x in t.values()], 0.2, 0.5, 0.015)


def _adv_stats_three_ways(adv, perm, mb):
    """[n_mb, 2] stats of rx_ppo_adv_stats, rx_ppo_adv_stats_ws and rx_ppo_adv_moments ->
    rx_ppo_adv_finalize; the chunk workspace sits between NaN pads."""
    from rx import _lib
    L = _lib.load()
    n_mb, pad = ur.ADV_N_MB, 64
    keep, b = _adv_batch(adv, perm, mb)
    s = _lib.stream_ptr()
    out = []
    st = torch.full((2 * n_mb,), float("nan"), device="cuda")
    _lib.check(L.rx_ppo_adv_stats(b, n_mb, _lib.ptr(st), s), "rx_ppo_adv_stats")
    out.append(st)
    n_ws = L.rx_ppo_adv_workspace_doubles(mb, n_mb)
    assert n_ws == 2 * n_mb * -(-mb // 2048)
    big = torch.full((n_ws + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((2 * n_mb,), float("nan"), device="cuda")
    _lib.check(L.rx_ppo_adv_stats_ws(b, n_mb, _lib.ptr(big[pad:pad + n_ws]), _lib.ptr(st), None, s), "adv_stats_ws")
    assert torch.isnan(big[:pad]).all() and torch.isnan(big[pad + n_ws:]).all()
    assert torch.isfinite(big[pad:pad + n_ws]).all()
    out.append(st)
    mom = torch.full((n_mb, 2), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full((2 * n_mb,), float("nan"), device="cuda")
    _lib.check(L.rx_ppo_adv_moments(b, n_mb, _lib.ptr(mom), s), "rx_ppo_adv_moments")
    _lib.check(L.rx_ppo_adv_finalize(_lib.ptr(mom), n_mb, mb, _lib.ptr(st), s), "rx_ppo_adv_finalize")
    out.append(st)
    assert torch.equal(out[0], out[2])  # include/rx.h: moments -> finalize == rx_ppo_adv_stats bit for bit
    return [x.double().cpu().numpy().reshape(n_mb, 2) for x in out]


@pytest.mark.parametrize("mb", ur.ADV_MB)
def test_adv_stats_tail_sizes(mb):
    """mb = 1 (the count > 1 guard: std 0), 2, under one 256-thread pass, a partial
    and a whole-plus-partial 2,048-row chunk, each entry point against float64 at
    the project's rtol = atol = 1e-6."""
    adv, perm = ur.adv_inputs(mb)
    ref = ur.adv_stats_ref(adv, perm, mb)
    worst = 0.0
    for got in _adv_stats_three_ways(adv, perm, mb):
        worst = max(worst, ur.tol_ratio(got, ref, 1e-6, 1e-6))
        if mb == 1:
            assert (got[:, 1] == 0).all() and np.array_equal(got[:, 0], adv[perm].astype(np.float64))
    print(f"\nadv stats mb={mb}: worst error / tolerance {worst:.4f}")
    assert worst <= 1.0


def test_adv_stats_cancellation():
    """Advantages 1000 + 0.01 sigma, mb = 3000: q and a * mean are ~3e9 and differ
    by ~0.3.  Mean: rtol 1e-6 of the float64 mean.  Std: against the float64
    two-pass std of the float32 inputs at rtol 2.2e-6 -- the float64 moment formula
    (q - a^2 / n) / (n - 1) itself is within 1.03e-6 on these inputs (it meets
    1.1e-6, one float64 rounding of q; test_update_ref_cpu.py), the kernels get twice that."""
    mb = 3000
    adv, perm = ur.adv_inputs(mb, offset=True)
    ref = ur.adv_stats_ref(adv, perm, mb)
    assert ur.ADV_OFFSET_STD_RTOL == 2.2e-6
    for k, got in enumerate(_adv_stats_three_ways(adv, perm, mb)):
        e_mean = np.abs(got[:, 0] / ref[:, 0] - 1).max()
        e_std = np.abs(got[:, 1] / ref[:, 1] - 1).max()
        print(f"\nadv stats cancellation, entry point {k}: mean {e_mean / 1e-6:.4f} of 1e-6, "
              f"std {e_std / ur.ADV_OFFSET_STD_RTOL:.4f} of {ur.ADV_OFFSET_STD_RTOL}")
        assert e_mean <= 1e-6 and e_std <= ur.ADV_OFFSET_STD_RTOL


# ------------------------------------------------------------ end to end
def test_ppo_update_at_a_tail_minibatch_size():
    """One PPO update at mb = 100 (25 envs x 16 steps, 4 minibatches): fused +
    graph against eager autograd with flat Adam, at the tolerances of
    test_fused_update_step_close_to_torch."""
    from tests.test_optim_gpu import _rollout
    from tests.test_ppo_gpu import _train_single_style
    over = dict(num_envs=25, num_steps=16, num_minibatches=4, kl_target=1e9, update_epochs=1)
    ta = _train_single_style(**over)[0]
    tb = _train_single_style(graph_update=False, **over)[0]
    assert ta.config["minibatch_size"] == 100
    tb.agent.load_state_dict(ta.agent.state_dict())
    data = _rollout(ta)
    np.random.seed(5)
    ta.ppo_update(*data)
    np.random.seed(5)
    tb.ppo_update(*data)
    ent = next(iter(ta._upd_graphs.values()))
    assert ent.fused is not None and ent.graph is not None
    assert float(ta._flat.step_t) == 4.0 == float(tb._flat.step_t)
    torch.testing.assert_close(ta._flat.flat_grad, tb._flat.flat_grad, rtol=2e-4,
                               atol=2e-5 * float(tb._flat.flat_grad.abs().max()))
    for x, y in zip(ta.agent.parameters(), tb.agent.parameters()):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=2e-6)
