"""The bf16 policy kernels against the operand-rounded float64 reference of
tests/bf16_ref.py ("The bf16 contract"): rx_policy_act in bf16
precision and k_ppo_grad_bf through FusedMinibatchGrad.

Every tolerance is 4 x an error of the reference's float32 twin against its
float64 run, measured on the host and recorded in bf16_ref.py (TWIN_*; checked
by tests/test_bf16_ref_cpu.py); none comes from a kernel.  Each case prints its
error / tolerance.

The other bf16 launches need no leg of their own: they are held bit for bit to
rx_policy_act in bf16 by
  * the policy bank            test_league_gpu.py::test_bank_equals_single, ::test_bank_two_car_layout
  * self-play                  test_selfplay_train_gpu.py::test_selfplay_rollout_steps_equals_per_step_path
  * league training            test_league_train_gpu.py::test_pinned_opponent_equals_selfplay_rollout,
                               ::test_mixed_opponents_equal_step_by_step_composition
  * rx_rollout_steps (the prebuilt-fragment forward)
                               test_rollout_gpu.py::test_rollout_steps_equals_per_step_path
  * eval                       test_eval_fused_gpu.py::test_policy_mode_single_agent, ::test_two_cars
each of which has a bf16 case.
"""
import functools

import numpy as np
import pytest
import torch

from tests import bf16_ref as br
from tests import update_ref as ur

pytestmark = pytest.mark.gpu
PAD = 64  # NaN rows behind every output


def _device_agent(D):
    from rx.optim import FlatAdam
    agent = ur.tail_agent(D).cuda()
    return agent, FlatAdam(agent, torch.optim.Adam(agent.parameters(), lr=1e-3, eps=1e-5), 0.5)


@functools.lru_cache(maxsize=None)
def _forward_ref(D, scale):
    """The float64 reference over the whole pool, once per (D, eps scale); a test at n rows reads the first n."""
    c = br.forward_case(D)
    out = br.policy_forward_bf16_ref(c["agent"], c["obs"], br.forward_eps(c, scale))
    for x in out:
        x.setflags(write=False)
    return out


def _check_forward(tag, D, scale, n, act, lp, val):
    """Rows [0, n) of the outputs against the reference: the tight bound on the
    non-fragile rows, the flip bound on the forward-fragile ones."""
    fragile = br.forward_case(D)["fragile"][:n]
    ref = tuple(x[:n] for x in _forward_ref(D, scale))
    err = br.forward_errors((act, lp, val), ref)
    worst = {}
    for k, e in err.items():
        tol = np.where(fragile, br.FWD_TOL[k][1], br.FWD_TOL[k][0])
        assert np.isfinite(e).all(), (tag, k)
        worst[k] = float((e / tol).max())
    print(f"\n{tag}: error / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" ({int(fragile.sum())} fragile rows of {n})")
    bad = {k: int(np.argmax(e / np.where(fragile, br.FWD_TOL[k][1], br.FWD_TOL[k][0]))) for k, e in err.items()
           if worst[k] > 1.0}
    assert not bad, (tag, worst, {k: (i, bool(fragile[i]), float(err[k][i])) for k, i in bad.items()})


@pytest.mark.parametrize("scale", br.FWD_EPS_SCALE)
@pytest.mark.parametrize("n", br.FWD_N)
@pytest.mark.parametrize("D", br.GRAD_D)
def test_policy_act_bf16_matches_the_reference(D, n, scale):
    """n = 1 (a partial 16-row tile), 16, 17, 65 (one row in the second workgroup
    pair), 4,099; eps = 0 (the action is mu) and 1.5 N(0, 1) (clamped samples and
    their log-probs).  The outputs are NaN behind row n and stay so."""
    from rx import _lib
    L = _lib.load()
    c = br.forward_case(D)
    agent, flat = _device_agent(D)
    obs = torch.from_numpy(c["obs"][:n].copy()).cuda()
    eps = torch.from_numpy(br.forward_eps(c, scale, n)).cuda()
    nan = float("nan")
    act = torch.full((n + PAD, 2), nan, device="cuda")
    lp, val = torch.full((n + PAD,), nan, device="cuda"), torch.full((n + PAD,), nan, device="cuda")
    io = _lib.RxPolicyIO(D, n, _lib.ptr(obs), _lib.ptr(eps), _lib.ptr(flat.flat_param), _lib.ptr(agent.log_std),
                         _lib.ptr(act), _lib.ptr(lp), _lib.ptr(val), 0, 0, _lib.RX_PREC_BF16, None, 0)
    _lib.check(L.rx_policy_act(io, _lib.stream_ptr()), "rx_policy_act")
    torch.cuda.synchronize()
    assert torch.isnan(act[n:]).all() and torch.isnan(lp[n:]).all() and torch.isnan(val[n:]).all()
    a = act[:n].cpu().numpy()
    if scale:
        if n >= 65:
            assert (np.abs(a) == 1).any()
    else:
        assert (np.abs(a) < 1).all()
    _check_forward(f"policy_act bf16 D={D} n={n} eps x {scale}", D, scale, n, a, lp[:n].cpu().numpy(),
                   val[:n].cpu().numpy())


@pytest.mark.parametrize("D", br.GRAD_D)
def test_policy_act_bf16_strided_rows(D):
    """n = 17 rows read as car 1 of an [n][2][D] observation buffer (obs_stride = 2 D)
    whose car 0 rows are NaN, written as car 1 of an [n][2][2] action buffer
    (act_stride = 4) and to actions2 with its own stride 3; every output slot
    the launch does not own stays NaN."""
    from rx import _lib
    L = _lib.load()
    n, scale = 17, br.FWD_EPS_SCALE[1]
    c = br.forward_case(D)
    agent, flat = _device_agent(D)
    nan = float("nan")
    obs = torch.full((n, 2, D), nan, device="cuda")
    obs[:, 1] = torch.from_numpy(c["obs"][:n].copy()).cuda()
    eps = torch.from_numpy(br.forward_eps(c, scale, n)).cuda()
    act = torch.full((n + PAD, 2, 2), nan, device="cuda")
    act2 = torch.full((n + PAD, 3), nan, device="cuda")
    lp, val = torch.full((n + PAD,), nan, device="cuda"), torch.full((n + PAD,), nan, device="cuda")
    io = _lib.RxPolicyIO(D, n, _lib.view_ptr(obs[:, 1]), _lib.ptr(eps), _lib.ptr(flat.flat_param),
                         _lib.ptr(agent.log_std), _lib.view_ptr(act[:, 1]), _lib.ptr(lp), _lib.ptr(val), 2 * D, 4,
                         _lib.RX_PREC_BF16, _lib.ptr(act2), 3)
    _lib.check(L.rx_policy_act(io, _lib.stream_ptr()), "rx_policy_act")
    torch.cuda.synchronize()
    assert torch.isnan(act[:, 0]).all() and torch.isnan(act[n:]).all()
    assert torch.isnan(act2[:, 2]).all() and torch.isnan(act2[n:]).all()
    assert torch.isnan(lp[n:]).all() and torch.isnan(val[n:]).all()
    assert torch.equal(act[:n, 1], act2[:n, :2])
    _check_forward(f"policy_act bf16 strided D={D} n={n}", D, scale, n, act[:n, 1].cpu().numpy(),
                   lp[:n].cpu().numpy(), val[:n].cpu().numpy())


class _Fused:
    """FusedMinibatchGrad in bf16 over br.grad_case(mb, D, absent), set up as test_ppo_tail_gpu._Fused."""

    def __init__(self, mb, D, absent):
        from rx.configs import base_config
        from rx.ppo_fused import FusedMinibatchGrad, supported
        self.case = br.grad_case(mb, D, absent)
        self.agent, self.flat = _device_agent(D)
        self.b = tuple(torch.from_numpy(x.copy()).cuda() for x in self.case["batch"])
        self.perm = torch.from_numpy(self.case["perm"].copy()).cuda()
        assert supported(self.agent, self.b, mb)
        cfg = base_config(clip_coef=ur.PPO_CLIP, ent_coef=ur.PPO_ENT, vf_coef=ur.PPO_VF, kl_target=1e9,
                          update_epochs=1, policy_dtype="bf16")
        self.fg = FusedMinibatchGrad(self.agent, self.flat, self.b, mb, self.perm, cfg)
        self.fg.adv_stats()
        self.stop = torch.zeros(1, dtype=torch.bool, device="cuda")
        self.kl_at_stop = torch.zeros(1, device="cuda")

    def grad(self, m):
        """-> (flat gradient, approx_kl) of minibatch m."""
        self.stop.zero_()
        self.fg.grad(m, self.stop, self.kl_at_stop)
        assert not bool(self.stop)
        return self.flat.flat_grad.double().cpu().numpy(), float(self.fg.ws_d.sum()) / self.case["mb"]


@pytest.mark.parametrize("mb,D,absent", br.grad_cases())
def test_ppo_grad_bf16_matches_the_reference(mb, D, absent):
    """mb = 2, 24, 100, 800 (test_ppo_tail_gpu.py's tails) x D x both minibatches, per
    parameter tensor relative to that tensor's max|g|, and approx_kl; absent: mb =
    100 with half of minibatch 1's perm slice -1 or >= n_rows, which the reference
    leaves out while it keeps the divisor and the statistics' count at mb."""
    from rx import _lib
    assert mb % 64 != 0 and (mb < 100 or _lib.load().rx_ppo_n_wg(mb) > 1)  # a tail; several workgroups from 100
    f = _Fused(mb, D, absent)
    if absent:
        perm = f.case["perm"][mb:]
        assert ((perm < 0) | (perm >= 2 * mb)).sum() == mb // 2 and (perm < 0).any() and (perm >= 2 * mb).any()
    failed = []
    for m in range(2):
        g64, kl64, _ = f.case["refs"][m]
        got, kl = f.grad(m)
        assert np.isfinite(got).all()
        ratio = {k: e / br.GRAD_TOL[k] for k, e in br.tensor_errors(got, g64, D).items()}
        kl_ratio = abs(kl - kl64) / br.KL_TOL
        print(f"\nppo_grad bf16 mb={mb} D={D} absent={absent} m={m}: error / tolerance "
              + ", ".join(f"{k} {v:.3f}" for k, v in ratio.items()) + f", approx_kl {kl_ratio:.3f}")
        if max(ratio.values()) > 1.0 or kl_ratio > 1.0:
            failed.append((m, {k: round(v, 3) for k, v in ratio.items() if v > 1.0}, round(kl_ratio, 3)))
    assert not failed, failed
