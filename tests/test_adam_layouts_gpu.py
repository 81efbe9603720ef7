"""rx_adam_clip_step through the C ABI at the layouts include/rx.h allows and the
Agent's 13 tensors never reach: more than 16 tensors (k_adam_apply's second
group of folds), tensors above 8,192 entries (the fold's later rounds), tensor
boundaries inside a 64-entry norm block, zero-length tensors, n = 1, a zero
gradient.  Reference: tests/update_ref.py adam_clip_ref in float64 at the
tolerances of tests/test_optim_gpu.py; tests/test_update_ref_cpu.py shows a
float32 evaluation uses at most 0.12 of them on these inputs."""
import ctypes

import numpy as np
import pytest
import torch

from tests import update_ref as ur

pytestmark = pytest.mark.gpu

PAD = 256  # NaN canary (floats) on each side of every buffer


def _cfg(sizes, max_norm):
    from rx import _lib
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cfg = _lib.RxAdamConfig(len(sizes), (ctypes.c_int64 * 33)(*offs.tolist()), ur.ADAM_BETAS[0], ur.ADAM_BETAS[1],
                            ur.ADAM_EPS, float(max_norm))
    return cfg


class _Padded:
    """n float32 values in the middle of a NaN-filled buffer."""

    def __init__(self, n, init=None):
        self.n = n
        self.big = torch.full((n + 2 * PAD,), float("nan"), device="cuda")
        self.t = self.big[PAD:PAD + n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)))

    def pads_intact(self):
        return bool(torch.isnan(self.big[:PAD]).all() and torch.isnan(self.big[PAD + self.n:]).all())


class _Run:
    def __init__(self, sizes, max_norm, p, m, v, step0):
        from rx import _lib
        self.L = _lib.load()
        self.cfg = _cfg(sizes, max_norm)
        n = int(sum(sizes))
        n_ws = self.L.rx_adam_workspace_floats(ctypes.byref(self.cfg))
        assert n_ws == -(-n // 64) * len(sizes) + 2  # ceil(n / 64) norm blocks x tensors + Adam's 2 scalars
        self.p, self.m, self.v = _Padded(n, p), _Padded(n, m), _Padded(n, v)
        self.g, self.ws = _Padded(n), _Padded(n_ws)
        self.step = torch.full((), float(step0), device="cuda")
        self.lr = torch.zeros((), dtype=torch.float64, device="cuda")

    def __call__(self, grad, lr, stop=None):
        from rx import _lib
        self.g.t.copy_(torch.from_numpy(np.ascontiguousarray(grad)))
        self.lr.fill_(lr)
        _lib.check(self.L.rx_adam_clip_step(ctypes.byref(self.cfg), _lib.ptr(self.p.t), _lib.ptr(self.g.t),
                                            _lib.ptr(self.m.t), _lib.ptr(self.v.t), _lib.ptr(self.step),
                                            _lib.ptr(self.lr), _lib.ptr(stop) if stop is not None else None,
                                            _lib.ptr(self.ws.t), _lib.stream_ptr()), "rx_adam_clip_step")

    def state(self):
        return {"p": self.p.t.cpu().numpy(), "m": self.m.t.cpu().numpy(), "v": self.v.t.cpu().numpy(),
                "g": self.g.t.cpu().numpy()}

    def pads_intact(self):
        return all(x.pads_intact() for x in (self.p, self.m, self.v, self.g, self.ws))


@pytest.mark.parametrize("layout,max_norm,grad_scale,imported", list(ur.adam_cases()))
def test_adam_layout_matches_float64(layout, max_norm, grad_scale, imported):
    sizes, p, m, v, grads, step0, lrs = ur.adam_inputs(layout, grad_scale, imported)
    ref = ur.adam_clip_ref(sizes, p, m, v, grads, step0, lrs, ur.ADAM_BETAS, ur.ADAM_EPS, max_norm)
    run = _Run(sizes, max_norm, p, m, v, step0)
    worst = dict.fromkeys("pmvg", 0.0)
    for it, (rp, rm, rv, rg, rstep) in enumerate(ref):
        run(grads[it], lrs[it])
        got = run.state()
        assert float(run.step) == rstep
        for name, want in zip("pmvg", (rp, rm, rv, rg)):
            assert np.isfinite(got[name]).all(), (it, name)
            ratio = ur.tol_ratio(got[name], want, *ur.ADAM_TOL[name])
            worst[name] = max(worst[name], ratio)
            assert ratio <= 1.0, (it, name, ratio)
        if grad_scale == 0.0:  # coef is exactly 1: the gradient comes back as exact zeros
            assert not got["g"].any()
    assert run.pads_intact()
    print(f"\nAdam {layout} max_norm={max_norm} scale={grad_scale} imported={imported}: worst error / tolerance "
          + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


def test_adam_zero_gradient_moves_only_by_the_moments():
    """A zero gradient on an imported state: the parameters move by Adam's own
    update from the decayed moments (the float64 reference), grads stay exact
    zeros, nothing is NaN -- at max_norm = 0.5, where total = 0 and coef =
    min(0.5 / 1e-6, 1) = 1."""
    sizes, p, m, v, grads, step0, lrs = ur.adam_inputs("32mixed", 0.0, True)
    assert not grads.any()
    ref = ur.adam_clip_ref(sizes, p, m, v, grads[:1], step0, lrs[:1], ur.ADAM_BETAS, ur.ADAM_EPS, 0.5)[0]
    run = _Run(sizes, 0.5, p, m, v, step0)
    run(grads[0], lrs[0])
    got = run.state()
    assert not got["g"].any() and all(np.isfinite(x).all() for x in got.values())
    assert np.abs(got["p"] - p).max() > 0  # it did move
    for name, want in zip("pmv", ref[:3]):
        assert ur.tol_ratio(got[name], want, *ur.ADAM_TOL[name]) <= 1.0, name
    assert float(run.step) == step0 + 1 and run.pads_intact()


def test_adam_stop_flag_changes_nothing():
    sizes, p, m, v, grads, step0, lrs = ur.adam_inputs("32mixed", 1.0, True)
    run = _Run(sizes, 0.5, p, m, v, step0)
    stop = torch.ones(1, dtype=torch.bool, device="cuda")
    run(grads[0], lrs[0], stop=stop)
    got = run.state()
    for name, want in zip("pmvg", (p, m, v, grads[0])):
        assert np.array_equal(got[name], want), name
    assert float(run.step) == step0 and run.pads_intact()


@pytest.mark.parametrize("D", [15, 19])
def test_norm_partials_equal_between_the_two_optimizer_paths(D):
    """rx_optim.hip: k_adam_norm's partials are "exactly the partials k_ppo_reduce
    writes".  rx_ppo_minibatch_grad + rx_adam_clip_step against
    rx_ppo_minibatch_update on the same minibatch (a tail size, clipping active):
    parameters, moments, clipped gradient and step count bit for bit."""
    from rx.configs import base_config
    from rx.optim import FlatAdam
    from rx.ppo_fused import FusedMinibatchGrad
    mb = 100
    batch, perm, _ = ur.ppo_case(mb, D)
    cfg = base_config(clip_coef=ur.PPO_CLIP, vf_coef=ur.PPO_VF, kl_target=1e9, update_epochs=1)
    res = []
    for fused in (False, True):
        ag = ur.tail_agent(D).cuda()
        fl = FlatAdam(ag, torch.optim.Adam(ag.parameters(), lr=1e-3, eps=1e-5), 0.5)
        fl.sync_lr()
        b = tuple(torch.from_numpy(x).cuda() for x in batch)
        fg = FusedMinibatchGrad(ag, fl, b, mb, torch.from_numpy(perm).cuda(), cfg)
        fg.adv_stats()
        stop = torch.zeros(1, dtype=torch.bool, device="cuda")
        kl = torch.zeros(1, device="cuda")
        for m in range(2):
            if fused:
                fg.update(m, stop, kl)
            else:
                fg.grad(m, stop, kl)
                fl.step(stop=stop)
        assert not bool(stop)
        res.append([t.clone() for t in (fl.flat_param, fl.exp_avg, fl.exp_avg_sq, fl.flat_grad, fl.step_t)])
    norm = float(torch.linalg.vector_norm(res[0][3]))
    assert norm <= 0.5 * (1 + 1e-5) and norm > 0.49  # the clip was active: the norms mattered
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert float(res[0][4]) == 2.0
