"""tests/update_ref.py is right, and the inputs of the tail-shape GPU tests are fair.

The float64 references are checked against the recorded reference vectors
(tests/golden/gae.npz, ppo_update.npz).  Then, for every input the GPU tests
use, a float32 evaluation on the host (the oracle's serial GAE, adam_clip_ref in
float32, float32 autograd) must sit within HALF of the tolerance the GPU test
applies against float64: the tolerance then has room for a correct float32
kernel, and a miss on the device is the kernel's.  Every test prints its worst
ratio (error / tolerance).
"""
import warnings

import numpy as np
import pytest
import torch

from tests import update_ref as ur


def _gae_bound(adv):
    return 1e-5 * np.abs(adv).max()  # the project's bound (tests/test_gae_gpu.py)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_gae_ref_matches_golden(golden, tag):
    """Bound: a float32 step rounds ~3 times at 2^-24 of the running magnitude and
    the recurrence damps old error by gamma lambda = 0.96, so the recorded float32
    vectors sit within ~3 * 6e-8 / (1 - 0.96) = 4.5e-6 of max|A|: inside 1e-5."""
    g = golden["gae"]
    c = lambda k: g[f"{tag}_{k}"]  # noqa: E731
    adv, ret = ur.gae_ref(c("rewards"), c("values"), c("dones"), c("next_value"), c("next_done"),
                          float(c("gamma")), float(c("lambda")))
    bound = _gae_bound(adv)
    ea, er = np.abs(adv - c("adv")).max(), np.abs(ret - c("ret")).max()
    print(f"\ngae_ref vs golden [{tag}]: adv {ea / bound:.3f}, ret {er / bound:.3f} of the bound")
    assert ea <= bound and er <= bound


def test_oracle_gae_meets_the_scan_bound(oracle):
    """The serial float32 recurrence (oracle.gae, what k_gae equals bit for bit)
    stays within 1e-5 max|A| of gae_ref on every input of test_gae_edges_gpu.py:
    the bound is fair to ask of k_gae_scan's re-associated float32 sums."""
    worst = 0.0
    for T in ur.GAE_T:
        for N in ur.GAE_N:
            for dones in ur.GAE_DONES:
                for nd_all in (False, True):
                    r, v, d, nv, nd = ur.gae_inputs(T, N, dones, nd_all)
                    for gamma, lam in ur.GAE_PARAMS:
                        adv, ret = ur.gae_ref(r, v, d, nv, nd, gamma, lam)
                        oa, orr = oracle.gae(r, v, d, nv, nd, gamma, lam)
                        bound = _gae_bound(adv)
                        ratio = max(np.abs(oa - adv).max(), np.abs(orr - ret).max()) / bound
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (T, N, dones, nd_all, gamma, lam, ratio)
    print(f"\noracle.gae vs gae_ref: worst {worst:.3f} of 1e-5 max|A|")


@pytest.mark.parametrize("tag", ["full", "d19"])
def test_ppo_loss_grad_ref_matches_golden(tag):
    """The reference's first minibatch (its shuffle, its weights): the float64
    gradient, clipped as clip_grad_norm_ does, against the gradient Adam saw, and
    approx_kl against the recorded one."""
    from tests.golden_util import load
    from tests.test_ppo_golden import _agent, _cfg
    fx = load("ppo_update.npz")
    c = _cfg(fx, tag)
    ag = _agent(fx, tag, "cpu")
    D = fx[f"{tag}_obs"].shape[-1]
    batch = tuple(fx[f"{tag}_{k}"].reshape((-1,) + ((D,) if k == "obs" else (2,) if k == "actions" else ()))
                  for k in ("obs", "actions", "logprobs", "advantages", "returns", "values"))
    inds = np.arange(c["batch_size"])
    np.random.RandomState(int(fx[f"{tag}_np_seed"])).shuffle(inds)
    g, kl = ur.ppo_loss_grad_ref(ag, batch, inds[:c["minibatch_size"]], c["clip_coef"], c["ent_coef"], c["vf_coef"])
    offs = np.concatenate([[0], np.cumsum([p.numel() for p in ag.parameters()])])
    total = np.sqrt(sum((g[a:b] ** 2).sum() for a, b in zip(offs[:-1], offs[1:])))
    g = g * min(c["max_grad_norm"] / (total + 1e-6), 1.0)
    want = fx[f"{tag}_grads"][0]
    ratio = ur.tol_ratio(want, g, ur.GRAD_RTOL, ur.GRAD_ATOL_REL * np.abs(g).max())
    print(f"\nppo_loss_grad_ref vs golden [{tag}]: {ratio:.4f} of the tolerance, kl diff "
          f"{abs(kl - float(fx[f'{tag}_kls'][0])):.2e}")
    assert ratio <= 1.0
    assert abs(kl - float(fx[f"{tag}_kls"][0])) <= 1e-6


def test_adam_inputs_leave_room_for_float32():
    """adam_clip_ref in float32 against float64 on every case of
    test_adam_layouts_gpu.py: within half of each tolerance."""
    worst = {}
    for layout, mn, gs, imported in ur.adam_cases():
        sizes, p, m, v, grads, step0, lrs = ur.adam_inputs(layout, gs, imported)
        r64 = ur.adam_clip_ref(sizes, p, m, v, grads, step0, lrs, ur.ADAM_BETAS, ur.ADAM_EPS, mn)
        r32 = ur.adam_clip_ref(sizes, p, m, v, grads, step0, lrs, ur.ADAM_BETAS, ur.ADAM_EPS, mn, dtype=np.float32)
        for a, b in zip(r32, r64):
            assert a[4] == b[4]
            for k, name in enumerate("pmvg"):
                assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
                ratio = ur.tol_ratio(a[k], b[k], *ur.ADAM_TOL[name])
                worst[name] = max(worst.get(name, 0.0), ratio)
                assert ratio <= 0.5, (layout, mn, gs, imported, name, ratio)
    print("\nAdam float32 twin vs float64, worst error / tolerance: "
          + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


def test_gradient_inputs_leave_room_for_float32():
    """float32 autograd on the host against ppo_loss_grad_ref for every (mb, D) and
    minibatch of test_ppo_tail_gpu.py: within half of the gradient tolerance (a
    clip tie that flips a branch between float32 and float64 would show here)."""
    worst = worst_kl = 0.0
    for mb in ur.PPO_MB:
        for D in ur.PPO_D:
            batch, perm, refs = ur.ppo_case(mb, D)
            ag = ur.tail_agent(D)
            for m, (g64, kl64) in enumerate(refs):
                g32, kl32 = ur.ppo_loss_grad_ref(ag, batch, perm[m * mb:(m + 1) * mb], ur.PPO_CLIP, ur.PPO_ENT,
                                                 ur.PPO_VF, dtype=torch.float32)
                ratio = ur.tol_ratio(g32, g64, ur.GRAD_RTOL, ur.GRAD_ATOL_REL * np.abs(g64).max())
                worst = max(worst, ratio)
                worst_kl = max(worst_kl, abs(kl32 - kl64) / (1e-5 + 1e-4 * abs(kl64)))
                assert np.isfinite(g64).all() and np.abs(g64).max() > 0
                assert ratio <= 0.5, (mb, D, m, ratio)
    print(f"\ngradient float32 twin vs float64: worst {worst:.4f} of the tolerance; KL {worst_kl:.4f} of its own")
    assert worst_kl <= 0.5


def test_bf16_bound_is_fair_at_the_tail_shapes():
    """The bf16 leg's bounds (4e-2 max|g|, cosine > 0.999) asked of the float64
    loss with bf16-rounded weight matrices, per shape of the bf16 leg: the bounds
    must hold for that reference itself before they are asked of the kernel."""
    for mb in ur.PPO_MB[:-1]:
        for D in ur.PPO_D:
            batch, perm, refs = ur.ppo_case(mb, D)
            ag = ur.tail_agent(D, bf16_weights=True)
            for m, (g64, _) in enumerate(refs):
                g, _ = ur.ppo_loss_grad_ref(ag, batch, perm[m * mb:(m + 1) * mb], ur.PPO_CLIP, ur.PPO_ENT, ur.PPO_VF)
                err = np.abs(g - g64).max() / np.abs(g64).max()
                cos = float(g @ g64 / np.sqrt((g @ g) * (g64 @ g64)))
                print(f"\nbf16-rounded weights mb={mb} D={D} m={m}: err {err:.2e} of max|g|, 1 - cos {1 - cos:.2e}")
                assert err <= 4e-2 and cos > 0.999, (mb, D, m, err, cos)


def test_adv_stats_ref_and_the_moment_formula():
    """adv_stats_ref == numpy's mean / std(ddof = 1); mb = 1 gives std 0.  And the
    cancellation case (1000 + 0.01 sigma): the float64 moment formula the kernels
    use, sqrt((q - a^2 / n) / (n - 1)), against the two-pass float64 std of the same
    float32 inputs -- the relative error printed here, times two, is the bound
    test_ppo_tail_gpu.py gives the kernels (ADV_OFFSET_STD_RTOL)."""
    for mb in ur.ADV_MB:
        adv, perm = ur.adv_inputs(mb)
        ref = ur.adv_stats_ref(adv, perm, mb)
        assert ref.shape == (ur.ADV_N_MB, 2)
        a = adv.astype(np.float64)[perm].reshape(ur.ADV_N_MB, mb)
        assert np.allclose(ref[:, 0], a.mean(1), rtol=1e-14, atol=0)
        if mb > 1:
            assert np.allclose(ref[:, 1], a.std(1, ddof=1), rtol=1e-12, atol=0)
        else:
            assert (ref[:, 1] == 0).all()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # torch warns about the zero degrees of freedom
                assert torch.isnan(torch.from_numpy(a[0]).std())  # what torch would give there
    worst = 0.0
    for mb in ur.ADV_MB[1:]:
        adv, perm = ur.adv_inputs(mb, offset=True)
        ref = ur.adv_stats_ref(adv, perm, mb)
        for m in range(ur.ADV_N_MB):
            got = ur.moment_std(adv[perm[m * mb:(m + 1) * mb]])
            if ref[m, 1] > 0:
                worst = max(worst, abs(got - ref[m, 1]) / ref[m, 1])
    print(f"\nfloat64 moment formula on 1000 + 0.01 sigma: worst relative std error {worst:.3e}")
    assert worst <= ur.ADV_OFFSET_STD_RTOL / 2
