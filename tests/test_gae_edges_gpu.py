"""k_gae and k_gae_scan at the shapes the golden vectors never reach: T that is
no multiple of 64 (k_gae_scan: empty lanes, a short last chunk, one step), N
that fills no block (4 envs per block in the scan, 256 in k_gae), every row
done, next_done all true.  Reference: tests/update_ref.py gae_ref (float64);
tests/test_update_ref_cpu.py shows the serial float32 recurrence meets the same
bound on these inputs.

Measured on an MI355X, worst error / bound of k_gae_scan over all patterns: T = 1
0.010, T = 2 0.019, T = 63 0.021, T = 64 0.026, T = 65 0.023, T = 130 0.026
(k_gae, == the oracle: 0.041 at most)."""
import numpy as np
import pytest
import torch

from tests import update_ref as ur

pytestmark = pytest.mark.gpu

PAD = 512  # NaN canary on each side of an output


def _canary(T, N):
    big = torch.full((T * N + 2 * PAD,), float("nan"), device="cuda")
    return big, big[PAD:PAD + T * N].view(T, N)


def _untouched(big, T, N):
    return bool(torch.isnan(big[:PAD]).all() and torch.isnan(big[PAD + T * N:]).all()
                and torch.isfinite(big[PAD:PAD + T * N]).all())


def _dev(*xs):
    return [torch.from_numpy(x).cuda() for x in xs]


@pytest.mark.parametrize("N", ur.GAE_N)
@pytest.mark.parametrize("T", ur.GAE_T)
def test_gae_edges(oracle, T, N):
    """Per done pattern, next_done and (gamma, lambda): k_gae == oracle.gae bit for
    bit and within 1e-5 max|A| of gae_ref; k_gae_scan within 1e-5 max(|A|, 1) of
    gae_ref for adv and ret; neither writes outside its [T, N] outputs."""
    from rx.gae import compute_gae
    worst_scan = worst_serial = 0.0
    for dones in ur.GAE_DONES:
        for nd_all in (False, True):
            r, v, d, nv, nd = ur.gae_inputs(T, N, dones, nd_all)
            tr, tv, td, tnv, tnd = _dev(r, v, d, nv, nd)
            for gamma, lam in ur.GAE_PARAMS:
                case = (dones, nd_all, gamma, lam)
                adv64, ret64 = ur.gae_ref(r, v, d, nv, nd, gamma, lam)
                amax = np.abs(adv64).max()
                # ---- k_gae
                big_a, out_a = _canary(T, N)
                big_r, out_r = _canary(T, N)
                compute_gae(tr, td, tv, tnv, tnd, gamma, lam, out=(out_a, out_r))
                assert _untouched(big_a, T, N) and _untouched(big_r, T, N), case
                oa, orr = oracle.gae(r, v, d, nv, nd, gamma, lam)
                a, rt = out_a.cpu().numpy(), out_r.cpu().numpy()
                assert np.array_equal(a, oa) and np.array_equal(rt, orr), case
                err = max(np.abs(a - adv64).max(), np.abs(rt - ret64).max())
                worst_serial = max(worst_serial, err / (1e-5 * amax))
                assert err <= 1e-5 * amax, (case, err, amax)
                # ---- k_gae_scan
                big_a, out_a = _canary(T, N)
                big_r, out_r = _canary(T, N)
                compute_gae(tr, td, tv, tnv, tnd, gamma, lam, scan=True, out=(out_a, out_r))
                assert _untouched(big_a, T, N) and _untouched(big_r, T, N), case
                bound = 1e-5 * max(amax, 1.0)
                ea = np.abs(out_a.cpu().numpy() - adv64).max()
                er = np.abs(out_r.cpu().numpy() - ret64).max()
                worst_scan = max(worst_scan, ea / bound, er / bound)
                assert ea <= bound and er <= bound, (case, ea, er, bound)
    print(f"\nGAE T={T} N={N}: worst error / bound: k_gae_scan {worst_scan:.4f}, k_gae {worst_serial:.4f}")


@pytest.mark.parametrize("scan", [False, True])
def test_gae_out_buffers_and_strided_inputs(scan):
    """Preallocated out= buffers and non-contiguous rewards / dones / values give
    the plain call's bits."""
    from rx.gae import compute_gae
    T, N = 65, 3
    r, v, d, nv, nd = _dev(*ur.gae_inputs(T, N, "bernoulli", False))
    adv, ret = compute_gae(r, d, v, nv, nd, 0.99, 0.95, scan=scan)
    out = (torch.full((T, N), float("nan"), device="cuda"), torch.full((T, N), float("nan"), device="cuda"))
    got = compute_gae(r, d, v, nv, nd, 0.99, 0.95, scan=scan, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(out[0], adv) and torch.equal(out[1], ret)
    sr, sd, sv = (x.t().contiguous().t() for x in (r, d, v))
    assert not sr.is_contiguous() and torch.equal(sr, r)
    adv2, ret2 = compute_gae(sr, sd, sv, nv, nd, 0.99, 0.95, scan=scan)
    assert torch.equal(adv2, adv) and torch.equal(ret2, ret)
