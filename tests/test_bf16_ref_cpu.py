"""tests/bf16_ref.py is right, its inputs are fair, and its tolerances have power.

  * bf16_round equals torch's float32 -> bfloat16 conversion bit for bit.
  * With every rounding site off, the hand-written backward is autograd.
  * The gradient batches: no forward- or backward-fragile row, every discrete
    decision of head_grad with its margin, every branch present.
  * The forward pools: at most 1 % fragile rows.
  * The float32 twin against the float64 run gives the numbers recorded in
    bf16_ref.py (TWIN_*), from which every tolerance of
    tests/test_bf16_exact_gpu.py is 4 x; the twin also stays inside the error
    budgets the fragility rules assume.
  * Each of the 17 single-site mutants and each structural mutant exceeds the
    tolerance of a tensor it feeds.
Every test prints what it measured.
"""
import functools

import numpy as np
import pytest
import torch

from tests import bf16_ref as br
from tests import update_ref as ur


# ------------------------------------------------------------------ bf16_round
def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _torch_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).bfloat16().float().numpy()


def test_bf16_round_equals_torch_bit_for_bit():
    f = np.float32
    rng = np.random.default_rng(3)
    wide = (rng.standard_normal(200_000) * np.exp(rng.standard_normal(200_000) * 20)).astype(f)
    # ties: 1 + 2^-8 lies between 1 (even) and 1 + 2^-7 -> down; 1 + 3 2^-8 between 1 + 2^-7 and 1 + 2^-6 (even) -> up
    ties = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.75 + 2.0 ** -9, 0.75 + 3 * 2.0 ** -9], dtype=f)
    assert np.array_equal(br.bf16_round(ties), np.array([1.0, 1 + 2.0 ** -6, 0.75, 0.75 + 2.0 ** -7], dtype=f))
    around = np.concatenate([np.nextafter(ties, f(0)), np.nextafter(ties, f(4))])  # one float32 ulp either side
    assert (br.bf16_round(around[:4]) <= ties).all() and (br.bf16_round(around[4:]) >= ties).all()
    assert (br.bf16_round(around[:4]) != br.bf16_round(around[4:])).all()
    # a carry into the next binade: the tie 2 - 2^-8 -> 2 (even), just above it, just below it
    carry = np.array([2 - 2.0 ** -8, 2 - 2.0 ** -9, 2 - 2.0 ** -8 - 2.0 ** -20], dtype=f)
    assert np.array_equal(br.bf16_round(carry), np.array([2.0, 2.0, 2 - 2.0 ** -7], dtype=f))
    zeros = np.array([0.0, -0.0], dtype=f)
    assert np.array_equal(np.signbit(br.bf16_round(zeros)), [False, True])
    # bf16 subnormals (quantum 2^-133): the ties 2^-134 -> 0 (even) and 3 2^-134 -> 2^-132, the edge of the
    # normals, random float32 subnormals
    sub = np.array([2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -133, 2.0 ** -149, 2.0 ** -126, 2.0 ** -126 - 2.0 ** -149])
    sub = np.concatenate([sub, rng.random(20_000) * 2.0 ** -126, rng.random(20_000) * 2.0 ** -130]).astype(f)
    assert br.bf16_round(sub[:2]).tolist() == [0.0, 2.0 ** -132]
    # overflow: float32's max and the top midpoint -> inf, the largest finite bf16 stays
    big = np.array([np.finfo(f).max, 2.0 ** 127 * (2 - 2.0 ** -8), 2.0 ** 127 * (2 - 2.0 ** -7), np.inf, np.nan],
                   dtype=f)
    assert np.isinf(br.bf16_round(big[:2])).all() and br.bf16_round(big[2:3])[0] == big[2]
    every = np.concatenate([wide, ties, around, carry, zeros, sub, big])
    every = np.concatenate([every, -every])
    got, want = br.bf16_round(every), _torch_bf16(every)
    nan = np.isnan(every)
    assert np.isnan(got[nan]).all() and np.isnan(want[nan]).all()
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan]))
    # float64 input: the same values, and ONE rounding: 1 + 2^-8 + 2^-40 is above the midpoint, while its
    # float32 rounding 1 + 2^-8 is the tie that goes down
    got64 = br.bf16_round(every[~nan].astype(np.float64))
    assert got64.dtype == np.float64 and np.array_equal(_bits(got64.astype(f)), _bits(want[~nan]))
    x = np.array([1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8 + 2.0 ** -40)])
    assert br.bf16_round(x).tolist() == [1 + 2.0 ** -7, -(1 + 2.0 ** -7)]
    assert br.bf16_round(x.astype(f)).tolist() == [1.0, -1.0]
    print(f"\nbf16_round == torch bfloat16 on {every.size} float32 values (ties, +-0, subnormals, overflow, NaN)")


# ------------------------------------------------------------------ gradient
@functools.lru_cache(maxsize=None)
def _twin_grads():
    """Per gradient case and minibatch: the twin's (gradient, kl, rows)."""
    out = {}
    for mb, D, absent in br.grad_cases():
        c = br.grad_case(mb, D, absent)
        for m in range(2):
            out[mb, D, absent, m] = br.ppo_grad_bf16_ref(c["agent"], c["batch"], c["perm"][m * mb:(m + 1) * mb],
                                                         dtype=np.float32)
    return out


def test_rounding_off_is_autograd():
    """Every site off: the hand-written backward against ppo_loss_grad_ref (float64
    autograd of the loss written out) within 1e-12 of max|g|, approx_kl within 1e-12."""
    worst = 0.0
    for mb, D, absent in br.grad_cases():
        if absent:  # autograd has no absent rows; the divisor and the statistics are checked by the mutants
            continue
        c = br.grad_case(mb, D)
        for m in range(2):
            idx = c["perm"][m * mb:(m + 1) * mb]
            g, kl, _ = br.ppo_grad_bf16_ref(c["agent"], c["batch"], idx, sites=br.NONE)
            batch = tuple(np.array(x) for x in c["batch"])
            ga, kla = ur.ppo_loss_grad_ref(c["agent"], batch, np.array(idx), ur.PPO_CLIP, ur.PPO_ENT, ur.PPO_VF)
            err = np.abs(g - ga).max() / np.abs(ga).max()
            worst = max(worst, err)
            assert err <= 1e-12 and abs(kl - kla) <= 1e-12, (mb, D, m, err)
            full = np.abs(c["refs"][m][0] - ga).max() / np.abs(ga).max()
            assert 1e-3 < full < 2e-2, full  # what all 17 roundings together move: the size the issue states
    print(f"\nrounding off vs float64 autograd: worst {worst:.2e} of max|g| (bound 1e-12)")


def test_gradient_batches_have_margins_and_every_branch():
    for mb, D, absent in br.grad_cases():
        c = br.grad_case(mb, D, absent)
        assert not br.fragile_rows(c["agent"], c["batch"][0]).any()
        for m in range(2):
            rows = c["refs"][m][2]
            assert not br.backward_fragile(rows).any()
            margins, counts = br.decision_margins(rows)
            print(f"\nmb={mb} D={D} absent={absent} m={m}: margins "
                  + ", ".join(f"{k} {v:.3g}" for k, v in margins.items()) + "; rows per branch "
                  + ", ".join(f"{k}: {v}" for k, v in counts.items()))
            assert margins["ratio"] >= br.RATIO_MARGIN and margins["adv"] >= br.ADV_MARGIN
            assert margins["vd"] >= br.VD_MARGIN and margins["q"] >= br.Q_MARGIN
            if mb >= 24:
                assert min(counts.values()) >= 1, counts
            live = rows["src"].size
            assert live == (mb if not (absent and m == 1) else mb // 2)


def test_twin_gradient_errors_are_the_recorded_ones():
    """The float32 twin against the float64 run, per parameter tensor relative to
    that tensor's max|g|, worst over all cases; approx_kl absolute.  The recorded
    values (bf16_ref.TWIN_GRAD_ERR, TWIN_KL_ERR) bound the measured ones and are
    not stale (within 25 %); GRAD_TOL / KL_TOL are 4 x them."""
    worst = dict.fromkeys(br.TENSORS, 0.0)
    worst_kl = 0.0
    for (mb, D, absent, m), (g32, kl32, _) in _twin_grads().items():
        g64, kl64, _ = br.grad_case(mb, D, absent)["refs"][m]
        for k, e in br.tensor_errors(g32, g64, D).items():
            worst[k] = max(worst[k], e)
        worst_kl = max(worst_kl, abs(kl32 - kl64))
    print("\ntwin vs float64, worst error / max|g| per tensor: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; approx_kl {worst_kl:.2e}")
    print("tolerances: " + ", ".join(f"{k} {v:.2e}" for k, v in br.GRAD_TOL.items()) + f"; approx_kl {br.KL_TOL:.2e}")
    for k, v in worst.items():
        assert v <= br.TWIN_GRAD_ERR[k] <= max(1.25 * v, 1e-12), (k, v, br.TWIN_GRAD_ERR[k])
        assert br.GRAD_TOL[k] == 4 * max(br.TWIN_GRAD_ERR[k], br.TWIN_FLOOR)
    assert worst_kl <= br.TWIN_KL_ERR <= 1.25 * worst_kl and br.KL_TOL == 4 * br.TWIN_KL_ERR


def test_twin_stays_inside_the_fragility_budgets():
    """What the fragility rules assume a float32 evaluation differs by, against the
    twin: hidden activations within FRAGILE_EPS (the recorded worst: TWIN_H_ERR),
    every backward operand within its budget; and no operand of the twin rounds
    to another bf16 than the float64 run's."""
    worst_h, worst_b = 0.0, {}
    for mb, D, absent in br.grad_cases():
        c = br.grad_case(mb, D, absent)
        obs = c["batch"][0]
        worst_h = max(worst_h, np.abs(br.hidden_activations(c["agent"], obs, np.float32)
                                      - br.hidden_activations(c["agent"], obs)).max())
        for m in range(2):
            r64, r32 = c["refs"][m][2], _twin_grads()[mb, D, absent, m][2]
            for k, b in r64["budgets"].items():
                d = np.abs(r32["ops"][k] - r64["ops"][k])
                worst_b[k] = max(worst_b.get(k, 0.0), float(np.where(d > 0, d / np.maximum(b, 1e-300), 0.0).max()))
                assert np.array_equal(br.bf16_round(r32["ops"][k]), br.bf16_round(r64["ops"][k])), (mb, D, m, k)
    for D in br.GRAD_D:
        c = br.forward_case(D)
        ok = ~c["fragile"]
        worst_h = max(worst_h, np.abs(br.hidden_activations(c["agent"], c["obs"], np.float32)
                                      - br.hidden_activations(c["agent"], c["obs"]))[ok].max())
    print(f"\ntwin hidden activations: worst |H - H64| {worst_h:.2e} (FRAGILE_EPS {br.FRAGILE_EPS:.0e}); "
          "operand error / budget: " + ", ".join(f"{k} {v:.3f}" for k, v in worst_b.items()))
    assert worst_h <= br.TWIN_H_ERR <= 1.25 * worst_h and br.TWIN_H_ERR <= br.FRAGILE_EPS / 3
    assert max(worst_b.values()) <= 0.5


# ------------------------------------------------------------------ forward
def test_forward_pools_and_twin_errors():
    """The forward pools keep at most 1 % forward-fragile rows (row 0 is one).  The
    twin against the float64 run: the non-fragile rows of the pools give the tight
    bound, the fragile rows of the pools as drawn (three quarters of uniform rows
    are fragile at FRAGILE_EPS; some 5 % of those flip an operand in the twin) the flip
    bound.  Recorded in bf16_ref.TWIN_FWD_ERR; FWD_TOL is 4 x."""
    tight = dict.fromkeys(br.TWIN_FWD_ERR, 0.0)
    flip = dict.fromkeys(br.TWIN_FWD_ERR, 0.0)
    for D in br.GRAD_D:
        c = br.forward_case(D)
        share, natural = c["fragile"].mean(), c["natural_fragile"].mean()
        flipped = 0
        assert 0 < share <= br.FRAGILE_QUOTA and c["fragile"][0]
        for scale in br.FWD_EPS_SCALE:
            eps = br.forward_eps(c, scale)
            r64 = br.policy_forward_bf16_ref(c["agent"], c["obs"], eps)
            if scale:
                assert (np.abs(r64[0]) == 1).mean() > 0.05  # clamped samples
            else:
                assert np.array_equal(r64[0], r64[3])  # eps = 0: the action is mu
            e = br.forward_errors(br.policy_forward_bf16_ref(c["agent"], c["obs"], eps, np.float32), r64)
            n64 = br.policy_forward_bf16_ref(c["agent"], c["natural"], eps)
            en = br.forward_errors(br.policy_forward_bf16_ref(c["agent"], c["natural"], eps, np.float32), n64)
            for k in tight:
                tight[k] = max(tight[k], e[k][~c["fragile"]].max(), en[k][~c["natural_fragile"]].max())
                flip[k] = max(flip[k], en[k][c["natural_fragile"]].max(), e[k][c["fragile"]].max())
            flipped = max(flipped, int((np.maximum(en["actions"], en["values"]) > 1e-5).sum()))
        print(f"\nforward pool D={D}: fragile share {share:.4f} (as drawn {natural:.3f}); rows of the pool as drawn "
              f"the twin moves beyond 1e-5: {flipped} of {br.FWD_POOL}")
    print("twin vs float64, worst |error|: " + ", ".join(f"{k} tight {tight[k]:.2e} flip {flip[k]:.2e}" for k in tight))
    print("tolerances: " + ", ".join(f"{k} tight {a:.2e} flip {b:.2e}" for k, (a, b) in br.FWD_TOL.items()))
    for k, (a, b) in br.TWIN_FWD_ERR.items():
        assert tight[k] <= a <= 1.25 * tight[k] and flip[k] <= b <= 1.25 * flip[k], (k, tight[k], flip[k])
        assert br.FWD_TOL[k] == (4 * a, 4 * b)


# ------------------------------------------------------------------ power
def _mutant_ratio(kind, name):
    """Worst (error / tolerance) of a mutant over the tensors it feeds, all cases, and where."""
    best = (0.0, None)
    for mb, D, absent in br.grad_cases():
        c = br.grad_case(mb, D, absent)
        for m in range(2):
            idx = c["perm"][m * mb:(m + 1) * mb]
            if kind == "site":
                g = br.ppo_grad_bf16_ref(c["agent"], c["batch"], idx, sites=br.ALL - {name})[0]
                feeds = [t for t in br.TENSORS if t[1:] in br.FEEDS[name]]
            else:
                g = br.ppo_grad_bf16_ref(c["agent"], c["batch"], idx, mutant=name)[0]
                feeds = br.TENSORS
            e = br.tensor_errors(g, c["refs"][m][0], D)
            t = max(feeds, key=lambda t: e[t] / br.GRAD_TOL[t])
            if e[t] / br.GRAD_TOL[t] > best[0]:
                best = (e[t] / br.GRAD_TOL[t], (t, mb, D, absent, m))
    return best


@pytest.mark.parametrize("site", br.SITES)
def test_single_site_mutant_exceeds_its_tolerance(site):
    ratio, where = _mutant_ratio("site", site)
    print(f"\nsite {site} left unrounded: error / tolerance {ratio:.1f} at (tensor, mb, D, absent, m) = {where}")
    assert ratio > 1.0


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_structural_mutant_exceeds_its_tolerance(mutant):
    ratio, where = _mutant_ratio("mutant", mutant)
    print(f"\nmutant {mutant}: error / tolerance {ratio:.1f} at (tensor, mb, D, absent, m) = {where}")
    assert ratio > 1.0
    if mutant == "drop_cols16":
        assert where[2] == 19
    if mutant in ("absent_through", "div_live"):
        assert where[3] and where[4] == 1
