"""Float64 restatements of the PPO update's four operations ("Tail
shapes"), for tests/test_update_ref_cpu.py and the GPU tests that run the HIP
kernels at their tail shapes.  Plain numpy / torch on the host; nothing here
calls librx, and the only import from rx is the Agent the loss needs.

  * gae_ref            agent/ppo.py:134-154
  * adv_stats_ref      agent/ppo.py:186-187 (mean, unbiased std per minibatch)
  * adam_clip_ref      agent/ppo.py:204-207 (clip_grad_norm_ + Adam, eps = 1e-5)
  * ppo_loss_grad_ref  agent/ppo.py:170-203 (loss, autograd gradient, approx_kl)

The second half builds the tests' inputs from numpy.random.default_rng(seed) on
the host, so the CPU checks and the device see the same arrays.
"""
import copy
import functools
import math
import types

import numpy as np
import torch


# ------------------------------------------------------------------ references
def gae_ref(r, v, d, nv, nd, gamma, lam):
    """PPO.compute_advantages in float64: r / v / d [T, N], nv / nd [N] -> (adv, ret) [T, N]."""
    r, v, d, nv, nd = (np.asarray(x, dtype=np.float64) for x in (r, v, d, nv, nd))
    T = r.shape[0]
    adv = np.zeros_like(r)
    run = np.zeros_like(nv)
    for t in reversed(range(T)):
        nnt = 1.0 - (nd if t == T - 1 else d[t + 1])
        nxt = nv if t == T - 1 else v[t + 1]
        delta = r[t] + gamma * nnt * nxt - v[t]
        adv[t] = run = delta + gamma * lam * nnt * run
    return adv, adv + v


def adv_stats_ref(adv, perm, mb):
    """(mean, unbiased std) of adv[perm[m * mb : (m + 1) * mb]] for every whole
    minibatch m of perm, float64 [n_mb, 2].  mb = 1 gives a standard deviation of
    0, the kernels' count > 1 guard; torch's std() of one element is NaN."""
    a = np.asarray(adv, dtype=np.float64)[np.asarray(perm)]
    a = a[:a.size // mb * mb].reshape(-1, mb)
    mean = a.mean(1)
    std = np.sqrt(((a - mean[:, None]) ** 2).sum(1) / (mb - 1)) if mb > 1 else np.zeros_like(mean)
    return np.stack([mean, std], 1)


def adam_clip_ref(sizes, p, m, v, grads, step0, lrs, betas, eps, max_norm, dtype=np.float64):
    """len(grads) steps of clip_grad_norm_(max_norm) + torch.optim.Adam over the
    tensors of ``sizes`` stored back to back in flat arrays, all arithmetic in
    ``dtype``: per-tensor norms -> total norm, coef = min(max_norm / (total +
    1e-6), 1) (max_norm <= 0: no clipping), then g *= coef; m = lerp(m, g, 1 - b1);
    v = b2 v + (1 - b2) g g; p += step_size * m / (sqrt(v) / bc2_sqrt + eps) with
    step_size = -lr / (1 - b1^s), bc2_sqrt = sqrt(1 - b2^s) (the step scalars are
    computed in float64 and rounded to ``dtype``, as rx_adam_scalars does).
    Returns one (p, m, v, clipped g, step) tuple per step."""
    f = dtype
    p, m, v = (np.array(x, dtype=f) for x in (p, m, v))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    b1, b2 = betas
    out = []
    step = float(step0)
    for g, lr in zip(grads, lrs):
        g = np.array(g, dtype=f)
        step += 1.0
        if max_norm > 0:
            norms = np.array([np.sqrt((g[a:b] * g[a:b]).sum(dtype=f)) for a, b in zip(offs[:-1], offs[1:])], dtype=f)
            total = np.sqrt((norms * norms).sum(dtype=f))
            coef = min(f(max_norm) / (total + f(1e-6)), f(1.0))
            g = g * f(coef)
        step_size = f(-(lr / (1.0 - b1 ** step)))
        bc2_sqrt = f(math.sqrt(1.0 - b2 ** step))
        m = m + f(1.0 - b1) * (g - m)
        v = v * f(b2) + f(1.0 - b2) * g * g
        p = p + step_size * (m / (np.sqrt(v) / bc2_sqrt + f(eps)))
        out.append((p.copy(), m.copy(), v.copy(), g.copy(), step))
    return out


def ppo_loss(agent, batch, idx, clip_coef, ent_coef, vf_coef):
    """The minibatch loss of agent/ppo.py:170-203 written out (Normal log-prob and
    entropy included) in the dtype of ``agent`` / ``batch`` -> (loss, approx_kl)."""
    obs, act, old_lp, adv, ret, val = (x[idx] for x in batch)
    mu = agent.actor_mu(obs)
    log_std = agent.log_std.to(mu.dtype)
    var = torch.exp(log_std) ** 2
    lp = (-((act - mu) ** 2) / (2 * var) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum(-1).expand_as(lp)
    value = agent.critic(obs).flatten()
    ratio = (lp - old_lp).exp()
    with torch.no_grad():
        kl = (old_lp - lp).mean()
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    v_clip = val + torch.clamp(value - val, -clip_coef, clip_coef)
    v_loss = 0.5 * torch.max((value - ret) ** 2, (v_clip - ret) ** 2).mean()
    return pg + ent_coef * (-entropy.mean()) + vf_coef * v_loss, kl


def ppo_loss_grad_ref(agent64, batch, idx, clip_coef, ent_coef, vf_coef, dtype=torch.float64):
    """Autograd of ppo_loss on a ``dtype`` (float64) deep copy of the Agent over
    rows ``idx`` of batch = (obs, actions, logprobs, advantages, returns, values)
    -> (flat gradient in parameters() order, approx_kl), float64 numpy / float.
    dtype = float32 is the CPU twin of test_update_ref_cpu.py."""
    ag = copy.deepcopy(agent64).cpu().to(dtype)
    b = tuple(torch.as_tensor(np.asarray(x)).to(dtype) for x in batch)
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    loss, kl = ppo_loss(ag, b, idx, clip_coef, ent_coef, vf_coef)
    grads = torch.autograd.grad(loss, list(ag.parameters()))
    return torch.cat([g.reshape(-1) for g in grads]).double().numpy(), float(kl)


# ---------------------------------------------------------------------- inputs
# GAE (tests/test_gae_edges_gpu.py): every T at which k_gae_scan's chunking
# changes (one lane, empty lanes, L = 1 exactly, L = 2 and 3 with a short last
# chunk) x every N at which a block is partial (k_gae_scan: 4 envs per block;
# k_gae: 256)
GAE_T = (1, 2, 63, 64, 65, 130)
GAE_N = (1, 3, 257)
GAE_DONES = ("bernoulli", "zeros", "ones", "last")
GAE_PARAMS = ((0.99, 0.95), (1.0, 1.0), (0.99, 0.0))


def gae_inputs(T, N, dones, next_done):
    """r ~ 10 sigma, v ~ 30 sigma (the golden generator's scales), float32; the
    done pattern: Bernoulli(0.3), all 0, all 1, or 1 only at t = T - 1."""
    rng = np.random.default_rng(1000 * T + N)
    r = rng.normal(0, 10, (T, N)).astype(np.float32)
    v = rng.normal(0, 30, (T, N)).astype(np.float32)
    nv = rng.normal(0, 30, N).astype(np.float32)
    if dones == "bernoulli":
        d = (rng.random((T, N)) < 0.3).astype(np.float32)
    elif dones == "ones":
        d = np.ones((T, N), dtype=np.float32)
    else:
        d = np.zeros((T, N), dtype=np.float32)
        if dones == "last":
            d[T - 1] = 1.0
    nd = np.full(N, 1.0 if next_done else 0.0, dtype=np.float32)
    return r, v, d, nv, nd


# rx_adam_clip_step (tests/test_adam_layouts_gpu.py)
ADAM_LAYOUTS = {
    "one": [1],
    "17x100": [100] * 17,                                 # the first layout beyond 16 tensors
    "32mixed": [1, 63, 65, 0, 130, 7] * 5 + [3, 9000],    # 32 tensors; > 8,192 entries through the u2 branch
    "20000x5": [20000, 1, 0, 64] * 5,                     # the fold's second and third rounds
}
ADAM_MAX_NORMS = (0.5, 1e6, 0.0)
ADAM_GRAD_SCALES = (1.0, 1e-4, 0.0)
ADAM_BETAS, ADAM_EPS, ADAM_STEPS = (0.9, 0.999), 1e-5, 6
# the project's tolerances (tests/test_optim_gpu.py): (rtol, atol) of parameters, clipped gradients, moments
ADAM_TOL = {"p": (2e-5, 2e-7), "g": (1e-5, 1e-7), "m": (2e-5, 1e-6), "v": (2e-5, 1e-6)}


def adam_cases():
    """(layout, max_norm, grad_scale, imported): every layout x max_norm x gradient
    scale from step 0, and each layout once from an imported state."""
    for layout in ADAM_LAYOUTS:
        for mn in ADAM_MAX_NORMS:
            for gs in ADAM_GRAD_SCALES:
                yield layout, mn, gs, False
        yield layout, 0.5, 1.0, True


def adam_inputs(layout, grad_scale, imported):
    """(sizes, p, m, v, grads [6, n], step0, lrs): parameters ~ 0.1 sigma, six
    gradients ~ (0.1 + it) * grad_scale sigma with lr = 3e-4 (1 - it / 6) (as
    test_flat_adam_matches_torch), from zero state at step 0 or from an imported
    state (moments of a past run, step = 10000)."""
    sizes = ADAM_LAYOUTS[layout]
    n = int(sum(sizes))
    rng = np.random.default_rng(sorted(ADAM_LAYOUTS).index(layout) * 10 + int(imported))
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    grads = np.stack([rng.standard_normal(n) * (0.1 + it) * grad_scale for it in range(ADAM_STEPS)]).astype(np.float32)
    if imported:
        m = (0.05 * rng.standard_normal(n)).astype(np.float32)
        v = (0.01 * rng.random(n) + 1e-6).astype(np.float32)
    else:
        m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    lrs = [3e-4 * (1 - it / ADAM_STEPS) for it in range(ADAM_STEPS)]
    return sizes, p, m, v, grads, (10000.0 if imported else 0.0), lrs


def tol_ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is torch.testing.assert_close's pass."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


# fused minibatch gradient (tests/test_ppo_tail_gpu.py): B = 2 mb
PPO_MB = (2, 24, 100, 800, 16400)
PPO_D = (15, 19)
PPO_CLIP, PPO_ENT, PPO_VF, PPO_KL_TARGET = 0.2, 0.0, 0.5, 0.015
GRAD_RTOL, GRAD_ATOL_REL = 2e-4, 2e-5  # the project's gradient tolerance: atol = 2e-5 max|g|


def tail_agent(D, bf16_weights=False):
    """The Agent of tests/test_ppo_fused_gpu.py (log_std = -0.8, head x 60), built
    on the host; bf16_weights rounds every weight matrix to bf16 (biases stay
    float32, as the bf16 kernels keep them)."""
    from rx.agent import Agent
    state = torch.random.get_rng_state()
    torch.manual_seed(7)
    ag = Agent(types.SimpleNamespace(shape=(D,)), types.SimpleNamespace(shape=(2,)))
    torch.random.set_rng_state(state)
    ag.log_std.fill_(-0.8)
    with torch.no_grad():
        ag.actor_mu[4].weight.mul_(60.0)
        if bf16_weights:
            for seq in (ag.actor_mu, ag.critic):
                for k in (0, 2, 4):
                    seq[k].weight.copy_(seq[k].weight.bfloat16().float())
    return ag


def ppo_batch(B, D, seed):
    """(obs, actions, logprobs, advantages, returns, values) float32 numpy, the
    distributions of tests/test_ppo_fused_gpu.py's _batch, and a permutation of B."""
    rng = np.random.default_rng(seed)
    f = np.float32
    obs = (rng.random((B, D)) * 2 - 1).astype(f)
    act = (rng.random((B, 2)) * 2 - 1).astype(f)
    logp = (rng.standard_normal(B) * 0.3 - 1.0).astype(f)
    adv = (rng.standard_normal(B) * 5.0 + 0.3).astype(f)
    ret = (rng.standard_normal(B) * 10).astype(f)
    val = (ret + rng.standard_normal(B) * 0.3).astype(f)  # value-clip: both branches
    return (obs, act, logp, adv, ret, val), rng.permutation(B).astype(np.int64)


@functools.lru_cache(maxsize=None)
def ppo_case(mb, D):
    """One (mb, D) case, computed once and shared: the batch, its permutation and
    per minibatch the float64 (gradient, approx_kl)."""
    batch, perm = ppo_batch(2 * mb, D, seed=100 * mb + D)
    ag = tail_agent(D)
    refs = [ppo_loss_grad_ref(ag, batch, perm[m * mb:(m + 1) * mb], PPO_CLIP, PPO_ENT, PPO_VF) for m in range(2)]
    for g, _ in refs:
        g.setflags(write=False)
    return batch, perm, refs


# advantage statistics
ADV_MB = (1, 2, 100, 1500, 3000)
ADV_N_MB = 3
# The cancellation case's bound on the std.  q and a^2 / n are ~ n 1e6 while their
# difference is ~ n 1e-4, so one float64 rounding of either (2^-53 relative) is
# 1e10 * 1.1e-16 = 1.1e-6 of the variance.  Measured on the host
# (test_update_ref_cpu.py): the float64 moment formula is within 1.03e-6 of the
# two-pass std on these inputs, so it meets 1.1e-6; the kernels get twice that.
ADV_OFFSET_STD_RTOL = 2.2e-6


def adv_inputs(mb, offset=False):
    """Advantages of n_mb = 3 minibatches and their permutation; offset: 1000 +
    0.01 sigma, the cancellation case of q - a * mean."""
    rng = np.random.default_rng(7000 + mb + int(offset))
    B = ADV_N_MB * mb
    x = rng.standard_normal(B)
    adv = (1000.0 + 0.01 * x if offset else 5.0 * x + 0.3).astype(np.float32)
    return adv, rng.permutation(B).astype(np.int64)


def moment_std(x):
    """The kernels' formula in float64: sqrt(max(q - a * (a / n), 0) / (n - 1)) of float32 inputs."""
    x = np.asarray(x, dtype=np.float64)
    a, q, n = x.sum(), (x * x).sum(), x.size
    return math.sqrt(max(q - a * (a / n), 0.0) / (n - 1))
