"""The bf16 policy kernels' arithmetic restated on the host ("The
bf16 contract"): float64 with round-to-nearest-even bf16 rounding at exactly
the matrix operands the kernels round, for tests/test_bf16_ref_cpu.py and
tests/test_bf16_exact_gpu.py.  Plain numpy; nothing here calls librx, and the
torch Agent is only read for its parameters.

Forward, per trunk (csrc/rx_policy_mfma.h, mlp_forward<.., kBF16> / mlp_forward_frag):
    z1 = bf(X) bf(W1)^T + b1, H1 = tanh(z1);  z2 = bf(H1) bf(W2)^T + b2, H2 = tanh(z2);
    y = bf(H2) bf(W3)^T;  actor mu = tanh(y + b3), critic v = y + b3.
Head gradient: head_grad (csrc/rx_ppo.hip) as written, no rounding.
Backward (ppo_grad_trunk_bf):
    dZ2 = (W3^T g) (1 - H2^2)                       W3, g, H2 unrounded
    dW3 = bf(g)^T bf(H2),   db3 = sum bf(g)
    dW2 = bf(dZ2)^T bf(H1), db2 = sum bf(dZ2)
    dZ1 = (bf(W2)^T bf(dZ2)) (1 - H1^2)             H1 unrounded
    dW1 = bf(dZ1)^T bf(X),  db1 = sum bf(dZ1)
Biases are never rounded; everything not listed is float32 in the kernels and
unrounded here.  SITES names the 17 roundings; ``sites`` switches single ones
off and ``mutant`` applies one structural error, for the power checks of
test_bf16_ref_cpu.py.

dtype = np.float32 is the host TWIN: the same arithmetic in float32 -- every sum
a sequential float32 chain in the REVERSE order of its index (numpy's float64
matmul and the kernels' MFMA tiles are two other orders), tanh as
rx_policy::tanh_fast (tools/tanh_error.py's emulation: correctly rounded exp2
and reciprocal), exp / log correctly rounded.  It is built from elementwise
float32 operations only, so its results do not depend on a BLAS.  What the twin
differs from the float64 run by is what a correct float32 kernel may differ by:
every tolerance below is 4 x a twin error recorded here.
"""
import functools
import math

import numpy as np

from tests import update_ref as ur

# ------------------------------------------------------------------ bf16 rounding
_BF_BITS = 8          # significant bits (1 implicit + 7 stored)
_BF_MIN_EXP = -125    # frexp exponent of the smallest normal, 2^-126 = 0.5 * 2^-125
_BF_MAX = float(2.0 ** 128 - 2.0 ** 120)  # largest finite bf16


def bf16_round(x):
    """x (float64 or float32, any shape) rounded to the nearest bf16, ties to even,
    in ONE rounding from the input's own precision and returned in its dtype.
    x = m 2^e with 0.5 <= |m| < 1 has the bf16 quantum 2^(e - 8) (2^-133 below the
    smallest normal: bf16 subnormals are covered); x / quantum is exact, rint is
    round-half-even, and the product back is exact.  Past the largest finite
    bf16's upper midpoint the result is +-inf; NaN and +-inf pass through."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    with np.errstate(invalid="ignore", over="ignore"):
        _, e = np.frexp(x)
        qe = np.maximum(e, _BF_MIN_EXP) - _BF_BITS
        r = np.ldexp(np.rint(np.ldexp(x, -qe)), qe)
        r = np.where(np.abs(r) > _BF_MAX, np.copysign(np.inf, x), r)
        r = np.where(np.isfinite(x), r, x)
    return r.astype(x.dtype)


def midpoint_distance(h):
    """(distance of |h| to the bf16 rounding midpoint of its own binade's grid cell,
    the cell's width q): float64, h != 0 normal."""
    h = np.abs(np.asarray(h, dtype=np.float64))
    _, e = np.frexp(h)
    q = np.ldexp(1.0, np.maximum(e, _BF_MIN_EXP) - _BF_BITS)
    t = h / q
    return np.abs(t - np.floor(t) - 0.5) * q, q


# ------------------------------------------------------------------ the contract
FWD_SITES = ("x", "w1", "h1", "w2", "h2", "w3")
BWD_SITES = ("dw3_g", "dw3_h2", "db3_g", "dw2_dz2", "dw2_h1", "db2_dz2", "dz1_w2", "dz1_dz2", "dw1_dz1", "dw1_x",
             "db1_dz1")
SITES = FWD_SITES + BWD_SITES
ALL = frozenset(SITES)
NONE = frozenset()
assert len(SITES) == 17
TENSORS = ("aW1", "ab1", "aW2", "ab2", "aW3", "ab3", "cW1", "cb1", "cW2", "cb2", "cW3", "cb3")  # Lay<D> order
# the parameter tensors (of either trunk) a rounding site feeds: forward sites feed all of them
FEEDS = {s: ("W1", "b1", "W2", "b2", "W3", "b3") for s in FWD_SITES}
FEEDS.update(dw3_g=("W3",), dw3_h2=("W3",), db3_g=("b3",), dw2_dz2=("W2",), dw2_h1=("W2",), db2_dz2=("b2",),
             dz1_w2=("W1", "b1"), dz1_dz2=("W1", "b1"), dw1_dz1=("W1",), dw1_x=("W1",), db1_dz1=("b1",))
MUTANTS = ("drop_cols16", "ones_zero", "absent_through", "div_live")
_HALF_LOG_2PI = 0.91893853320467274178


def tensor_slices(D):
    sizes = [64 * D, 64, 64 * 64, 64, 2 * 64, 2, 64 * D, 64, 64 * 64, 64, 64, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    return {k: slice(int(a), int(b)) for k, a, b in zip(TENSORS, offs[:-1], offs[1:])}


def trunks_of(agent):
    """(actor, critic) dicts of float64 W1 [64, D], b1, W2, b2, W3 [n_out, 64], b3 and the float64 log_std."""
    out = []
    for seq in (agent.actor_mu, agent.critic):
        t = {}
        for k, i in ((1, 0), (2, 2), (3, 4)):
            t[f"W{k}"] = seq[i].weight.detach().cpu().double().numpy()
            t[f"b{k}"] = seq[i].bias.detach().cpu().double().numpy()
        out.append(t)
    return out[0], out[1], agent.log_std.detach().cpu().double().numpy()


def _tanh_fast32(x):
    """rx_policy::tanh_fast on float32 (csrc/rx_policy.h; tools/tanh_error.py)."""
    f = np.float32
    ax = np.abs(x)
    with np.errstate(over="ignore"):
        e = np.exp2((ax * f(2.8853900817779268)).astype(np.float64)).astype(f)
        r = (f(1) / (e + f(1))).astype(f)
    t = np.copysign((r * f(-2) + f(1)).astype(f), x)  # fmaf(r, -2, 1): the product by 2 is exact
    return np.where(ax < f(2.0 ** -12), x, t).astype(f)


class _Arith:
    """float64: numpy's own sums.  float32: reverse-order sequential chains."""

    def __init__(self, dtype):
        self.f = np.dtype(dtype).type
        assert self.f in (np.float32, np.float64)
        self.twin = self.f is np.float32

    def arr(self, x):
        return np.asarray(x, dtype=self.f)

    def mm(self, a, b):
        """a [n, k] @ b [k, m]"""
        if not self.twin:
            return a @ b
        acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
        for k in reversed(range(a.shape[1])):
            acc += a[:, k, None] * b[None, k, :]
        return acc

    def colsum(self, a):
        if not self.twin:
            return a.sum(0)
        acc = np.zeros(a.shape[1], dtype=np.float32)
        for k in reversed(range(a.shape[0])):
            acc += a[k]
        return acc

    def tanh(self, x):
        return _tanh_fast32(x) if self.twin else np.tanh(x)

    def exp(self, x):
        return np.exp(np.asarray(x, dtype=np.float64)).astype(self.f)

    def log(self, x):
        return np.log(np.asarray(x, dtype=np.float64)).astype(self.f)


def _trunk_forward(A, t, X, sites):
    r = lambda s, v: bf16_round(v) if s in sites else v  # noqa: E731
    W1, b1, W2, b2, W3 = (A.arr(t[k]) for k in ("W1", "b1", "W2", "b2", "W3"))
    z1 = A.mm(r("x", X), r("w1", W1).T) + b1
    H1 = A.tanh(z1)
    z2 = A.mm(r("h1", H1), r("w2", W2).T) + b2
    H2 = A.tanh(z2)
    y = A.mm(r("h2", H2), r("w3", W3).T)
    return H1, H2, y


def _normal_logp(A, diff, var, lsc):
    f = A.f
    return -(diff * diff) / (f(2) * var) - lsc - f(_HALF_LOG_2PI)


def _scales(A, log_std):
    scale = A.exp(A.arr(log_std))
    return scale, scale * scale, A.log(scale)


def policy_forward_bf16_ref(agent, obs, eps, dtype=np.float64, sites=ALL):
    """k_policy_act in bf16 precision: obs [n, D], eps [n, 2] (float32 values) ->
    (actions [n, 2], log-probs [n], values [n], the pre-clamp mu [n, 2]) in dtype."""
    A = _Arith(dtype)
    actor, critic, log_std = trunks_of(agent)
    X, eps = A.arr(obs), A.arr(eps)
    _, _, ya = _trunk_forward(A, actor, X, sites)
    _, _, yc = _trunk_forward(A, critic, X, sites)
    mu = A.tanh(ya + A.arr(actor["b3"]))
    scale, var, lsc = _scales(A, log_std)
    act = np.clip(eps * scale + mu, A.f(-1), A.f(1))
    logp = A.f(0) + _normal_logp(A, act[:, 0] - mu[:, 0], var[0], lsc[0])
    logp = logp + _normal_logp(A, act[:, 1] - mu[:, 1], var[1], lsc[1])
    return act, logp, yc[:, 0] + A.arr(critic["b3"])[0], mu


def hidden_activations(agent, obs, dtype=np.float64):
    """[n, 256]: the pre-rounding H1 and H2 of both trunks, the forward's rounding decisions."""
    A = _Arith(dtype)
    actor, critic, _ = trunks_of(agent)
    X = A.arr(obs)
    return np.concatenate([h for t in (actor, critic) for h in _trunk_forward(A, t, X, ALL)[:2]], axis=1)


# A row is FORWARD-FRAGILE when a pre-rounding H1 / H2 entry of either trunk lies
# within FRAGILE_EPS of a bf16 rounding midpoint: a correct float32 kernel may
# then round that operand the other way and move every later quantity by a bf16
# step (2^-9 relative of that entry), not by float32 rounding.
#   The float32 error of an entry: its pre-activation is a sum of <= 64 exact
# products (bf16 x bf16 fits float32's significand) plus a bias, and a
# sequential float32 chain rounds each of its <= 64 partial sums by at most half
# an ulp.  A partial sum in [0.5, 1) rounds by <= 2^-25 = 3.0e-8 (the
# pre-activations' rms is ~0.5), uniformly: standard deviation 1.7e-8, 1.4e-7 for
# the 64 of a chain; tanh' <= 1 passes at most that on, and tanh_fast adds <=
# 1.4e-7 (rx_policy.h): 2.8e-7 as the typical size.  FRAGILE_EPS = 1e-6 is 3.6
# times that.  It is a statistical bound, not the worst case: 64 half-ulps of
# partial sums up to 4 (7.6e-6) would call every row fragile, and the matrix
# cores round far fewer partial sums than a chain does.  The twin confirms it:
# its worst |H - H64| over the non-fragile rows of every input of these tests
# (no operand upstream of them can have flipped) is TWIN_H_ERR
# (test_bf16_ref_cpu.py prints and asserts it), a quarter of the bound.
FRAGILE_EPS = 1e-6
TWIN_H_ERR = 2.6e-7  # measured: worst twin-against-float64 hidden activation, non-fragile rows


def fragile_rows(agent, obs, eps=FRAGILE_EPS):
    return (midpoint_distance(hidden_activations(agent, obs))[0] < eps).any(1)


def adv_stats_of(adv, idx):
    """float64 (mean, unbiased std) over mb = len(idx) of rx_ppo_adv_stats: an absent row adds nothing."""
    idx = np.asarray(idx, dtype=np.int64)
    live = (idx >= 0) & (idx < adv.shape[0])
    a = np.zeros(idx.size)
    a[live] = np.asarray(adv, dtype=np.float64)[idx[live]]
    return a.mean(), (math.sqrt(((a - a.mean()) ** 2).sum() / (a.size - 1)) if a.size > 1 else 0.0)


def ppo_grad_bf16_ref(agent, batch, idx, clip_coef=ur.PPO_CLIP, vf_coef=ur.PPO_VF, dtype=np.float64, sites=ALL,
                      mutant=None, part_of=None):
    """k_ppo_grad_bf for the minibatch rows ``idx`` (an entry outside [0, n_rows)
    is an absent row: left out, the divisor stays mb = len(idx)) of batch = (obs,
    actions, logprobs, advantages, returns, values) -> (flat gradient in Lay<D>
    order, approx_kl, per-row diagnostics of the live rows), all float64 numpy /
    float whatever ``dtype`` computed them in.  The advantage statistics are those
    of rx_ppo_adv_stats (mean and unbiased std over mb, an absent row adding
    nothing), computed in float64 and rounded to dtype.  ``mutant``: one of MUTANTS.
    ``part_of``: the whole minibatch's index slice when idx is only a part of it
    (the statistics and the divisor are the whole minibatch's)."""
    assert mutant is None or mutant in MUTANTS
    A = _Arith(dtype)
    f = A.f
    actor, critic, log_std = trunks_of(agent)
    obs, act, oldlp, adv, ret, val = batch
    n_rows, D = obs.shape
    idx = np.asarray(idx, dtype=np.int64)
    whole = idx if part_of is None else np.asarray(part_of, dtype=np.int64)
    mb = whole.size
    live = (idx >= 0) & (idx < n_rows)
    mean, sd = (f(x) for x in adv_stats_of(adv, whole))
    src = idx % n_rows if mutant == "absent_through" else idx[live]
    invM = f(1) / f(src.size if mutant == "div_live" else mb)
    X = A.arr(obs[src])
    if mutant == "drop_cols16":
        X = X.copy()
        X[:, 16:] = 0
    act, oldlp, adv, ret, val = (A.arr(x[src]) for x in (act, oldlp, adv, ret, val))
    clip, lo, hi = f(clip_coef), f(1) - f(clip_coef), f(1) + f(clip_coef)
    rnd = lambda s, v: bf16_round(v) if s in sites else v  # noqa: E731

    ops, budgets = {}, {}

    def backward(name, t, H1, H2, g, bud_g):
        W2, W3 = A.arr(t["W2"]), A.arr(t["W3"])
        dh2 = A.mm(g, W3)
        dZ2 = dh2 * (f(1) - H2 * H2)
        dW3 = A.mm(rnd("dw3_g", g).T, rnd("dw3_h2", H2))
        db3 = A.colsum(rnd("db3_g", g))
        dW2 = A.mm(rnd("dw2_dz2", dZ2).T, rnd("dw2_h1", H1))
        db2 = A.colsum(rnd("db2_dz2", dZ2))
        zr, wr = rnd("dz1_dz2", dZ2), rnd("dz1_w2", W2)
        dh1 = A.mm(zr, wr)
        dZ1 = dh1 * (f(1) - H1 * H1)
        dW1 = A.mm(rnd("dw1_dz1", dZ1).T, rnd("dw1_x", X))
        db1 = A.colsum(rnd("db1_dz1", dZ1))
        if mutant == "ones_zero":
            db1 = np.zeros_like(db1)
        ops.update({f"g_{name}": g, f"dZ2_{name}": dZ2, f"dZ1_{name}": dZ1})
        if bud_g is not None:  # first-order float32 error budgets of the three operands (OPERAND BUDGETS below)
            budgets[f"g_{name}"] = bud_g
            budgets[f"dZ2_{name}"] = ((bud_g @ np.abs(W3)) * (1 - H2 * H2) + np.abs(dh2) * 2 * np.abs(H2) * ACT_ERR
                                      + 4 * _U * np.abs(dZ2))
            budgets[f"dZ1_{name}"] = (8 * _U * (np.abs(zr) @ np.abs(wr)) * (1 - H1 * H1)
                                      + np.abs(dh1) * 2 * np.abs(H1) * ACT_ERR + 4 * _U * np.abs(dZ1))
        return [dW1, db1, dW2, db2, dW3, db3]

    want_budgets = not A.twin and sites == ALL and mutant is None
    # actor: clipped surrogate (head_grad<0>)
    H1, H2, y = _trunk_forward(A, actor, X, sites)
    mu = A.tanh(y + A.arr(actor["b3"]))
    _, var, lsc = _scales(A, log_std)
    diff = act - mu
    logp = f(0) + _normal_logp(A, diff[:, 0], var[0], lsc[0])
    logp = logp + _normal_logp(A, diff[:, 1], var[1], lsc[1])
    An = (adv - mean) / (sd + f(1e-8))
    ratio = A.exp(logp - oldlp)
    u1, u2 = -An * ratio, -An * np.clip(ratio, lo, hi)
    g1 = np.where(u1 > u2, f(1), np.where(u1 == u2, f(0.5), f(0)))  # torch.max splits ties
    inr = ((ratio >= lo) & (ratio <= hi)).astype(f)
    dlogp = invM * (g1 * -An + (f(1) - g1) * -An * inr) * ratio
    g = dlogp[:, None] * diff / var * (f(1) - mu * mu)
    bud = None
    if want_budgets:
        rel_logp = (np.abs(diff) / var).sum(1) * ACT_ERR + 8 * _U * (1 + np.abs(logp) + np.abs(oldlp))
        with np.errstate(divide="ignore"):
            rel = rel_logp[:, None] + ACT_ERR / np.abs(diff) + 2 * np.abs(mu) * ACT_ERR / (1 - mu * mu) + 8 * _U
        bud = np.where(g == 0, 0.0, np.abs(g) * rel)
    grads = backward("actor", actor, H1, H2, g, bud)
    kl = float((oldlp - logp).astype(np.float64).sum()) / mb
    # critic: clipped value loss (head_grad<1>)
    H1c, H2c, yc = _trunk_forward(A, critic, X, sites)
    v = yc[:, 0] + A.arr(critic["b3"])[0]
    vd = v - val
    vc = val + np.clip(vd, -clip, clip)
    e1, e2 = v - ret, vc - ret
    q1, q2 = e1 * e1, e2 * e2
    gq1 = np.where(q1 > q2, f(1), np.where(q1 == q2, f(0.5), f(0)))
    vin = ((vd >= -clip) & (vd <= clip)).astype(f)
    gv = f(vf_coef) * f(0.5) * invM * (gq1 * f(2) * e1 + (f(1) - gq1) * f(2) * e2 * vin)
    if want_budgets:  # d gv / d v = vf / mb on the unclipped branch and inside the clip, 0 on the clipped one
        bud = ((vf_coef / mb * ACT_ERR) * ((gq1 > 0) | (vin > 0)) + 8 * _U * np.abs(gv))[:, None]
    grads += backward("critic", critic, H1c, H2c, gv[:, None], bud)
    flat = np.concatenate([x.reshape(-1) for x in grads]).astype(np.float64)
    rows = dict(logp=logp, mu=mu, value=v, ratio=ratio, An=An, u1_minus_u2=u1 - u2, vd=vd, q1_minus_q2=q1 - q2)
    rows = {k: np.asarray(x, dtype=np.float64) for k, x in rows.items()}
    rows.update(src=src, ops={k: np.asarray(x, dtype=np.float64) for k, x in ops.items()}, budgets=budgets)
    return flat, kl, rows


# OPERAND BUDGETS.  The backward's matrix operands g, dZ2 and dZ1 are rounded to
# bf16 too, and a kernel whose float32 value of one of them falls on the other
# side of a rounding midpoint moves a gradient tensor by a bf16 step of that
# entry (~1e-4 .. 1e-3 of the tensor's max), three orders above float32 rounding.
# With such flips left to chance the twin's error, and so the tolerance, is a
# coin toss per tensor.  So the float64 run also bounds, to first order, what a
# float32 evaluation may differ by at every operand entry, from ACT_ERR (the
# bound on H, mu and the value: FRAGILE_EPS) and the unit roundoff u = 2^-24:
#   log-prob       sum_j |a_j - mu_j| / var_j ACT_ERR + 8 u (1 + |logp| + |old logp|)
#   g (actor)      |g| (that + ACT_ERR / |a_j - mu_j| + 2 |mu_j| ACT_ERR / (1 - mu_j^2) + 8 u)
#   g (critic)     vf / mb ACT_ERR where the value enters (not on the clipped branch) + 8 u |g|
#   dZ2            (budget(g) |W3|) (1 - H2^2) + |W3^T g| 2 |H2| ACT_ERR + 4 u |dZ2|
#   dZ1            8 u (|bf dZ2| |bf W2|) (1 - H1^2) + |W2^T dZ2| 2 |H1| ACT_ERR + 4 u |dZ1|
#                  (8 = sqrt(64): the 64-term sum of exact products, as FRAGILE_EPS counts it)
# A row is BACKWARD-FRAGILE when an operand entry lies within its budget of a
# rounding midpoint.  The gradient batches redraw such rows like the
# forward-fragile ones, so neither the twin nor a correct kernel flips an operand
# and the twin's error is float32 rounding alone.  test_bf16_ref_cpu.py checks the
# budgets against the twin: its worst |operand - float64 operand| / budget.
_U = 2.0 ** -24
ACT_ERR = FRAGILE_EPS


def backward_fragile(rows):
    """[live rows] bool: an operand entry of the float64 run within its budget of a bf16 rounding midpoint."""
    bad = np.zeros(rows["src"].size, dtype=bool)
    for k, b in rows["budgets"].items():
        bad |= (midpoint_distance(rows["ops"][k])[0] < b).any(1)
    return bad


def tensor_errors(got, want, D):
    """{tensor: max |got - want| / max |want|} per parameter tensor."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return {k: float(np.abs(got[s] - want[s]).max() / np.abs(want[s]).max()) for k, s in tensor_slices(D).items()}


# ---------------------------------------------------------------------- inputs
GRAD_MB = (2, 24, 100, 800)
GRAD_D = (15, 19)
FWD_N = (1, 16, 17, 65, 4099)
FWD_POOL = FWD_N[-1]
FWD_EPS_SCALE = (0.0, 1.5)  # eps = 0 (action = mu) and 1.5 x N(0, 1) (clamped samples)
FRAGILE_QUOTA = 0.01        # the share of forward-fragile rows a forward batch keeps
# decision margins of the gradient batches (relative for the ratio, absolute otherwise)
RATIO_MARGIN, ADV_MARGIN, VD_MARGIN, Q_MARGIN = 1e-3, 1e-2, 1e-3, 1e-3
_RATIO_CLASSES = ((0.55, 0.79), (0.81, 1.19), (1.21, 1.6))       # below / inside / above 1 +- clip
_VD_CLASSES = ((-0.5, -0.21), (-0.19, 0.19), (0.21, 0.5))        # v - old value against +- clip


def _draw_obs(rng, n, D):
    return (rng.random((n, D)) * 2 - 1).astype(np.float32)


def _redraw_fragile(agent, obs, rng, keep=()):
    """Redraws the forward-fragile rows of obs (all but the rows in ``keep``) until none is left."""
    keep = np.asarray(keep, dtype=np.int64)
    for _ in range(200):
        bad = fragile_rows(agent, obs)
        bad[keep] = False
        if not bad.any():
            return obs
        obs[bad] = _draw_obs(rng, int(bad.sum()), obs.shape[1])
    raise AssertionError("fragile rows left")


@functools.lru_cache(maxsize=None)
def forward_case(D):
    """The forward pool of one D: FWD_POOL observation rows (a test at n rows reads
    the first n), the N(0, 1) block eps is scaled from, and the fragile mask.
    Uniform rows are forward-fragile far more often than the quota (``natural``
    keeps the rows as drawn, ``natural_fragile`` their mask: the twin's flip error
    is measured there, on some 3,000 fragile rows): the pool keeps fragile rows at
    an even spacing up to the quota, the first kept one moved to row 0 so that
    every n has one, and redraws the others until they are not fragile."""
    rng = np.random.default_rng(7100 + D)
    agent = ur.tail_agent(D)
    obs = _draw_obs(rng, FWD_POOL, D)
    noise = rng.standard_normal((FWD_POOL, 2)).astype(np.float32)
    natural = obs.copy()
    natural_fragile = fragile_rows(agent, obs)
    frag = np.flatnonzero(natural_fragile)
    quota = int(FRAGILE_QUOTA * FWD_POOL)
    keep = frag[np.linspace(0, frag.size - 1, min(quota, frag.size)).astype(np.int64)]
    obs[[0, keep[0]]] = obs[[keep[0], 0]]
    keep[0] = 0
    obs = _redraw_fragile(agent, obs, rng, keep)
    mask = fragile_rows(agent, obs)
    assert np.array_equal(np.flatnonzero(mask), np.sort(keep))
    for x in (obs, noise, mask, natural, natural_fragile):
        x.setflags(write=False)
    return dict(agent=agent, obs=obs, noise=noise, fragile=mask, natural=natural, natural_fragile=natural_fragile)


def forward_eps(case, scale, n=FWD_POOL):
    """The eps block of the first n pool rows: scale x the case's N(0, 1) draws, float32."""
    return (case["noise"][:n] * np.float32(scale)).astype(np.float32)


def forward_errors(got, want):
    """{output: [n] |got - want|} of (actions, log-probs, values, ...) tuples; an
    action row's error is the larger of its two."""
    out = {}
    for k, a, b in zip(("actions", "logprobs", "values"), got, want):
        e = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
        out[k] = e.reshape(e.shape[0], -1).max(1)
    return out


def _act_logp(agent, obs, noise):
    """The float64 reference's forward of rows obs: the action mu + std * noise
    clamped and stored in float32, its log-prob, and the value."""
    A = _Arith(np.float64)
    actor, critic, log_std = trunks_of(agent)
    X = A.arr(obs)
    mu = np.tanh(_trunk_forward(A, actor, X, ALL)[2] + actor["b3"])
    scale, var, lsc = _scales(A, log_std)
    act = np.clip(mu + scale * noise, -1, 1).astype(np.float32)
    diff = act - mu
    logp = _normal_logp(A, diff[:, 0], var[0], lsc[0]) + _normal_logp(A, diff[:, 1], var[1], lsc[1])
    return act, logp, _trunk_forward(A, critic, X, ALL)[2][:, 0] + critic["b3"][0]


def _grad_batch(mb, D, seed, absent):
    """B = 2 mb rows and their permutation (absent: half of minibatch 1's slice
    replaced by -1 and by entries >= B).  The actions are rollout-like (mu + std
    N(0, 1), clamped); the old log-probs, old values and returns are placed
    around the float64 reference's own forward so that every discrete decision of
    head_grad has a margin: row k of a minibatch takes ratio class k % 3 (below /
    inside / above 1 +- clip) with advantage sign (k // 3) % 2, and value class
    k % 5 (below the clip with the unclipped, then the clipped error the larger;
    inside; above likewise).  Rows that are forward- or backward-fragile are
    redrawn (observation and action; the advantage stays, so the minibatch
    statistics and every other row's gradient stay) until none is left."""
    rng = np.random.default_rng(seed)
    agent = ur.tail_agent(D)
    B = 2 * mb
    f = np.float32
    perm = rng.permutation(B).astype(np.int64)
    k = np.empty(B, dtype=np.int64)
    k[perm] = np.arange(B) % mb  # position within its minibatch
    if absent:
        perm[mb::4] = -1
        perm[mb + 1::4] = B + 7 * np.arange(perm[mb + 1::4].size)
    rc = np.array(_RATIO_CLASSES)[k % 3]
    sign = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    adv = (0.3 + sign * 5.0 * (0.5 + np.abs(rng.standard_normal(B)))).astype(f)
    vcls = k % 5
    vr = np.array(_VD_CLASSES)[np.array([0, 0, 1, 2, 2])[vcls]]
    r_side = np.where(np.isin(vcls, (0, 3)), 1.0, -1.0)
    obs = np.empty((B, D), dtype=f)
    act = np.empty((B, 2), dtype=f)
    oldlp, val, ret = np.empty(B, dtype=f), np.empty(B, dtype=f), np.empty(B, dtype=f)
    todo = np.arange(B)
    for _ in range(500):
        n = todo.size
        obs[todo] = _draw_obs(rng, n, D)
        act[todo], logp, v = _act_logp(agent, obs[todo], rng.standard_normal((n, 2)))
        oldlp[todo] = logp - np.log(rc[todo, 0] + rng.random(n) * (rc[todo, 1] - rc[todo, 0]))
        val[todo] = v - (vr[todo, 0] + rng.random(n) * (vr[todo, 1] - vr[todo, 0]))
        vd = v - val[todo].astype(np.float64)
        vc = val[todo] + np.clip(vd, -ur.PPO_CLIP, ur.PPO_CLIP)
        # q1 - q2 = (v - vc) (v + vc - 2 R): R on either side of (v + vc) / 2, 0.3 .. 3 away
        ret[todo] = (v + vc) / 2 + r_side[todo] * (0.3 + 2.7 * rng.random(n))
        batch = (obs, act, oldlp, adv, ret, val)
        bad = np.zeros(B, dtype=bool)
        bad[todo[fragile_rows(agent, obs[todo])]] = True
        for m in range(2):
            whole = perm[m * mb:(m + 1) * mb]
            rows = ppo_grad_bf16_ref(agent, batch, whole[np.isin(whole, todo)], part_of=whole)[2]
            bad[rows["src"][backward_fragile(rows)]] = True
        todo = np.flatnonzero(bad)
        if todo.size == 0:
            return agent, batch, perm
    raise AssertionError("fragile rows left")


@functools.lru_cache(maxsize=None)
def grad_case(mb, D, absent=False):
    """One gradient case, computed once and shared: agent, batch, perm and per
    minibatch the float64 (gradient, approx_kl, row diagnostics)."""
    agent, batch, perm = _grad_batch(mb, D, 9000 + 100 * mb + D + 50 * absent, absent)
    refs = [ppo_grad_bf16_ref(agent, batch, perm[m * mb:(m + 1) * mb]) for m in range(2)]
    for x in batch + (perm,) + tuple(r[0] for r in refs):
        x.setflags(write=False)
    return dict(agent=agent, batch=batch, perm=perm, refs=refs, mb=mb, D=D)


def grad_cases():
    """(mb, D, absent) of every gradient case of the CPU and the GPU tests."""
    return [(mb, D, False) for mb in GRAD_MB for D in GRAD_D] + [(100, D, True) for D in GRAD_D]


def decision_margins(rows, clip=ur.PPO_CLIP):
    """Smallest distance of a minibatch's rows from each discrete decision of
    head_grad, and how many rows took each branch: ratio below / inside / above the
    clip by the sign of the normalised advantage; value difference below / inside /
    above the clip, outside it by the larger squared error."""
    ratio, An, vd, qd = rows["ratio"], rows["An"], rows["vd"], rows["q1_minus_q2"]
    rcls = np.where(ratio < 1 - clip, 0, np.where(ratio > 1 + clip, 2, 1))
    vcls = np.where(vd < -clip, 0, np.where(vd > clip, 2, 1))
    out = np.abs(vcls - 1) == 1
    counts = {f"ratio{'<=>'[c]} A{'-+'[s]}": int(((rcls == c) & ((An > 0) == bool(s))).sum())
              for c in range(3) for s in range(2)}
    counts.update({"vd inside": int((vcls == 1).sum())})
    counts.update({f"vd{'< >'[c]} q1{'<>'[s]}q2": int(((vcls == c) & ((qd > 0) == bool(s))).sum())
                   for c in (0, 2) for s in range(2)})
    margins = dict(ratio=float(np.minimum(np.abs(ratio / (1 - clip) - 1), np.abs(ratio / (1 + clip) - 1)).min()),
                   adv=float(np.abs(An).min()),
                   vd=float(np.minimum(np.abs(vd + clip), np.abs(vd - clip)).min()),
                   q=float(np.abs(qd[out]).min()) if out.any() else float("inf"))
    return margins, counts


# ------------------------------------------------- recorded twin errors, tolerances
# Measured on the host by tests/test_bf16_ref_cpu.py (which asserts that they still
# hold and are not stale) and listed in DESIGN.md §4.  Nothing here comes from a
# kernel.  Every tolerance is 4 x the twin's worst error over all cases: the factor
# covers the kernels' own (third) summation order and tanh_fast on the hardware's
# exp2 / reciprocal, which the twin emulates correctly rounded.
#
# Gradient: per parameter tensor, max |error| / that tensor's max |g|.  The bias
# gradients of layers 2 and 3 are sums of bf16 values that float32 holds exactly
# on these inputs, so the twin's error there is 0; TWIN_FLOOR, one float32 ulp at
# the tensor's largest entry (the resolution of a float32 accumulator), stands in
# for a twin error below it.
TWIN_FLOOR = 2.0 ** -23
TWIN_GRAD_ERR = dict(aW1=3.2e-7, ab1=3.3e-8, aW2=3.6e-7, ab2=0.0, aW3=4.2e-7, ab3=0.0,
                     cW1=2.2e-7, cb1=1.1e-8, cW2=2.1e-7, cb2=0.0, cW3=2.4e-7, cb3=0.0)
GRAD_TOL = {k: 4 * max(v, TWIN_FLOOR) for k, v in TWIN_GRAD_ERR.items()}
TWIN_KL_ERR = 1.7e-7  # approx_kl, absolute
KL_TOL = 4 * TWIN_KL_ERR
# Forward: absolute error per row, (non-fragile rows, fragile rows)
TWIN_FWD_ERR = dict(actions=(1.7e-7, 5.4e-4), logprobs=(1.5e-6, 2.8e-3), values=(1.9e-7, 1.9e-3))
FWD_TOL = {k: (4 * a, 4 * b) for k, (a, b) in TWIN_FWD_ERR.items()}
