"""CPU check of the raycast's float32 box test (rx_kernels.hip: rays_wave's operand setup,
chunk_needed_f, chunk_needed_q, slab_keep, f32_up; rx_cull.h: rx_cull_f32_down / _up,
rx_cull_quadrant), emulated here operation by operation in numpy: every float32 operation
rounds as the kernel's (float32 array arithmetic; ``fma32`` is an exactly rounded fused
multiply-add; np.fmin / np.fmax are fminf / fmaxf), every float64 one as -ffp-contract=off
leaves it.  The exact side is seg_test as tests/test_prefilter_cpu.py's ``exact_hit`` states
it, plus t = C / D.

Property 1 (the box test is conservative).  For a ray and a segment that the exact test hits
at t, ANY axis-aligned box that holds both end points of the segment -- the segment's own box,
and that box padded to the size of a chunk's, a face through the origin or 1e-9 beside it on a
third of the rows -- rounded outward to float32, and ANY bound best > t (inf, nextafter(t),
t (1 + 1e-12), t + 1): the box test keeps the box, in the plain form and in the quadrant-ordered
one, with id2 as the build divides (below) and moved by +-2 ulps (the derivation grants
6 * 2^-24 relative on a slab end point).

Property 2.  chunk_needed_q decides as chunk_needed_f on every input (the lanes of a wave that
takes the quadrant form share the quadrant; a lane alone always does).

The inputs put the magnitudes where the margins decide (DESIGN.md §4 "Placed tracks"): slot
centres 0, (1e3, -1e3), (2^17, 2^17), (-2^20, 3 * 2^18), (2^26, -2^26); slot radii 4 .. 8000;
segments of 0.05 .. 300; origins inside the slot circle and up to 100 radii outside, t from
exactly 0 up; hits near an end point (a corner of the segment's box), axis-parallel segments
(a box of no height: every entry grazes), segments at 1.2e-10 / L .. 1e-4 to the ray (|dotp|
from just above the 1e-10 cut, where the computed t and s err most); directions random, k pi / 2 and their 1-ulp
neighbours, and unit vectors with a component of exactly +0.0 / -0.0.

The build's float32 division.  rx/_build.py compiles with -O3 -ffp-contract=off and no
fast-math flag, and hipcc's default for HIP device code is
-fhip-fp32-correctly-rounded-divide-sqrt: `1.0f / d` is the correctly rounded quotient
(v_div_scale_f32 / v_div_fmas_f32 / v_div_fixup_f32 in rays_wave's code, not a bare
v_rcp_f32).  The emulation divides in float32 -- correctly rounded -- and
test_build_divides_correctly_rounded holds the flags to that.

Mutation record (this file's inputs, seed 5; required keeps = exact hits x 2 boxes x 4 bounds
x 2 forms = 3,848,080 on 240,505 exact hits of 300,000 rows; `python -m tests.test_slab_cpu`
prints it, per slot centre in the order above):
  shipped rules, id2 as divided / - 2 ulps / + 2 ulps   lose 0 / 0 / 0;
  without open_axes (id = 0, offsets left at n * 0)       loses 407,160
                                                          (85,000 / 85,440 / 86,544 / 86,480 / 63,696);
  without the |ox| + |oy| terms of mbf0 and mbf           loses 162,488
                                                          (0 / 908 / 15,892 / 29,326 / 116,362);
  mb and mt without their factor 1e10 (the 1 / 1e-10      loses 56
  of the |dotp| cut)                                      (44 / 8 / 4 / 0 / 0).
The second mutant loses nothing at the origin-centred slot -- where every GPU test stood before
the placed tracks -- and most at 2^26, where float32 resolves positions to 8 units only.  The
third is caught by the grazing segments alone (|dotp| just above 1e-10: the computed hit lies
up to eps_s |v2| off the segment), and only where the coordinate terms do not cover for it.
Finer mutants lose nothing on these inputs: the slack k = 0, mbf without its 2^-22 term or with
its factor 3 at 1, no clamp at -mtf, bm without mtf -- the margins have that much room.
"""
import numpy as np

from tests.test_prefilter_cpu import exact_hit

F = np.float32
D = np.float64
INF32 = F(np.inf)
CENTRES = ((0.0, 0.0), (1e3, -1e3), (2.0 ** 17, 2.0 ** 17), (-2.0 ** 20, 3 * 2.0 ** 18), (2.0 ** 26, -2.0 ** 26))
PER_CENTRE = 60_000
HALF_PI = np.pi / 2


# ------------------------------------------------------------------------------ float32 pieces
def fma32(a, b, c):
    """float32 fma, exactly rounded: the product of two float32 is exact in float64; the sum with c
    is rounded to odd in float64 (TwoSum gives the error's sign), which the final rounding to
    float32 cannot tell from the exact sum (53 >= 24 + 2 bits)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, D) * np.asarray(b, D)
        c = np.broadcast_to(np.asarray(c, D), p.shape)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def f32_up(x):
    """rx_kernels.hip f32_up / rx_cull.h rx_cull_f32_up: the smallest float32 >= x."""
    with np.errstate(over="ignore"):
        f = np.asarray(x, D).astype(F)
    return np.where(f.astype(D) < x, np.nextafter(f, INF32), f)


def f32_down(x):
    """rx_cull.h rx_cull_f32_down."""
    with np.errstate(over="ignore"):
        f = np.asarray(x, D).astype(F)
    return np.where(f.astype(D) > x, np.nextafter(f, -INF32), f)


def box_f32(b):
    """rx_cull_box_f32: [n, 4] float64 (x0, y0, x1, y1) rounded outward."""
    return np.stack([f32_down(b[:, 0]), f32_down(b[:, 1]), f32_up(b[:, 2]), f32_up(b[:, 3])], 1)


def quadrant_box(q, f):
    """rx_cull_quadrant per row: (near.x, near.y, far.x, far.y) for direction quadrant q."""
    nx, ny = (q & 1) != 0, (q & 2) != 0
    return np.stack([np.where(nx, f[:, 2], f[:, 0]), np.where(ny, f[:, 3], f[:, 1]),
                     np.where(nx, f[:, 0], f[:, 2]), np.where(ny, f[:, 1], f[:, 3])], 1)


def slab_keep(lo, hi, bm):
    k = F(2.0 ** -20)
    x = fma32(-np.abs(lo), k, lo)  # v_fma_f32 x, -|lo|, k, lo
    y = fma32(np.abs(hi), k, hi)   # v_fma_f32 y, |hi|, k, hi
    with np.errstate(invalid="ignore"):
        return ~((x - y) > F(1e-6)) & (x < bm)


def chunk_needed_f(box, ops, bm):
    (clx, cly), (chx, chy), (idx, idy) = ops["clo"], ops["chi"], ops["id2"]
    t1x, t1y = fma32(box[:, 0], idx, clx), fma32(box[:, 1], idy, cly)
    t2x, t2y = fma32(box[:, 2], idx, chx), fma32(box[:, 3], idy, chy)
    lo = np.fmax(np.fmax(np.fmin(t1x, t2x), np.fmin(t1y, t2y)), -ops["mtf"])
    hi = np.fmin(np.fmax(t1x, t2x), np.fmax(t1y, t2y))
    return slab_keep(lo, hi, bm)


def chunk_needed_q(box, ops, bm):
    """box: the rows' own quadrant block (quadrant_box(ops["quad"], .))."""
    (cnx, cny), (cfx, cfy), (idx, idy) = ops["cn"], ops["cf"], ops["id2"]
    tnx, tny = fma32(box[:, 0], idx, cnx), fma32(box[:, 1], idy, cny)
    tfx, tfy = fma32(box[:, 2], idx, cfx), fma32(box[:, 3], idy, cfy)
    lo = np.fmax(np.fmax(tnx, tny), -ops["mtf"])
    hi = np.fmin(tfx, tfy)
    return slab_keep(lo, hi, bm)


def operands(r, id_ulps=0, open_axes=True, origin_terms=True, cut_factor=1e10):
    """rays_wave's float32 box-test operands of rows r (ox, oy, cs, sn and the slot's cx, cy, rad, L).
    id_ulps: id2 moved by that many float32 ulps; open_axes / origin_terms False, cut_factor 1: the mutants."""
    ox, oy, cx, cy, rad, L = (r[k] for k in ("ox", "oy", "cx", "cy", "rad", "L"))
    ddx, ddy = ox - cx, oy - cy
    Rr = np.sqrt(ddx * ddx + ddy * ddy) + rad
    T = Rr + L
    u2 = 2.0 ** -52
    mt = u2 * L * (4.0 * Rr + 2.0 * T) * cut_factor + u2 * T + 1e-9
    mb = u2 * (3.0 * Rr + 2.0 * L) * L * cut_factor + 1e-9
    oxf, oyf = ox.astype(F), oy.astype(F)
    mag = np.abs(oxf) + np.abs(oyf) if origin_terms else np.zeros_like(oxf)
    mbf0 = mb.astype(F) * (F(1.0) + F(2.0 ** -20)) + F(3.0) * (mag + F(1.0)) * F(2.0 ** -24)
    mbf = mbf0 + (mag + mbf0) * F(2.0 ** -22)
    mtf = mt.astype(F) * (F(1.0) + F(2.0 ** -20)) + F(1e-6)
    nlo = (-(oxf + mbf), -(oyf + mbf))
    nhi = (mbf - oxf, mbf - oyf)
    csf, snf = r["cs"].astype(F), r["sn"].astype(F)
    zero = (csf == 0, snf == 0)
    with np.errstate(divide="ignore"):
        id2 = [np.where(z, F(0.0), F(1.0) / d) for z, d in zip(zero, (csf, snf))]
    for _ in range(abs(id_ulps)):
        id2 = [np.where(z, v, np.nextafter(v, INF32 if id_ulps > 0 else -INF32)) for z, v in zip(zero, id2)]
    quad = (np.signbit(csf).astype(np.int64)) | (np.signbit(snf).astype(np.int64) << 1)
    neg = ((quad & 1) != 0, (quad & 2) != 0)
    nn = [np.where(g, h, l) for g, h, l in zip(neg, nhi, nlo)]
    nf = [np.where(g, l, h) for g, h, l in zip(neg, nhi, nlo)]

    def times_id(n1, n2):
        c1, c2 = [a * i for a, i in zip(n1, id2)], [a * i for a, i in zip(n2, id2)]
        if open_axes:
            c1 = [np.where(z, -INF32, c) for z, c in zip(zero, c1)]
            c2 = [np.where(z, INF32, c) for z, c in zip(zero, c2)]
        return c1, c2

    clo, chi = times_id(nlo, nhi)
    cn, cf = times_id(nn, nf)
    return dict(clo=clo, chi=chi, cn=cn, cf=cf, id2=id2, mtf=mtf, quad=quad, mb=mb, mt=mt, T=T, zero=zero[0] | zero[1])


# ------------------------------------------------------------------------------ inputs
def rows(seed=5, per_centre=PER_CENTRE):
    """Rays x segments round every slot centre; dict of float64 columns.  A ray is built from its
    hit: a point P inside the slot circle, a direction, a distance t back to the origin, and a
    segment through P."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("ox", "oy", "cs", "sn", "sx", "sy", "v2x", "v2y", "cx", "cy", "rad", "L", "centre",
                           "dkind", "skind", "outside")}
    n = per_centre
    for ci, (cx, cy) in enumerate(CENTRES):
        r0 = np.exp(rng.uniform(np.log(4.0), np.log(8000.0), n))
        ln = np.minimum(np.exp(rng.uniform(np.log(0.05), np.log(300.0), n)), 0.45 * r0)
        rho = rng.uniform(0.0, 1.0, n) * (r0 - 1.01 * ln - 1e-6)
        pa = rng.uniform(-np.pi, np.pi, n)
        px, py = cx + rho * np.cos(pa), cy + rho * np.sin(pa)
        frac = rng.uniform(0.0, 1.0, n)
        frac = np.where(rng.random(n) < 0.25, rng.choice([0.0, 1.0], n) + rng.normal(0, 1e-9, n), frac)
        # directions: 0 random, 1 k pi / 2, 2 their 1-ulp neighbours, 3 a component of exactly +-0.0
        dk = rng.choice(4, n, p=[0.55, 0.15, 0.15, 0.15])
        base = rng.integers(-2, 7, n) * HALF_PI
        th = np.where(dk == 0, rng.uniform(-np.pi, np.pi, n), base)
        th = np.where(dk == 2, np.nextafter(base, np.where(rng.random(n) < 0.5, np.inf, -np.inf)), th)
        cs, sn = np.cos(th), np.sin(th)
        z = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        one = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        first = rng.random(n) < 0.5
        cs = np.where(dk == 3, np.where(first, z, one), cs)
        sn = np.where(dk == 3, np.where(first, one, z), sn)
        # segments: 0 any direction, 1 axis-parallel (a box of no width or height), 2 grazing: at an
        # angle of 1.2e-10 / L .. 1e-4 to the ray, |dotp| from just above the 1e-10 cut -- where the
        # computed t and s carry the errors eps_t, eps_s that mb and mt exist for
        sk = rng.choice(3, n, p=[0.55, 0.2, 0.25])
        ua = rng.uniform(-np.pi, np.pi, n)
        ux, uy = np.cos(ua), np.sin(ua)
        k4 = rng.integers(4, size=n)
        ux = np.where(sk == 1, np.array([1.0, 0.0, -1.0, 0.0])[k4], ux)
        uy = np.where(sk == 1, np.array([0.0, 1.0, 0.0, -1.0])[k4], uy)
        dl = np.exp(rng.uniform(np.log(1.2e-10 / ln), np.log(1e-4))) * rng.choice([-1.0, 1.0], n)
        ux = np.where(sk == 2, cs * np.cos(dl) - sn * np.sin(dl), ux)
        uy = np.where(sk == 2, sn * np.cos(dl) + cs * np.sin(dl), uy)
        # t: exactly 0, tiny, inside the circle, up to 100 radii away
        tk = rng.choice(4, n, p=[0.06, 0.14, 0.45, 0.35])
        t = np.select([tk == 0, tk == 1, tk == 2], [np.zeros(n), np.exp(rng.uniform(np.log(1e-9), np.log(1e-2), n)),
                                                   rng.uniform(0.0, 1.0, n) * r0],
                      np.exp(rng.uniform(np.log(1.0), np.log(100.0), n)) * r0)
        ox, oy = px - t * cs, py - t * sn
        sx, sy = px - frac * ln * ux, py - frac * ln * uy
        v2x, v2y = ln * ux, ln * uy
        for k, v in (("ox", ox), ("oy", oy), ("cs", cs), ("sn", sn), ("sx", sx), ("sy", sy), ("v2x", v2x), ("v2y", v2y),
                     ("cx", np.full(n, cx)), ("cy", np.full(n, cy)), ("rad", r0 * (1.0 + 1e-12) + 1e-9),
                     ("L", np.sqrt(v2x * v2x + v2y * v2y) * (1.0 + 1e-12) + 1e-12),  # rx_cull_geo's roundings up
                     ("centre", np.full(n, ci)), ("dkind", dk), ("skind", sk), ("outside", np.hypot(ox - cx, oy - cy) > r0)):
            out[k].append(v)
    r = {k: np.concatenate(v) for k, v in out.items()}
    # every end point lies inside the slot circle the kernel is told of
    ex, ey = r["sx"] + r["v2x"], r["sy"] + r["v2y"]
    assert np.all(np.maximum(np.hypot(r["sx"] - r["cx"], r["sy"] - r["cy"]), np.hypot(ex - r["cx"], ey - r["cy"])) <= r["rad"])
    return r


def boxes(r, seed=6):
    """(the segment's own box, a padded box, the padded box's plane kind) -- [n, 4] float64 as
    rx_cull_box_segment builds them.  Plane kind 1: a face of the padded box through the origin's
    coordinate, 2 / 3: 1e-9 max(1, |coord|) below / above it, 0: none."""
    rng = np.random.default_rng(seed)
    n = len(r["ox"])
    ex, ey = r["sx"] + r["v2x"], r["sy"] + r["v2y"]
    own = np.stack([np.minimum(r["sx"], ex), np.minimum(r["sy"], ey), np.maximum(r["sx"], ex), np.maximum(r["sy"], ey)], 1)
    ln = np.hypot(r["v2x"], r["v2y"])
    pad = rng.uniform(0.0, 8.0, (n, 4)) * ln[:, None] * (rng.random((n, 4)) < 0.8)
    big = own + pad * np.array([-1.0, -1.0, 1.0, 1.0])
    kind = rng.choice(4, n, p=[0.64, 0.12, 0.12, 0.12])
    done = kind == 0
    for a, o in ((0, r["ox"]), (1, r["oy"])):
        e = 1e-9 * np.maximum(1.0, np.abs(o))
        target = o + np.select([kind == 2, kind == 3], [-e, e], 0.0)
        lo = ~done & (target <= own[:, a])
        big[lo, a] = target[lo]
        done |= lo
        hi = ~done & (target >= own[:, a + 2])
        big[hi, a + 2] = target[hi]
        done |= hi
    kind = np.where(done, kind, 0)
    assert np.all(big[:, :2] <= own[:, :2]) and np.all(big[:, 2:] >= own[:, 2:])
    return own, big, kind


def exact(r):
    """(hit, t) of seg_test."""
    v3x, v3y = -r["sn"], r["cs"]
    hit = exact_hit(r["ox"], r["oy"], r["sx"], r["sy"], r["v2x"], r["v2y"], v3x, v3y)
    v1x, v1y = r["ox"] - r["sx"], r["oy"] - r["sy"]
    dotp = r["v2x"] * v3x + r["v2y"] * v3y
    cross = r["v2x"] * v1y - r["v2y"] * v1x
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(np.signbit(dotp), -cross, cross) / np.abs(dotp)
    return hit, np.where(hit, t, np.inf)


def bounds(t):
    """Four bounds best > t (rows where one is not, as t (1 + 1e-12) at t = 0, get inf)."""
    b = [np.full(len(t), np.inf), np.nextafter(t, np.inf), t * (1.0 + 1e-12), t + 1.0]
    return [np.where(v > t, v, np.inf) for v in b]


def lost(r, hit, t, own, big, forms=("f", "q"), **mutant):
    """The number of required keeps the box test loses, and of required keeps."""
    ops = operands(r, **mutant)
    n_lost = n_req = 0
    for b in (own, big):
        fb = box_f32(b)
        qb = quadrant_box(ops["quad"], fb)
        for best in bounds(t):
            bm = f32_up(best) + ops["mtf"]
            for form in forms:
                keep = chunk_needed_f(fb, ops, bm) if form == "f" else chunk_needed_q(qb, ops, bm)
                n_lost += int((hit & ~keep).sum())
                n_req += int(hit.sum())
    return n_lost, n_req


_CACHE = {}


def _inputs():
    if not _CACHE:
        r = rows()
        own, big, kind = boxes(r)
        hit, t = exact(r)
        _CACHE.update(r=r, own=own, big=big, kind=kind, hit=hit, t=t)
    return tuple(_CACHE[k] for k in ("r", "own", "big", "kind", "hit", "t"))


# ------------------------------------------------------------------------------ tests
def test_fma32_rounds_once():
    from fractions import Fraction

    def nearest_f32(q):  # a nonzero Fraction in float32's normal range, round half to even
        s, q = (-1.0 if q < 0 else 1.0), abs(q)
        e = q.numerator.bit_length() - q.denominator.bit_length() - 24
        while q / Fraction(2) ** e >= 2 ** 24:
            e += 1
        while q / Fraction(2) ** e < 2 ** 23:
            e -= 1
        m = q / Fraction(2) ** e
        n = m.numerator // m.denominator
        rem = m - n
        n += 1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2) else 0
        return F(s * float(n) * 2.0 ** e)

    one, e = F(1.0), F(2.0 ** -23)
    # (1 + e)(1 - e) + (-1) = -e^2 exactly: a separately rounded product would give 0
    assert fma32(one + e, one - e, -one) == -F(2.0 ** -46)
    # 2^30 + 128 + 64 (1 - 2^-46): a hair below the middle of two float32; the sum rounded to
    # float64 first IS the middle, and the tie would then go up to the even neighbour
    a, b, c = F(2.0 ** -20) * (one + e), F(2.0 ** 26) * (one - e), F(2.0 ** 30) + F(128.0)
    assert fma32(a, b, c) == c
    assert fma32(F(3.0), F(0.0), -INF32) == -INF32 and fma32(-F(5.0), F(0.0), INF32) == INF32
    rng = np.random.default_rng(1)
    a = (rng.normal(size=400) * 2.0 ** rng.integers(-8, 8, 400)).astype(F)
    b = (rng.normal(size=400) * 2.0 ** rng.integers(-8, 8, 400)).astype(F)
    c = np.where(rng.random(400) < 0.5, -(a.astype(D) * b.astype(D)) * (1 + rng.normal(size=400) * 1e-7),
                 rng.normal(size=400)).astype(F)  # half of them cancel to a few ulps
    got = fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        q = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        if q != 0 and abs(q) > Fraction(1, 2 ** 100):
            assert g == nearest_f32(q), (x, y, z)


def test_build_divides_correctly_rounded():
    """No flag of the build relaxes float32 division (hipcc's default for HIP device code is the
    correctly rounded quotient), nor contraction: the emulation's F(1) / d and separate roundings."""
    from rx import _build
    flags = " ".join(_build.FLAGS)
    for bad in ("fast-math", "-Ofast", "reciprocal-math", "unsafe-math", "no-hip-fp32-correctly-rounded", "approx-func",
                "relaxed-math", "denormals-to-zero", "-ffp-model"):
        assert bad not in flags, flags
    assert "-ffp-contract=off" in _build.FLAGS


def test_inputs_reach_every_rule():
    r, own, big, kind, hit, t = _inputs()
    ops = operands(r)
    for ci in range(len(CENTRES)):
        m = hit & (r["centre"] == ci)
        assert m.sum() >= 20_000, (ci, int(m.sum()))
        for dk in range(4):
            assert (m & (r["dkind"] == dk)).sum() >= 2_000, (ci, dk)
        for sk in range(3):
            assert (m & (r["skind"] == sk)).sum() >= 2_000, (ci, sk)
        assert (m & ops["zero"]).sum() >= 2_000, ci  # csf == 0 or snf == 0
        assert (m & r["outside"]).sum() >= 3_000 and (m & ~r["outside"]).sum() >= 3_000, ci
        assert (m & (t == 0)).sum() >= 200 and (m & (t > ops["T"] * 0.5)).sum() >= 100, ci
        for k in (1, 2, 3):
            assert (m & (kind == k)).sum() >= 1_000, (ci, k)
        # grazing: the hit point within mb of a face of the segment's own box
        with np.errstate(invalid="ignore"):
            px, py = r["ox"] + t * r["cs"], r["oy"] + t * r["sn"]
            gap = np.minimum(np.minimum(np.abs(px - own[:, 0]), np.abs(px - own[:, 2])),
                             np.minimum(np.abs(py - own[:, 1]), np.abs(py - own[:, 3])))
            assert (m & (gap <= ops["mb"])).sum() >= 3_000, ci
    L = np.hypot(r["v2x"], r["v2y"])[hit]
    assert L.min() < 0.06 and L.max() > 250.0


def test_box_test_keeps_every_box_of_an_exact_hit():
    r, own, big, kind, hit, t = _inputs()
    for id_ulps in (0, -2, 2):
        n_lost, n_req = lost(r, hit, t, own, big, id_ulps=id_ulps)
        assert n_req > 1_500_000
        assert n_lost == 0, (id_ulps, n_lost, n_req)


def test_mutants_lose_required_keeps():
    """Without open_axes, without the |ox| + |oy| terms of mbf, and with mb and mt short of their
    factor 1e10, required keeps are lost on these inputs (the counts: the module docstring) -- the
    inputs reach the rules."""
    r, own, big, kind, hit, t = _inputs()
    assert lost(r, hit, t, own, big, forms=("f",), open_axes=False)[0] > 0
    assert lost(r, hit, t, own, big, forms=("f",), origin_terms=False)[0] > 0
    assert lost(r, hit, t, own, big, forms=("f",), cut_factor=1.0)[0] > 0


def test_quadrant_form_decides_as_the_plain_form():
    r, own, big, kind, hit, t = _inputs()
    rng = np.random.default_rng(8)
    n = len(t)
    ops = operands(r)
    # the boxes of the hits, and boxes anywhere round the slot: kept and rejected ones
    far = np.stack([r["cx"], r["cy"], r["cx"], r["cy"]], 1) + rng.uniform(-1.0, 1.0, (n, 4)) * r["rad"][:, None]
    far = np.concatenate([np.minimum(far[:, :2], far[:, 2:]), np.maximum(far[:, :2], far[:, 2:])], 1)
    span = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), n))
    finite = np.where(np.isfinite(t), t, span)
    kept = rejected = 0
    for b in (own, big, far):
        fb = box_f32(b)
        qb = quadrant_box(ops["quad"], fb)
        for best in (np.full(n, np.inf), finite, finite * rng.uniform(0.0, 2.0, n), span):
            bm = f32_up(best) + ops["mtf"]
            kf, kq = chunk_needed_f(fb, ops, bm), chunk_needed_q(qb, ops, bm)
            assert np.array_equal(kf, kq), int((kf != kq).sum())
            kept += int(kf.sum())
            rejected += int((~kf).sum())
    assert kept > 500_000 and rejected > 500_000, (kept, rejected)


if __name__ == "__main__":
    r, own, big, kind, hit, t = _inputs()
    print("exact hits", int(hit.sum()), "of", len(hit), "rows; per centre",
          [int((hit & (r["centre"] == c)).sum()) for c in range(len(CENTRES))])
    for name, kw in (("shipped", {}), ("id2 - 2 ulp", dict(id_ulps=-2)), ("id2 + 2 ulp", dict(id_ulps=2)),
                     ("no open_axes", dict(open_axes=False)), ("no |ox| + |oy| in mbf", dict(origin_terms=False)),
                     ("mb, mt without the factor 1e10", dict(cut_factor=1.0))):
        n_lost, n_req = lost(r, hit, t, own, big, **kw)
        print(f"{name}: loses {n_lost:,} of {n_req:,} required keeps")
        for c in range(len(CENTRES)):
            m = r["centre"] == c
            rc = {k: v[m] for k, v in r.items()}
            print("   centre", CENTRES[c], lost(rc, hit[m], t[m], own[m], big[m], **kw)[0])
