"""The arithmetic the fifth-generation walk rests on (enum_walk5.hip), modelled in numpy.  CPU-only.

1. The fused add: fma(nd, 1.0, t) is one rounding of the real number nd + t, the double `nd + t` gives.  Checked with
   the C library's fma on bit patterns: random doubles of every scale, zeros of either sign, denormals, sums that
   round, sums that cancel.

2. The candidate layout of the generation: z = 0, +1, -1 in lanes 0, 1, 2 of EVERY 16-lane row, +-2 ... +-27 over the
   other 52 lanes — 55 distinct candidates.  With the ballot m of `dist_j <= bound`: m = 0 iff no child survives; the
   copies of a candidate agree; popcount(m & FPHIP_ZONCE) is the length of the surviving prefix of the reference's
   zig-zag whenever popcount(m) < 64; popcount(m) = 64 iff all of +-27 survive; popcount 4 is one child, 8 is two.

3. A node with exactly two surviving candidates and no tie: the survivor beside z = 0 is z = +1 (bit 1 of the ballot)
   iff c > x_0 — the direction STEP takes —, the distance in that lane has the bits of STEP's sequence (x = fma(z, sgd,
   x_0), a = x - c, nd = pd + a a r), and x_0 +- 1.0 is STEP's x.

4. A tie (|x_0 - c| = 0.5 exactly): z = 0 and the neighbour on the other side of c have equal distances: no child, or
   at least two — popcount 0 or >= 8, never a chain link and never the no-tie pair path."""
import ctypes
import ctypes.util
import os
import re

import numpy as np

import conftest as C
from test_walk_bcast_model import _bits, _reference_prefix, _zig, roundto

SRC = os.path.join(C.ROOT, "fplll_amd", "csrc", "enum_walk.hip")
ZONCE = 0xfff8fff8fff8ffff
COPIES = [[0, 16, 32, 48], [1, 17, 33, 49], [2, 18, 34, 50]]


def lane_z5():
    """z of the 64 lanes: the kernel's  zig_of((lane & 15) < 3 ? (lane & 15) : (lane & 15) + 13 * (lane >> 4), false)."""
    return np.array([float(_zig(l & 15 if (l & 15) < 3 else (l & 15) + 13 * (l >> 4))) for l in range(64)])


def test_the_layout_of_the_model_is_the_kernels():
    src = open(SRC).read()
    assert re.search(r"zz = \(double\)zig_of\(\(lane & 15\) < 3 \? \(lane & 15\) : \(lane & 15\) \+ 13 \* \(lane >> 4\), "
                     r"false\);", src)
    assert re.search(r"#define FPHIP_ZONCE 0x%xull" % ZONCE, src)
    z = lane_z5()
    for want, lanes in zip((0.0, 1.0, -1.0), COPIES):
        assert [l for l in range(64) if z[l] == want] == lanes
    rest = [z[l] for l in range(64) if (l & 15) >= 3]
    assert rest == [float(_zig(i)) for i in range(3, 55)]  # +2, -2, ... +27, -27 in lane order
    assert sorted(set(z)) == [float(v) for v in range(-27, 28)]
    once = [l for l in range(64) if (ZONCE >> l) & 1]
    assert sorted(z[once]) == [float(v) for v in range(-27, 28)]  # every candidate once


def _fma():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    return libm.fma


def test_fma_by_one_is_the_add_bit_for_bit():
    fma = _fma()
    assert fma(2.0 ** 53, 1.0, 1.0) == 2.0 ** 53 and fma(3.0, 5.0, 2.0 ** -60) == 15.0  # (it is a real fma: one rounding)
    rng = np.random.default_rng(50)
    nd = rng.uniform(0.0, 4.0, 6000) * 10.0 ** rng.integers(-12, 13, 6000)
    t = rng.uniform(0.0, 4.0, 6000) * 10.0 ** rng.integers(-12, 13, 6000)
    edge = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-320, 2.2250738585072014e-308, 1.0, -1.0, 2.0 ** 53, 2.0 ** -53,
                     1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 1.7976931348623157e308, 0.1, 0.7, 1e-17])
    a, b = np.meshgrid(edge, edge)
    nd = np.concatenate([nd, a.ravel(), np.nextafter(t[:1000], np.inf), t[:500]])
    t = np.concatenate([t, b.ravel(), t[:1000] * 2.0 ** -53, -np.nextafter(t[:500], 0.0)])  # halves of an ulp; cancellation
    assert len(nd) == len(t)
    with np.errstate(over="ignore"):
        want = nd + t
    got = np.array([fma(float(x), 1.0, float(y)) for x, y in zip(nd, t)])
    assert np.array_equal(_bits(got), _bits(want))
    assert np.any(want != nd) and np.any(want == nd) and np.any(np.isinf(want))


def _ballot5(c, nd, r, bound):
    """The kernel's test: around rint(c) — the tie correction comes after it."""
    x1 = np.rint(c)
    a1 = x1 - c
    aj = a1[:, None] + lane_z5()[None, :]
    ndj = nd[:, None] + aj * aj * r[:, None]
    return ndj <= bound[:, None], ndj, x1, a1


def _cases(seed=51, n=60000):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-40.0, 40.0, n)
    tie = rng.random(n) < 0.3  # exact ties: integer, half-integer and quarter centres
    c = np.where(tie, np.round(c * 4.0) / 4.0, c)
    big = rng.random(n) < 0.1
    c = np.where(big, c * 1e9, c)
    nd = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.9)
    span = rng.uniform(0.2, 45.0, n)
    room = rng.uniform(0.1, 3.0, n)
    r = room / (span * span)
    bound = nd + room * rng.uniform(0.0, 1.2, n)
    dy = rng.random(n) < 0.3  # dyadic cases: every operation exact
    r = np.where(dy, 2.0 ** -rng.integers(4, 13, n), r)
    nd = np.where(dy, np.round(nd * 16.0) / 16.0, nd)
    c = np.where(dy & ~big, np.round(c * 4.0) / 4.0, c)
    return c, nd, r, bound


def _check_prefix(c, nd, r, bound):
    m, _, _, _ = _ballot5(c, nd, r, bound)
    pop = m.sum(axis=1)
    pre, _ = _reference_prefix(c, nd, r, bound)
    for lanes in COPIES:
        g = m[:, lanes]
        assert np.all(g.all(axis=1) == g.any(axis=1))
    assert np.all((pop == 0) == (pre == 0))
    assert np.all(m[:, 0] == (pop > 0))
    once = np.array([(ZONCE >> l) & 1 for l in range(64)], dtype=bool)
    hot = (pop > 0) & (pop < 64)
    assert np.all(m[hot][:, once].sum(axis=1) == pre[hot])
    assert np.all((pop == 64) == (pre >= 55))
    assert np.all((pop == 4) == (pre == 1)) and np.all((pop == 8) == (pre == 2))
    assert not np.any((pop > 0) & (pop < 4)) and not np.any((pop > 4) & (pop < 8))
    return pop, pre


def test_popcount_of_the_layout_is_the_surviving_prefix():
    c, nd, r, bound = _cases()
    pop, pre = _check_prefix(c, nd, r, bound)
    for want in (0, 1, 2, 3, 53, 54, 55, 56):
        assert np.any(pre == want), want
    assert np.any(pre > 70) and np.any(pop == 63) and np.any(pop == 64)


def test_bounds_exactly_on_a_candidates_distance():
    c, nd, r, _ = _cases(52)
    rng = np.random.default_rng(53)
    j = rng.integers(0, 64, len(c))
    j[:4000] = rng.integers(0, 4, 4000)  # crowd the chain / pair / wide boundaries
    j[4000:6000] = rng.integers(51, 58, 2000)  # and the hot / slow one
    _, dist = _reference_prefix(c, nd, r, np.full(len(c), np.inf))
    bound = dist[np.arange(len(c)), j]
    pop, pre = _check_prefix(c, nd, r, bound)
    assert np.all(pre >= j + 1) and np.any(pre > j + 1)
    for want in (1, 2, 3, 54, 55, 56):
        assert np.any(pre == want), want


def _pair_centres():
    """Centres where a pair can go wrong: next to half-integers (the two neighbours nearly tie), next to integers (both
    neighbours nearly share the second place), large |x| up to 2^52 - 1 (half-integers end there), ordinary ones."""
    rng = np.random.default_rng(54)
    k = np.concatenate([np.arange(-40, 40), rng.integers(-2 ** 30, 2 ** 30, 3000), rng.integers(-2 ** 51, 2 ** 51, 3000),
                        np.array([2 ** 52 - 1, -(2 ** 52 - 1), 2 ** 52 - 2, -(2 ** 52 - 2)])]).astype(np.float64)
    half = k + np.where(np.abs(k + 0.5) < 2.0 ** 52, 0.5, 0.0)
    cs = [half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf), k, np.nextafter(k, np.inf),
          np.nextafter(k, -np.inf), rng.uniform(-50.0, 50.0, 20000), rng.uniform(-1.0, 1.0, 5000) * 1e12]
    c = np.concatenate(cs)
    c = np.concatenate([c, np.round(c[-25000:] * 8.0) / 8.0])  # dyadic fractions
    return c[np.abs(np.rint(c)) <= 2.0 ** 52 - 1]


def _step_child(x0, c, pd, r):
    """The second child as STEP forms it: z(1) = 1, sgd = +-1, x = fma(z, sgd, x_0) = x_0 + sgd (exact integers: the fma
    and the add are the same double), a = x - c, nd = pd + a a r."""
    sgd = np.where(c >= x0, 1.0, -1.0)
    x = 1.0 * sgd + x0
    a = x - c
    return x, pd + a * a * r, sgd


def test_the_no_tie_pair_is_read_off_the_test():
    c = _pair_centres()
    rng = np.random.default_rng(55)
    n = len(c)
    pd = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.9)
    r = rng.uniform(0.05, 3.0, n)
    dy = rng.random(n) < 0.3
    r = np.where(dy, 2.0 ** -rng.integers(0, 6, n).astype(np.float64), r)
    pd = np.where(dy, np.round(pd * 16.0) / 16.0, pd)
    inf = np.full(n, np.inf)
    _, ndj, x1, a1 = _ballot5(c, pd, r, inf)
    # bounds: exactly on the second child's distance (it survives by `<=`, the third may tie with it), one ulp above,
    # and halfway to the third
    d2 = np.minimum(ndj[:, 1], ndj[:, 2])
    d3 = np.maximum(ndj[:, 1], ndj[:, 2])
    seen_pair = 0
    for bound in (d2, np.nextafter(d2, np.inf), d2 + 0.5 * (d3 - d2)):
        m, ndj, x1, a1 = _ballot5(c, pd, r, bound)
        pop = m.sum(axis=1)
        pair = (pop == 8) & (np.abs(a1) != 0.5)
        seen_pair += int(pair.sum())
        up = m[pair, 1]
        assert np.all(up != m[pair, 2])  # exactly one of the two neighbours
        cp, xp, pdp, rp = c[pair], x1[pair], pd[pair], r[pair]
        assert np.all(up == (cp > xp))  # bit 1 iff c > x_0 ...
        assert not np.any(cp == xp)  # (an integer centre: both neighbours or neither)
        x0, _ = roundto(cp)
        assert np.array_equal(_bits(x0), _bits(xp))  # (no tie: rint is roundto)
        xs, nds, sgd = _step_child(x0, cp, pdp, rp)
        assert np.all((sgd > 0) == up)  # ... which is STEP's direction
        lane = np.where(up, 1, 2)
        assert np.array_equal(_bits(ndj[pair][np.arange(len(lane)), lane]), _bits(nds))
        assert np.array_equal(_bits(np.where(up, xp + 1.0, xp - 1.0)), _bits(xs))
        pre, _ = _reference_prefix(cp, pdp, rp, bound[pair])
        assert np.all(pre == 2)
    assert seen_pair > 20000
    big = np.abs(c) > 2.0 ** 40
    m, _, _, a1 = _ballot5(c[big], pd[big], r[big], d2[big])
    assert np.any((m.sum(axis=1) == 8) & (np.abs(a1) != 0.5))  # (pairs among the large centres as well)


def test_a_tie_has_no_child_or_at_least_two():
    rng = np.random.default_rng(56)
    k = np.concatenate([np.arange(-300, 300), rng.integers(-2 ** 40, 2 ** 40, 4000), rng.integers(-2 ** 51, 2 ** 51, 4000)])
    c = k.astype(np.float64) + 0.5
    n = len(c)
    pd = rng.uniform(0.0, 2.0, n)
    r = rng.uniform(0.01, 3.0, n)
    pops = set()
    for bound in (pd + rng.uniform(0.0, 3.0, n), pd + 0.25 * r, pd + 2.25 * r, pd):
        m, ndj, x1, a1 = _ballot5(c, pd, r, bound)
        assert np.all(np.abs(a1) == 0.5)
        other = np.where(a1 > 0.0, 2, 1)  # x_0 above c: the neighbour below shares its distance
        assert np.array_equal(_bits(ndj[:, 0]), _bits(ndj[np.arange(n), other]))
        pop = m.sum(axis=1)
        assert np.all((pop == 0) | (pop >= 8))
        pops |= set(int(v) for v in pop)
    assert {0, 8, 13} <= pops  # no child; the two that tie; those and the next two, which tie as well
