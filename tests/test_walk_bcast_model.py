"""The arithmetic the EXPAND test of enum_walk.hip rests on since the first child's distance is a row broadcast
(DESIGN.md section 3), modelled in numpy.  CPU-only.

1. The candidate of lane j is tested with  a_j = a1 + z_j  instead of  (x_0 + z_j) - c,  a1 = x_0 - c taken after the
   tie correction of roundto().  a1 is exact (Sterbenz: |x_0 - c| <= 1/2), x_0 + z is an exact integer while
   |x_0| + 31 <= 2^53, so both expressions are ONE rounding of the same real number: the same double, and the same
   square.  Checked on bit patterns.  Above the boundary x_0 + z itself rounds and the two differ — outside the domain
   of the walk, whose step x_0 + z(i) departs from the reference's incremental x += dx there as well.

2. The lane layout: z = 0 in lane 0 of every 16-lane row (lanes 0, 16, 32, 48), +1, -1, ... +30, -30 over the other
   60 lanes.  With the ballot m of `dist_j <= bound`: m = 0 iff no child survives; popcount(m) - 3 is the length of the
   surviving prefix of the reference's zig-zag whenever popcount(m) < 64; popcount(m) = 64 iff all of +-30 survive
   (then the 61st child onwards is tested one by one)."""
import os
import re

import numpy as np

import conftest as C

SRC = os.path.join(C.ROOT, "fplll_amd", "csrc", "enum_walk.hip")
TWO53 = 2.0 ** 53


def _zig(i):
    """z(i) of the zig-zag with the first step up: 0, +1, -1, +2, -2, ... (zig_of(i, false) of the kernel)."""
    hh = (i + 1) >> 1
    return hh if i & 1 else -hh


def lane_z():
    """z of the 64 lanes: the kernel's  (lane & 15) == 0 ? 0.0 : zig_of(lane - (lane >> 4), false)."""
    return np.array([0.0 if (l & 15) == 0 else float(_zig(l - (l >> 4))) for l in range(64)])


def roundto(c):
    """(x_0, a1) of the walk: rint, ties away from zero, a1 = x_0 - c with the sign flipped where the tie moved x_0."""
    x = np.rint(c)
    a = x - c
    fix = (np.abs(a) == 0.5) & ((a < 0.0) == (c > 0.0))
    x = np.where(fix, x - (a + a), x)
    a = np.where(fix, -a, a)
    return x, a


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def test_the_layout_of_the_model_is_the_kernels():
    src = open(SRC).read()
    assert re.search(r"zz\s*=\s*\(lane & 15\) == 0 \? 0\.0 : \(double\)zig_of\(lane - \(lane >> 4\), false\);", src)
    z = lane_z()
    assert [l for l in range(64) if z[l] == 0.0] == [0, 16, 32, 48]
    rest = [z[l] for l in range(64) if l & 15]
    assert rest == [float(_zig(i)) for i in range(1, 61)]  # +1, -1, ... +30, -30 in lane order
    assert sorted(set(z)) == [float(v) for v in range(-30, 31)]


def _centres():
    rng = np.random.default_rng(20)
    cs = []
    for e in range(-3, 16):  # scales 10^-3 .. 10^15
        cs.append(rng.uniform(-1.0, 1.0, 20000) * 10.0 ** e)
    k = np.concatenate([np.arange(-300, 300), rng.integers(-2 ** 40, 2 ** 40, 4000), rng.integers(-2 ** 51, 2 ** 51, 4000)])
    half = k.astype(np.float64) + 0.5  # exact halves and their two neighbours
    cs += [half, np.nextafter(half, np.inf), np.nextafter(half, -np.inf)]
    ints = k.astype(np.float64)
    cs += [ints, np.nextafter(ints, np.inf), np.nextafter(ints, -np.inf)]
    tiny = np.array([5e-324, 2.5e-320, 2.2250738585072014e-308, 1e-300])  # denormals, the smallest normal
    cs.append(np.array([0.0, -0.0, 0.5, -0.5, 0.49999999999999994, -0.49999999999999994, 0.5000000000000001,
                        -0.5000000000000001, 1.5, -1.5, 2.5, -2.5]))
    cs += [tiny, -tiny]
    # below the boundary |x_0| + 31 = 2^53: the last centres of the domain (spacing 1 there: all integers)
    top = TWO53 - 31.0 - np.arange(0.0, 200.0)
    cs += [top, -top]
    return np.concatenate(cs)


def test_a1_plus_z_is_x_plus_z_minus_c_bit_for_bit():
    c = _centres()
    x, a = roundto(c)
    assert np.all(np.abs(x) + 31.0 <= TWO53)
    assert np.any(np.abs(x) + 31.0 == TWO53)  # (the boundary itself is inside)
    assert np.any((np.abs(a) == 0.5) & (np.abs(x) > np.abs(c)))  # (ties, moved away from zero)
    for z in sorted(set(lane_z())) + [31.0, -31.0]:  # (+-31: the domain statement covers the former layout as well)
        new = a + z
        old = (x + z) - c
        assert np.array_equal(_bits(new), _bits(old)), z
        assert np.array_equal(_bits(new * new), _bits(old * old)), z


def test_above_two_to_the_53_the_two_differ():
    """The other side of the boundary: x_0 + z rounds (ties to even), a1 + z does not — the domain ends where the
    docstring says it does, not earlier."""
    c = np.array([TWO53 - 30.0, TWO53, -(TWO53 - 30.0), -TWO53])  # |x_0| + 31 = 2^53 + 1 and above
    x, a = roundto(c)
    assert np.all(a == 0.0) and np.all(np.abs(x) + 31.0 > TWO53 - 1.0)
    differ = 0
    for z in sorted(set(lane_z())) + [31.0, -31.0]:
        differ += int(np.sum(_bits(a + z) != _bits((x + z) - c)))
    assert differ > 0
    # the first integer past the boundary, by hand: 2^53 + 1 is no double
    x1 = np.float64(TWO53)
    assert (x1 + 1.0) - x1 == 0.0 and np.float64(0.0) + 1.0 == 1.0


def _reference_prefix(c, nd, r, bound, ncand=140):
    """Length of the surviving prefix of the reference's zig-zag (enumerate_base.cpp:80-93): x_0, then alternately
    towards and away from the centre; the distance by the reference's sequence, x formed first."""
    x0, _ = roundto(c)
    sgn = np.where(c >= x0, 1.0, -1.0)
    zs = np.array([float(_zig(i)) for i in range(ncand)])
    x = x0[:, None] + sgn[:, None] * zs[None, :]
    al = x - c[:, None]
    dist = nd[:, None] + al * al * r[:, None]
    ok = dist <= bound[:, None]
    return np.cumprod(ok, axis=1).sum(axis=1), dist


def _ballot(c, nd, r, bound):
    _, a1 = roundto(c)
    aj = a1[:, None] + lane_z()[None, :]
    ndj = nd[:, None] + aj * aj * r[:, None]
    return ndj <= bound[:, None], ndj


def _cases():
    rng = np.random.default_rng(21)
    n = 60000
    c = rng.uniform(-40.0, 40.0, n)
    # a share of exact ties: integer, half-integer and quarter centres
    tie = rng.random(n) < 0.3
    c = np.where(tie, np.round(c * 4.0) / 4.0, c)
    big = rng.random(n) < 0.1
    c = np.where(big, c * 1e9, c)
    nd = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.9)
    # r such that the number of children ranges from 0 to well above 61
    span = rng.uniform(0.2, 45.0, n)  # about the half-width of the interval of children
    room = rng.uniform(0.1, 3.0, n)
    r = room / (span * span)
    bound = nd + room * rng.uniform(0.0, 1.2, n)
    dy = rng.random(n) < 0.3  # dyadic cases: every operation exact, so that ties +-z are ties of the doubles
    r = np.where(dy, 2.0 ** -rng.integers(4, 13, n), r)
    nd = np.where(dy, np.round(nd * 16.0) / 16.0, nd)
    c = np.where(dy & ~big, np.round(c * 4.0) / 4.0, c)
    return c, nd, r, bound


def _check(c, nd, r, bound):
    m, _ = _ballot(c, nd, r, bound)
    pop = m.sum(axis=1)
    pre, _ = _reference_prefix(c, nd, r, bound)
    z0 = m[:, [0, 16, 32, 48]]
    assert np.all(z0.all(axis=1) == z0.any(axis=1))
    assert np.all((pop == 0) == (pre == 0))
    assert np.all(z0.all(axis=1) == (pop > 0))  # any candidate passes: z = 0 passes in its four lanes
    hot = (pop > 0) & (pop < 64)
    assert np.all(pop[hot] - 3 == pre[hot])
    assert np.all((pop == 64) == (pre >= 61))
    return pop, pre


def test_popcount_of_the_new_layout_is_the_surviving_prefix():
    c, nd, r, bound = _cases()
    pop, pre = _check(c, nd, r, bound)
    # the cases cover: no child, one child (a chain link), both sides of the hot / slow boundary, the slow path
    for want in (0, 1, 2, 59, 60):
        assert np.any(pre == want), want
    assert np.any(pre == 61) and np.any(pre == 62) and np.any(pre > 70)
    assert np.any(pop == 63) and np.any(pop == 64)


def test_bounds_exactly_on_a_candidates_distance():
    """bound = the distance of the j-th child of the reference's zig-zag, as a double: that child survives (`<=`), and on
    dyadic inputs with an integer or half-integer centre so does its mirror image of EQUAL distance."""
    c, nd, r, _ = _cases()
    rng = np.random.default_rng(22)
    j = rng.integers(0, 70, len(c))
    j[:2000] = rng.integers(56, 66, 2000)  # crowd the hot / slow boundary
    _, dist = _reference_prefix(c, nd, r, np.full(len(c), np.inf))
    bound = dist[np.arange(len(c)), j]
    pop, pre = _check(c, nd, r, bound)
    assert np.all(pre >= j + 1)
    assert np.any(pre > j + 1)  # (ties: the mirror image came along)
    for want in (59, 60, 61, 62, 63):
        assert np.any(pre == want), want
