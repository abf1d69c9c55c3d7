"""The first child's distance of an expansion of the third-generation walk (enum_walk.hip, CHAIN = true) is computed by
every lane from wave-uniform operands,

    nd' = nd + a1 * a1 * r            (a1 = x1 - c after roundto()'s tie correction),

where it used to be lane 0's entry of the 64-lane test sent through the LDS crossbar,

    nd' = nd + aj * aj * r,  aj = (x1 + z_0) - c,  z_0 = +0.0.

The two are the same double in every case: the only thing `x1 + 0.0` can change is the sign of a zero coefficient
(-0.0 + 0.0 = +0.0), which can change the sign of a zero aj at most, and the square removes it.  Checked here bit for
bit (uint64 views) in numpy float64 with the kernel's operation sequence (separate multiplies and add, the
reference's order): random centres of several magnitudes, exact ties of both signs and both parities of the integer
below, centres that round to -0.0 and +-0.0 themselves, and a parent distance of 0."""
import numpy as np


def _roundto(c):
    """x1, a1 of the kernel: rint (ties to even), then ties away from zero with a1 = x1 - c kept in step."""
    x1 = np.rint(c)
    a1 = x1 - c
    fix = (np.abs(a1) == 0.5) & ((a1 < 0.0) == (c > 0.0))
    x1 = np.where(fix, x1 - (a1 + a1), x1)
    a1 = np.where(fix, -a1, a1)
    return x1, a1


def _both(c, nd, r):
    x1, a1 = _roundto(c)
    xj = x1 + np.float64(0.0)  # lane 0 of the test: z = 0
    aj = xj - c
    lane0 = nd + aj * aj * r
    uniform = nd + a1 * a1 * r
    return x1, lane0, uniform


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _operands(rng, n):
    nd = rng.uniform(0.0, 4.0e4, n) * rng.choice([1.0, 1e-6, 1e6], n)
    r = rng.uniform(0.5, 3.0e3, n) * rng.choice([1.0, 1e-3, 1e3], n)
    return nd, r


def test_random_centres():
    rng = np.random.default_rng(20261016)
    n = 4 * 10**6
    c = rng.standard_normal(n) * rng.choice([1e-3, 1.0, 50.0, 1e4, 1e9, 1e15], n)
    nd, r = _operands(rng, n)
    _, lane0, uniform = _both(c, nd, r)
    assert _same_bits(lane0, uniform)


def test_exact_ties_of_both_signs_and_parities():
    rng = np.random.default_rng(1)
    n = 10**6
    m = rng.integers(-2**40, 2**40, n).astype(np.float64)
    m[:8] = [0.0, -1.0, 1.0, -2.0, 2.0, 3.0, -3.0, 2.0**51]
    c = m + 0.5  # an exact tie above an even or an odd integer, on either side of zero
    assert np.all(c - m == 0.5)
    nd, r = _operands(rng, n)
    x1, lane0, uniform = _both(c, nd, r)
    assert np.array_equal(x1, np.where(c > 0.0, m + 1.0, m))  # away from zero
    assert {(bool(s), bool(p)) for s, p in zip(c[:4096] > 0, np.mod(m[:4096], 2.0) == 1.0)} == \
        {(False, False), (False, True), (True, False), (True, True)}
    assert _same_bits(lane0, uniform)


def test_signed_zeros_and_a_zero_parent_distance():
    rng = np.random.default_rng(2)
    n = 5 * 10**5
    c = -rng.uniform(0.0, 0.5, n)  # rounds to -0.0
    c[:4] = [-0.0, 0.0, -0.5, 0.5]
    nd, r = _operands(rng, n)
    nd[::2] = 0.0
    x1, lane0, uniform = _both(c, nd, r)
    assert np.all(np.signbit(x1[4:]) & (x1[4:] == 0.0))
    assert _same_bits(lane0, uniform)
    # the same centres with nd = 0 everywhere, and random centres with nd = 0
    z = np.zeros(n)
    _, lane0, uniform = _both(c, z, r)
    assert _same_bits(lane0, uniform)
    _, lane0, uniform = _both(rng.standard_normal(n) * 30.0, z, r)
    assert _same_bits(lane0, uniform)
