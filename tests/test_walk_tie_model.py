"""The arithmetic the EXPAND test of enum_walk.hip rests on since roundto()'s tie test left the chain link (DESIGN.md
section 3), modelled in numpy like tests/test_walk_bcast_model.py.  CPU-only.

The 64-lane test runs around x_0 = rint(c) (ties to even), not around roundto(c) (ties away from zero); the tie is
corrected later, on the descent with siblings only.  That is sound because on a tie — a1 = rint(c) - c = +-0.5 exactly —

1. the 61 candidates around either of the two nearest integers have the same multiset of |a1 + z_j|:
   {0.5, 0.5, 1.5, 1.5, ... 29.5, 29.5, 30.5}.  The distance depends on |a_j| only (a square), so the ballot around
   rint(c) has the popcount of the ballot around roundto(c), and the z = 0 distance — the first child's — is the same
   double;
2. z = 0 and its neighbour on the other side of c share |a_j| = 0.5, so a tie has no child or at least two: the
   popcount is 0 or >= 5 (z = 0 sits in four lanes), never 4 — a chain link never sees a tie;
3. for a centre that is no tie rint(c) IS roundto(c): nothing changes.

The magnitudes go up to 2^52, where the half-integers end."""
import numpy as np

from test_walk_bcast_model import _bits, _check, lane_z, roundto

TWO52 = 2.0 ** 52


def rint_a(c):
    """(x_0, a1) of the vector test: the raw v_rndne result, no tie correction."""
    x = np.rint(c)
    return x, x - c


def _ballot_with(c, nd, r, bound, x_a):
    _, a1 = x_a(c)
    aj = a1[:, None] + lane_z()[None, :]
    ndj = nd[:, None] + aj * aj * r[:, None]
    return ndj <= bound[:, None], ndj


def _half_centres(n, rng):
    """Half-integer centres of both signs: small ones, every binade up to 2^52 (the last half-integers are
    2^52 - 0.5 and its negative), even and odd integer parts — rint goes towards zero for one, away for the other."""
    k = np.concatenate([np.arange(-40, 40), rng.integers(-2 ** 20, 2 ** 20, n), rng.integers(-2 ** 40, 2 ** 40, n),
                        rng.integers(-2 ** 51, 2 ** 51, n), 2 ** 52 - 1 - np.arange(0, 40), -(2 ** 52) + np.arange(0, 40)])
    for e in range(1, 52):
        k = np.concatenate([k, 2 ** e + rng.integers(0, 2 ** e, 8), -(2 ** e) - rng.integers(0, 2 ** e, 8) - 1])
    c = k.astype(np.float64) + 0.5
    assert np.all(c - np.floor(c) == 0.5) and np.max(np.abs(c)) == TWO52 - 0.5
    return c


def _operands(c, rng):
    """Random r, nd and bounds around the half-width of the interval of children (0 to well above 61 children); a share
    of dyadic r and nd, where every operation is exact."""
    n = len(c)
    nd = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.9)
    span = rng.uniform(0.2, 45.0, n)
    room = rng.uniform(0.1, 3.0, n)
    r = room / (span * span)
    bound = nd + room * rng.uniform(0.0, 1.2, n)
    dy = rng.random(n) < 0.3
    r = np.where(dy, 2.0 ** -rng.integers(4, 13, n), r)
    nd = np.where(dy, np.round(nd * 16.0) / 16.0, nd)
    return nd, r, bound


def _assert_same_test(c, nd, r, bound):
    """The ballot around rint(c) against the one around roundto(c): popcount, z = 0 lanes, z = 0 distance."""
    m_raw, d_raw = _ballot_with(c, nd, r, bound, rint_a)
    m_fix, d_fix = _ballot_with(c, nd, r, bound, roundto)
    pop_raw, pop_fix = m_raw.sum(axis=1), m_fix.sum(axis=1)
    assert np.array_equal(pop_raw, pop_fix)
    z0 = [0, 16, 32, 48]
    assert np.array_equal(m_raw[:, z0], m_fix[:, z0])
    assert np.array_equal(_bits(d_raw[:, z0]), _bits(d_fix[:, z0]))
    # the multiset of distances is the same: the sorted rows agree bit for bit
    assert np.array_equal(_bits(np.sort(d_raw, axis=1)), _bits(np.sort(d_fix, axis=1)))
    return pop_raw


def test_a_tie_tested_around_rint_is_the_tie_tested_around_roundto():
    rng = np.random.default_rng(61)
    c = np.tile(_half_centres(3000, rng), 4)
    x_raw, a_raw = rint_a(c)
    x_fix, a_fix = roundto(c)
    assert np.all(np.abs(a_raw) == 0.5) and np.all(np.abs(a_fix) == 0.5)
    moved = x_raw != x_fix
    assert np.any(moved & (c > 0)) and np.any(moved & (c < 0)) and np.any(~moved & (c > 0)) and np.any(~moved & (c < 0))
    assert np.all(np.abs(x_fix) > np.abs(c))  # (roundto: away from zero, always)
    assert np.array_equal(a_fix[moved], -a_raw[moved]) and np.array_equal(a_fix[~moved], a_raw[~moved])
    # the multiset of |a1 + z| is {0.5 x 5, 1.5 x 2, ... 29.5 x 2, 30.5} over the 64 lanes, whichever integer is x_0
    want = np.sort(np.concatenate([[0.5] * 5, np.repeat(np.arange(1.5, 30.0), 2), [30.5]]))
    for a in (a_raw, a_fix):
        assert np.array_equal(np.sort(np.abs(a[:, None] + lane_z()[None, :]), axis=1), np.tile(want, (len(c), 1)))
    nd, r, bound = _operands(c, rng)
    pop = _assert_same_test(c, nd, r, bound)
    assert np.all((pop == 0) | (pop >= 5))
    for want_pop in (0, 5, 7, 63, 64):
        assert np.any(pop == want_pop), want_pop
    # ... and the popcount is the surviving prefix of the reference's zig-zag (the checks of test_walk_bcast_model.py)
    _check(c, nd, r, bound)


def test_bounds_exactly_on_a_candidates_distance_of_a_tie():
    """bound = the distance of one of the candidates, as a double (`<=` holds with equality there): the candidate and
    its mirror image of equal |a_j| survive together, around either integer."""
    rng = np.random.default_rng(62)
    c = np.tile(_half_centres(2000, rng), 3)
    nd, r, _ = _operands(c, rng)
    _, dist = _ballot_with(c, nd, r, np.full(len(c), np.inf), roundto)
    lane = rng.integers(0, 64, len(c))
    lane[:3000] = rng.choice([0, 1, 2, 3, 4, 62, 63], 3000)  # crowd both ends: the chain boundary and the slow one
    bound = dist[np.arange(len(c)), lane]
    pop = _assert_same_test(c, nd, r, bound)
    assert np.all(pop >= 5)  # (the bound is some candidate's distance: z = 0 passes, and with it its mirror image)
    assert np.any(pop == 5) and np.any(pop == 63) and np.any(pop == 64)
    # where nothing rounds (dyadic r, nd; |c| small enough for a_j^2 r to be exact) the mirror image came along exactly
    below = np.nextafter(bound, -np.inf)
    pop_below = _assert_same_test(c, nd, r, below)
    assert np.all((pop_below == 0) | (pop_below >= 5))
    assert np.any(pop_below == 0)


def test_nothing_changes_for_a_centre_that_is_no_tie():
    rng = np.random.default_rng(63)
    half = _half_centres(500, rng)
    c = np.concatenate([rng.uniform(-40.0, 40.0, 40000), rng.uniform(-1.0, 1.0, 20000) * 1e9,
                        np.nextafter(half, np.inf), np.nextafter(half, -np.inf),
                        np.arange(-50.0, 50.0), rng.integers(-2 ** 51, 2 ** 51, 2000).astype(np.float64),
                        np.array([0.0, -0.0, 0.49999999999999994, -0.49999999999999994, 0.5000000000000001,
                                  -0.5000000000000001, 5e-324, -5e-324])])
    x_raw, a_raw = rint_a(c)
    x_fix, a_fix = roundto(c)
    assert not np.any(np.abs(a_raw) == 0.5)
    assert np.array_equal(_bits(x_raw), _bits(x_fix)) and np.array_equal(_bits(a_raw), _bits(a_fix))
    nd, r, bound = _operands(c, rng)
    m_raw, d_raw = _ballot_with(c, nd, r, bound, rint_a)
    m_fix, d_fix = _ballot_with(c, nd, r, bound, roundto)
    assert np.array_equal(m_raw, m_fix) and np.array_equal(_bits(d_raw), _bits(d_fix))
    pop = m_raw.sum(axis=1)
    assert np.any(pop == 4)  # (the chain link exists here — and only here)
