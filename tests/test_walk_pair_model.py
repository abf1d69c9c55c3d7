"""Model of the change of the fourth-generation walk (enum_walk4.hip), in numpy float64 — the
arithmetic of the kernel, which is compiled without contraction: separate multiplies and adds.

Ready pair siblings: a descent whose expansion has exactly two children forms the second child (x2, nd2, S2) from the
operands it holds in registers.  It must be bit for bit what the third generation's STEP forms later from the stored
level registers (x0, c, pd), the pushed column par and the row mk of mu: x = fma(z(1), sgd, x0), a = x - c,
nd = pd + a a r, S = par - (DUAL ? a : x) mk.  The fma is modelled exactly (rational arithmetic, one rounding).
Random and half-integer centres, both step directions, radii exactly on a candidate's distance; the expansion's 61
candidates are modelled as well, so that each case IS a pair node (popcount 5) of the kernel's vector test."""
from fractions import Fraction

import numpy as np


def _zz():
    """z_j of the 64 lanes: 0 in lane 0 of every 16-lane row, +1, -1, ... +30, -30 over the other 60."""
    out = []
    for lane in range(64):
        if lane % 16 == 0:
            out.append(0.0)
        else:
            i = lane - (lane >> 4)
            hh = (i + 1) >> 1
            out.append(float(hh if i & 1 else -hh))
    return np.array(out)


ZZ = _zz()


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds once, to nearest even)


def _expansion(c1, nd, r, bound):
    """The kernel's vector test around rint(c): (popcount, x1, a1) with the tie correction of the descent with siblings."""
    x1 = np.rint(c1)
    a1 = x1 - c1
    ndj = nd + (a1 + ZZ) * (a1 + ZZ) * r
    pop = int(np.count_nonzero(ndj <= bound))
    if abs(a1) == 0.5 and ((a1 < 0.0) == (c1 > 0.0)):
        x1 = x1 - (a1 + a1)
        a1 = -a1
    return pop, x1, a1, ndj


def _descent_pair(x1, c1, nd, r, S, mk1, dual):
    s = np.float64(1.0) if c1 >= x1 else np.float64(-1.0)
    x2 = x1 + s
    a2 = x2 - c1
    nd2 = nd + a2 * a2 * r
    S2 = S - (a2 if dual else x2) * mk1
    return x2, nd2, S2


def _step_today(x0, c, pd, r, par, mk, dual, i=1):
    hh = (i + 1) >> 1
    zd = float(hh if i & 1 else -hh)
    sgd = 1.0 if c >= x0 else -1.0
    xk = np.float64(_fma(zd, sgd, x0))
    a = xk - c
    nd = pd + a * a * r
    S = par - (a if dual else xk) * mk
    return xk, nd, S


def _cases(rng):
    """(c1, nd, r) of nodes: random centres, exact half-integers of both signs, centres next to a half, large ones."""
    out = []
    for _ in range(400):
        out.append((rng.uniform(-40, 40), rng.uniform(0, 3), rng.uniform(0.05, 2)))
    for h in range(-12, 13):
        for _ in range(4):
            out.append((h + 0.5, rng.uniform(0, 3), rng.uniform(0.05, 2)))
            out.append((h + 0.5, 0.25 * rng.integers(0, 8), 2.0 ** -int(rng.integers(0, 4))))  # (dyadic: exact sums)
    for h in (-3, 0, 7):
        for e in (np.nextafter(h + 0.5, 100.0), np.nextafter(h + 0.5, -100.0)):
            out.append((e, rng.uniform(0, 3), rng.uniform(0.05, 2)))
    for _ in range(50):
        out.append((rng.uniform(-1, 1) * 2.0 ** 40, rng.uniform(0, 3), rng.uniform(0.05, 2)))
    return [(np.float64(a), np.float64(b), np.float64(c)) for a, b, c in out]


def test_the_ready_sibling_is_the_step_s_sibling_bit_for_bit():
    rng = np.random.default_rng(20240611)
    pairs = ties = ups = downs = 0
    for c1, nd, r in _cases(rng):
        # the radius exactly on the second child's distance: two children, the third fails
        x_near = np.rint(c1)
        dists = sorted(nd + ((x_near + z) - c1) * ((x_near + z) - c1) * r for z in range(-3, 4))
        bound = dists[1]
        pop, x1, a1, ndj = _expansion(c1, nd, r, bound)
        if pop != 5:
            assert pop > 5 and dists[2] == dists[1]  # (the third child shares the second's distance: no pair node)
            continue
        pairs += 1
        ties += abs(a1) == 0.5
        k = int(rng.integers(2, 40))
        S = rng.uniform(-5, 5, 64)
        mk1 = rng.uniform(-0.5, 0.5, 64)
        for dual in (False, True):
            x2, nd2, S2 = _descent_pair(x1, c1, nd, r, S, mk1, dual)
            xs, nds, Ss = _step_today(x1, c1, nd, r, S.copy(), mk1, dual)
            assert x2.tobytes() == xs.tobytes()
            assert np.float64(nd2).tobytes() == np.float64(nds).tobytes()
            assert S2[:k].tobytes() == Ss[:k].tobytes()
            # the sibling is the second survivor of the vector test: within the bound, and its distance is the
            # distance the test computed in the lane of z = x2 - rint(c)
            assert nd2 <= bound
            lane = int(np.flatnonzero(ZZ == x2 - np.rint(c1))[0])
            assert np.float64(ndj[lane]).tobytes() == np.float64(nd2).tobytes()
        ups += x2 > x1
        downs += x2 < x1
    assert pairs > 400 and ties > 100 and ups > 100 and downs > 100, (pairs, ties, ups, downs)


def test_a_tie_steps_towards_the_other_nearest_integer():
    """On a tie x1 is roundto(c) (away from zero) and the step direction comes from the corrected x1: the sibling is
    the OTHER nearest integer, at the first child's distance."""
    for c1 in (2.5, -2.5, 0.5, -0.5, 17.5, -1001.5):
        c1 = np.float64(c1)
        pop, x1, a1, _ = _expansion(c1, np.float64(0.25), np.float64(1.0), np.float64(0.5))
        assert pop == 5 and abs(x1) > abs(c1) and abs(a1) == 0.5
        x2, nd2, _ = _descent_pair(x1, c1, np.float64(0.25), np.float64(1.0), np.zeros(64), np.zeros(64), False)
        assert abs(x2) < abs(c1) and abs(x2 - c1) == 0.5 and nd2 == 0.5
