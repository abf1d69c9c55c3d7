"""An exact rational reference of the closest-vector enumeration (enumerate_block(..., target=t)) and its named inputs.

The model is exact_enum.py, whose blocks are used as they are: dyadic_block(d, seed, q, rexp) with a seeded target of
multiples of 1/q in [-4, 4].

Exactness, stated again for a target.  The coefficients x_j are integers, mu(j,i) and t_i multiples of 1/q, so every
centre  c_i = t_i - sum_j x_j mu(j,i)  is a multiple of 1/q and so is alpha = x_i - c_i; alpha^2 is a multiple of 1/q^2
and alpha^2 r_ii one of 2^-(2 log2 q + max e).  With the radii used here every partial distance is a multiple of that
unit below 2^10 and every centre a multiple of 1/q below 2^10: every product and every sum of the walk — in any order,
contracted or not — is exact in double.  Pruning vectors are multiples of 1/8 in [1/4, 1] and the radii small dyadic
numbers, so the bounds pruning_k * R are exact too.  The reference below is plain rational arithmetic
(fractions.Fraction) over the order-free definition of the visited set; the tests that use it compare with `==` only.
"""
from fractions import Fraction

import numpy as np

import exact_enum as E


def _frac(v):
    return Fraction(float(v))


def _round_away(c):
    """roundto() of the reference on a rational: the nearest integer, ties away from zero."""
    fl = c.numerator // c.denominator
    fr = c - fl
    if fr > Fraction(1, 2) or (fr == Fraction(1, 2) and c > 0):
        return fl + 1
    return fl


def exact_cvp_enumerate(mut, rdiag, pruning, R, target, max_nodes=10**6):
    """The set of nodes a closest-vector enumeration of radius^2 R around `target` visits, by its order-free
    definition, in rational arithmetic.

    A node (x_k .. x_{d-1}) is visited iff every partial distance  sum_{i >= j} (x_i - c_i)^2 r_ii,  j = d-1 .. k,  is
    <= pruning_j * R  (pruning None: 1), with  c_i = t_i - sum_{j > i} x_j mu(j,i).  There is no sign condition: with a
    target the reference walks the whole tree (enumerate_base.cpp:80, !is_svp), and a leaf of distance 0 is a candidate
    (:44, :99).

    nodes[k] is the plain number of visited nodes of level k, minus 1 (mod 2^64: the reference decrements an unsigned
    counter without a check, enumerate_base.cpp:180-183) for every level k0 < k < d, where k0 is the level at which the
    rounding descent of prepare_enumeration (enumerate.cpp:167-215) stopped: x_k = roundto(c_k) from k = d - 1 down
    while the distance accumulated so far is <= R (the radius, not the pruned bound); k0 = 0 when it never stops.

    Returns (nodes, candidates, stats):
      nodes       list of d + 1 ints (nodes[d] = 0, like the C ABI's array);
      candidates  [(dist, x)] with dist a float (0.0 included) and x a tuple of d floats, sorted;
      stats       dict: `int_centres` / `half_centres` — counted nodes whose centre is an integer / an odd multiple of
                  1/2; `at_bound` — candidates with dist == pruning_0 * R; `max_children` — the largest number of
                  children of one node; `k0`; `plain` — the per-level counts without the compensation; `min_group` —
                  the number of candidates at the smallest candidate distance."""
    d = len(rdiag)
    mu = [[_frac(mut[k][j]) for j in range(d)] for k in range(d)]  # mu[k][j] = mu(j,k), j > k
    r = [_frac(v) for v in rdiag]
    t = [_frac(v) for v in target]
    Rf = _frac(R)
    bound = [(_frac(pruning[k]) if pruning is not None else Fraction(1)) * Rf for k in range(d)]
    plain = [0] * d
    cands = []
    stats = dict(int_centres=0, half_centres=0, at_bound=0, max_children=0)
    total = [0]
    x = [0] * d

    def centre(k):
        return t[k] - sum((x[j] * mu[k][j] for j in range(k + 1, d) if x[j]), Fraction(0))

    def visit(k, pd):
        c = centre(k)
        ch = []
        lo = c.numerator // c.denominator  # floor(c)
        v = lo
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            ch.append(v)
            v -= 1
        v = lo + 1
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            ch.append(v)
            v += 1
        stats["max_children"] = max(stats["max_children"], len(ch))
        for v in ch:
            nd = pd + (v - c) * (v - c) * r[k]
            plain[k] += 1
            total[0] += 1
            assert total[0] <= max_nodes, "the tree is larger than the exact reference is meant for"
            if c.denominator == 1:
                stats["int_centres"] += 1
            elif c.denominator == 2:
                stats["half_centres"] += 1
            x[k] = v
            if k == 0:
                cands.append((nd, tuple(float(u) for u in x)))
            else:
                visit(k - 1, nd)
        x[k] = 0

    visit(d - 1, Fraction(0))
    # the rounding descent of prepare_enumeration, exactly
    newdist, k = Fraction(0), d - 1
    while k >= 0 and newdist <= Rf:
        c = centre(k)
        x[k] = _round_away(c)
        newdist += (x[k] - c) * (x[k] - c) * r[k]
        k -= 1
    k0 = k + 1
    nodes = list(plain) + [0]
    for i in range(k0 + 1, d):
        nodes[i] = (nodes[i] - 1) % 2**64
    for nd, _ in cands:
        assert Fraction(float(nd)) == nd, "a distance is not a double: the inputs are not dyadic enough"
    stats["at_bound"] = sum(1 for nd, _ in cands if nd == bound[0])
    stats["k0"] = k0
    stats["plain"] = plain
    best = min((nd for nd, _ in cands), default=None)
    stats["min_group"] = sum(1 for nd, _ in cands if nd == best)
    return nodes, sorted((float(nd), xs) for nd, xs in cands), stats


def dyadic_target(d, seed, q):
    """A seeded target of d multiples of 1/q in [-4, 4]."""
    rng = np.random.default_rng(seed + 5000)
    return rng.integers(-4 * q, 4 * q + 1, size=d).astype(np.float64) / float(q)


def _dyt(d, seed, q, rexp, R, pruned=False):
    def make():
        mut, rdiag = E.dyadic_block(d, seed, q=q, rexp=rexp)
        return mut, rdiag, (E.step_pruning(d) if pruned else None), R, dyadic_target(d, seed, q)
    return make


def _z8t():
    mut, rdiag = E.zd_block(8)
    return mut, rdiag, None, 4.0, np.full(8, 0.5)


# name -> () -> (mut, rdiag, pruning or None, radius^2, target).  The blocks of exact_enum.TIE_BLOCKS with a seeded
# target, at radii chosen on the exact reference alone for the window of tests/test_enum_cvp_cpu.py (2 000 .. 30 000
# exact nodes; sizes: the table there).  dy20t and pr28t: the rounding descent from the target leaves the radius
# (k0 = 2 and 4).  q2t (q = 2): EVERY centre is an integer or a half-integer.  z8t: Z^8 around (1/2, .., 1/2): every
# centre is 1/2, the 2^8 closest vectors tie at distance 2, and one coordinate off by 3/2 still fits under R = 4:
# (1 + m) 2^m nodes m coordinates deep, 4096 in all.
CVP_BLOCKS = {
    "dy12t": _dyt(12, 7, 4, (0, 1, 2), 1.25),
    "dy20t": _dyt(20, 7, 4, (0, 1, 2), 1.0),
    "pr28t": _dyt(28, 11, 4, (0, 1, 2), 1.25, pruned=True),
    "q2t": _dyt(16, 5, 2, (0, 1), 2.0),
    "z8t": _z8t,
}

_exact_cache = {}


def exact_of(name):
    """exact_cvp_enumerate of a named block, computed once per process and shared (treat as read-only)."""
    if name not in _exact_cache:
        mut, rdiag, pruning, R, target = CVP_BLOCKS[name]()
        _exact_cache[name] = exact_cvp_enumerate(mut, rdiag, pruning, R, target, max_nodes=30000)
    return _exact_cache[name]
