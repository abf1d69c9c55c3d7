"""Exact-tie inputs for the enumeration and an exact rational reference of what it has to visit.

The seeded blocks of conftest.py are in general position: no centre is an integer or a half-integer, no two siblings
have the same distance, no distance equals its bound.  The blocks made here are the opposite — every one of those
coincidences happens hundreds of times — and they are built from dyadic rationals, so that every operation of the
enumeration is EXACT in double whatever its order.  That gives a reference which shares nothing with the kernels or
with oracle/enum_oracle.c: plain rational arithmetic (fractions.Fraction) over the order-free definition of the
visited set (exact_enumerate).  The tests that use it compare with `==` only.
"""
from fractions import Fraction

import numpy as np


def dyadic_block(d, seed, q=4, rexp=(0,), zero_frac=0.3):
    """A seeded block of d rows made of dyadic rationals: returns (mut, rdiag), mut[i][j] = mu(j,i) for j > i (the
    layout a plugin receives), zero elsewhere.

      * mu(j,i) is a seeded integer in [-q/2, q/2] divided by q (q a power of two): exactly +-1/2, +-1/4 (q = 4) and 0
        all occur; a seeded share `zero_frac` of the entries is set to 0 on top of that (untouched q-vectors);
      * r_kk = 2^-e_k, e_k drawn from `rexp` and sorted non-decreasing in k (r_kk does not grow with k).

    Exactness.  The coefficients x_j are integers, so every centre  c_k = -sum_j x_j mu(j,k)  is a multiple of 1/q, and
    so is alpha = x_k - c_k; alpha^2 is a multiple of 1/q^2 and alpha^2 r_kk one of 2^-(2 log2 q + max e).  With the
    radii used here every partial distance is a multiple of that unit below 2^10, i.e. an integer below
    2^(10 + 2 log2 q + max e) <= 2^26 times a power of two: every product and every sum of the walk — in any order,
    contracted or not — is exact in double, and so are the centres (multiples of 1/q below 2^10).  Pruning vectors used
    with these blocks are multiples of 1/8 in [1/4, 1] and the radii small dyadic numbers, so the bounds
    pruning_k * R are exact too.  (The dual recursion drives its centres by alpha instead of x: its centres are
    multiples of 1/q^depth and the argument does not hold there; the dual tests compare with the oracle only.)"""
    assert q >= 2 and q & (q - 1) == 0
    rng = np.random.default_rng(seed)
    num = rng.integers(-(q // 2), q // 2 + 1, size=(d, d))
    num[rng.random((d, d)) < zero_frac] = 0
    mu = np.tril(num.astype(np.float64) / float(q), -1)
    e = np.sort(rng.choice(np.asarray(rexp, dtype=np.int64), size=d))
    rdiag = np.ldexp(1.0, -e).astype(np.float64)
    return np.ascontiguousarray(mu.T), rdiag


def step_pruning(d, low=0.25):
    """A pruning vector of multiples of 1/8, non-increasing in k, from 1 (level 0) down to `low` (level d - 1)."""
    lo8 = int(round(low * 8))
    assert 2 <= lo8 <= 8
    p = np.array([(8 - ((8 - lo8) * k) // max(1, d - 1)) / 8.0 for k in range(d)])
    assert p[0] == 1.0 and np.all(np.diff(p) <= 0.0) and p.min() >= 0.25
    return p


def _frac(v):
    return Fraction(float(v))  # exact: a double IS a dyadic rational


def exact_enumerate(mut, rdiag, pruning, R, max_nodes=10**6):
    """The set of nodes an SVP enumeration of radius^2 R visits, by its order-free definition, in rational arithmetic.

    A node (x_k .. x_{d-1}) is visited iff
      * every partial distance  sum_{i >= j} (x_i - c_i)^2 r_ii,  j = d-1 .. k,  is <= pruning_j * R  (pruning None: 1), and
      * the first non-zero coefficient from the top is positive, or all coefficients are zero (the reference walks half
        of the tree: below an all-zero prefix it only counts upwards, enumerate_base.cpp:86-89).
    The children of a node are found by stepping away from floor(c) in both directions while the (convex) distance
    stays within the bound: no zig-zag, no rounding, no floating point.

    nodes[k] counts the visited nodes of level k the way the reference does: the all-zero prefix is NOT counted at the
    levels >= 1 (enumerate_base.cpp:181-184 takes back what the entry of those levels adds; the C oracle, which is pinned
    against the reference, differs from the plain count by exactly 1 at every level >= 1), the zero leaf is counted at
    level 0.  Candidates are the level-0 nodes of distance > 0 (:42-46).

    Returns (nodes, candidates, stats):
      nodes       list of d + 1 ints (nodes[d] = 0, like the C ABI's array);
      candidates  [(dist, x)] with dist a float and x a tuple of d floats, sorted;
      stats       dict: `int_centres` / `half_centres` — counted nodes below a NON-zero prefix whose centre is an
                  integer / an odd multiple of 1/2 (below the zero prefix every centre is 0 and the reference takes
                  another path); `at_bound` — candidates with dist == pruning_0 * R; `max_group` — the largest number of
                  candidates of one distance; `distinct` — the number of distinct candidate distances; `max_children`
                  — the largest number of children of one node; `level_min` — per level the smallest non-zero partial
                  distance of a visited node (float, None if there is none): the exact sub-solution distances."""
    d = len(rdiag)
    mu = [[_frac(mut[k][j]) for j in range(d)] for k in range(d)]  # mu[k][j] = mu(j,k), j > k
    r = [_frac(v) for v in rdiag]
    Rf = _frac(R)
    bound = [(_frac(pruning[k]) if pruning is not None else Fraction(1)) * Rf for k in range(d)]
    nodes = [0] * (d + 1)
    cands = []
    stats = dict(int_centres=0, half_centres=0, at_bound=0, max_group=0, distinct=0, max_children=0,
                 level_min=[None] * d)
    total = [0]
    x = [0] * d

    def children(k, c, pd, zero_prefix):
        out = []
        lo = c.numerator // c.denominator  # floor(c)
        v = lo
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            out.append(v)
            v -= 1
        v = lo + 1
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            out.append(v)
            v += 1
        if zero_prefix:
            out = [v for v in out if v >= 0]
        return out

    def visit(k, pd, zero_prefix):
        c = -sum((x[j] * mu[k][j] for j in range(k + 1, d) if x[j]), Fraction(0))
        ch = children(k, c, pd, zero_prefix)
        stats["max_children"] = max(stats["max_children"], len(ch))
        for v in ch:
            nd = pd + (v - c) * (v - c) * r[k]
            still_zero = zero_prefix and v == 0
            if k == 0 or not still_zero:
                nodes[k] += 1
                total[0] += 1
                assert total[0] <= max_nodes, "the tree is larger than the exact reference is meant for"
            if not zero_prefix:
                if c.denominator == 1:
                    stats["int_centres"] += 1
                elif c.denominator == 2:
                    stats["half_centres"] += 1
            if nd > 0 and (stats["level_min"][k] is None or nd < stats["level_min"][k]):
                stats["level_min"][k] = nd
            x[k] = v
            if k == 0:
                if nd > 0:
                    cands.append((nd, tuple(float(t) for t in x)))
            else:
                visit(k - 1, nd, still_zero)
        x[k] = 0

    visit(d - 1, Fraction(0), True)
    groups = {}
    for nd, _ in cands:
        groups[nd] = groups.get(nd, 0) + 1
    stats["at_bound"] = groups.get(bound[0], 0)
    stats["max_group"] = max(groups.values()) if groups else 0
    stats["distinct"] = len(groups)
    for nd in list(groups) + [m for m in stats["level_min"] if m is not None]:
        assert Fraction(float(nd)) == nd, "a distance is not a double: the inputs are not dyadic enough"
    stats["level_min"] = [None if m is None else float(m) for m in stats["level_min"]]
    return nodes, sorted((float(nd), xs) for nd, xs in cands), stats


def ball_count(d, R):
    """The number of x in Z^d with |x|^2 <= R: the d-th power of the one-dimensional theta series, in integers."""
    n = int(R)
    assert n >= 0
    one = [0] * (n + 1)
    v = 0
    while v * v <= n:
        one[v * v] += 1 if v == 0 else 2
        v += 1
    coef = [1] + [0] * n
    for _ in range(d):
        nxt = [0] * (n + 1)
        for a, ca in enumerate(coef):
            if ca:
                for b, cb in enumerate(one):
                    if cb and a + b <= n:
                        nxt[a + b] += ca * cb
        coef = nxt
    return sum(coef)


def zd_block(d):
    """Z^d: mu = 0, r_kk = 1."""
    return np.zeros((d, d)), np.ones(d)


def zd_nodes(d, R):
    """The reference's per-level counts on Z^d: level k holds half of the non-zero points of the (d-k)-dimensional
    ball, plus the zero leaf at level 0."""
    return [(ball_count(d - k, R) - 1) // 2 + (1 if k == 0 else 0) for k in range(d)] + [0]


# ---- the named tie blocks of tests/test_enum_exact_ties_{cpu,gpu}.py ----------------------------------------------
def _dy(d, seed, q, rexp, R, pruned=False):
    def make():
        mut, rdiag = dyadic_block(d, seed, q=q, rexp=rexp)
        return mut, rdiag, (step_pruning(d) if pruned else None), R
    return make


def _zd(d, R):
    def make():
        mut, rdiag = zd_block(d)
        return mut, rdiag, None, R
    return make


# name -> () -> (mut, rdiag, pruning or None, radius^2); sizes and tie counts of each: the table in
# tests/test_enum_exact_ties_cpu.py.  q2 (q = 2): EVERY centre is an integer or a half-integer.  dy20big is dy20's
# block at R = 2: 181179 nodes, above what the exact reference is meant for (40-100 us per node) — the C oracle,
# which equals the exact reference on every block of TIE_BLOCKS, is the reference there.
TIE_BLOCKS = {
    "z8": _zd(8, 4.0),
    "z12": _zd(12, 2.0),
    "eq10": _dy(10, 3, 4, (0,), 3.0),
    "dy12": _dy(12, 7, 4, (0, 1, 2), 1.0),
    "dy20": _dy(20, 7, 4, (0, 1, 2), 1.5),
    "pr28": _dy(28, 11, 4, (0, 1, 2), 1.5, pruned=True),
    "q2": _dy(16, 5, 2, (0, 1), 2.0),
}
ORACLE_ONLY_BLOCKS = {"dy20big": _dy(20, 7, 4, (0, 1, 2), 2.0)}
DYADIC = ("eq10", "dy12", "dy20", "pr28", "q2")  # the blocks every kind of tie is demanded of

_exact_cache = {}


def exact_of(name):
    """exact_enumerate of a named block, computed once per process and shared (treat as read-only)."""
    if name not in _exact_cache:
        mut, rdiag, pruning, R = TIE_BLOCKS[name]()
        _exact_cache[name] = exact_enumerate(mut, rdiag, pruning, R, max_nodes=30000)
    return _exact_cache[name]


def fat_level_block(d, fat, seed):
    """More than 63 children with exact ties: a dyadic block (q = 4, r = 1) whose level `fat` has r = 2^-12 and
    mu(j, fat) = 0 for every j > fat — every node of that level has centre 0, its children +-z have EQUAL distances
    z^2 2^-12 on both sides of the boundary between the first 63 candidates (one ballot) and the rest (one by one).
    Below the level the coefficients up to +-64 enter the centres through mu(fat, i) in multiples of 1/4.  Distances
    are multiples of 2^-16 below 2^10: exact."""
    mut, rdiag = dyadic_block(d, seed, q=4, rexp=(0,))
    mut = mut.copy()
    rdiag = rdiag.copy()
    mut[fat, fat + 1:] = 0.0
    rdiag[fat] = 2.0 ** -12
    return mut, rdiag


def wide_dyadic_block(d=72, d0=40, seed=9, R=1.0, cheap=(45, 66)):
    """conftest.wide_block_with_candidates made dyadic: dyadic_block(d0, seed, q=4, rexp=(0,1,2)) below, rows >= d0 of
    r_kk = R / 2 except the `cheap` ones (R / 8), mu zero between the rows >= d0 (their centres stay 0: integer
    centres, children +-1 of equal distance) and seeded multiples of 1/4 from every row >= d0 into the columns < d0."""
    mut0, r0 = dyadic_block(d0, seed, q=4, rexp=(0, 1, 2))
    rng = np.random.default_rng(seed + 2000)
    num = rng.integers(-2, 3, size=(d - d0, d0))
    num[rng.random((d - d0, d0)) < 0.3] = 0
    mu = np.zeros((d, d))
    mu[:d0, :d0] = mut0.T
    mu[d0:, :d0] = num / 4.0
    rdiag = np.concatenate([r0, np.full(d - d0, R / 2.0)])
    for k in cheap:
        rdiag[k] = R / 8.0
    return np.ascontiguousarray(mu.T), rdiag, R


def reports_at_current_bound(log, evaluator, maxdist):
    """Feeds `log` [(dist, x)] to `evaluator` from radius^2 `maxdist` and counts the candidates whose distance EQUALS
    the bound current when they are reported: the `<=` of the bound test after an evaluator returned max_dist = dist."""
    n, m = 0, float(maxdist)
    for dist, x in log:
        n += dist == m
        m = float(evaluator.eval_sol(x, dist, m))
    return n


def best_n_guarantee(mut, rdiag, pruning, cands, n):
    """What a BEST_N run (n solutions kept) must end with on ANY walk order, from the exact candidate list `cands`:
    returns (m_n, final_fixed, head_fixed), m_n the n-th smallest candidate distance.  The bound of such a run never
    drops below m_n, so a candidate all of whose partial distances pass pruning_k * m_n ("safe"; every candidate of an
    unpruned block) is reported whatever happened before.  final_fixed: at least n candidates of distance <= m_n are
    safe — the final bound IS m_n.  head_fixed: also every candidate shorter than m_n is safe — the kept distances are
    the n smallest of the multiset."""
    d = len(rdiag)
    dists = sorted(a for a, _ in cands)
    m = dists[n - 1]

    def safe(x):
        if pruning is None:
            return True
        pd = 0.0
        for k in range(d - 1, -1, -1):
            c = 0.0
            for j in range(d - 1, k, -1):
                c = c - x[j] * mut[k, j]
            a = x[k] - c
            pd = pd + a * a * rdiag[k]  # (exact on the dyadic blocks)
            if not pd <= pruning[k] * m:
                return False
        return True

    near = [(a, safe(x)) for a, x in cands if a <= m]
    final_fixed = sum(1 for _, s in near if s) >= n
    head_fixed = final_fixed and all(s for a, s in near if a < m)
    return m, final_fixed, head_fixed
