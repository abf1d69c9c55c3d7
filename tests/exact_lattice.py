"""An exact reference for the three solvers (shortest_vector, closest_vector(s), short_vectors / vectors_near /
theta_series): Fincke-Pohst enumeration of an integer basis in rational arithmetic.  No GPU, no float: the
Gram-Schmidt data are list_helpers.gso_exact's Fractions, every comparison is between rationals, every norm that is
returned is a Python integer.  It shares nothing with the kernels or with tests/svp_model.py: no radius margin, no
rounding of centres, no zig-zag, no row exponents.

  short_exact(B, N, rows=None, level=None)  -> ([(norm, x)], nodes)   0 < |xB|^2 <= N, one of each pair +-x
  near_exact(B, t, N)                       -> ([(norm, x)], nodes)   |xB - t|^2 <= N, the whole tree
  lambda1_exact(B, rows=None)               -> (norm, [x], nodes)     the minimum and every minimal vector (one of +-x)
  closest_exact(B, t)                       -> (dist, [x], nodes)     the minimal |xB - t|^2 and every closest point
  d_eff_exact(B)                            -> last_useful_index (svpcvp.cpp:32-43) on the exact r_ii

B is [d][n] Python integers (rows = basis vectors, linearly independent), x a tuple of d integers, lists sorted by
(norm, x).  `nodes` counts every visited tree node (every accepted coefficient at every level, the zero leaf included).
"""
from fractions import Fraction

import list_helpers as H


def _ints(B, rows=None):
    B = [[int(v) for v in row] for row in B]
    return B if rows is None else B[:rows]


_gso_cache = {}


def _gso(B):
    """list_helpers.gso_exact of B, kept per basis (the families' members are asked for many times)."""
    key = tuple(tuple(row) for row in B)
    if key not in _gso_cache:
        _gso_cache[key] = H.gso_exact(B)
    return _gso_cache[key]


def _floor(c):
    return c.numerator // c.denominator


def _target_coord(B, mu, r, t):
    """The Gram-Schmidt coordinates of the integer vector t (tc_i = <t, b*_i> / r_i) and |t - its projection on the
    span|^2, both exact."""
    d = len(B)
    s = [Fraction(0)] * d  # <t, b*_i>
    for i in range(d):
        s[i] = Fraction(sum(a * b for a, b in zip(t, B[i]))) - sum((mu[i][j] * s[j] for j in range(i)), Fraction(0))
    tc = [s[i] / r[i] for i in range(d)]
    perp = Fraction(sum(a * a for a in t)) - sum((tc[i] * s[i] for i in range(d)), Fraction(0))
    assert perp >= 0
    return tc, perp


def _walk(B, N, tc, perp, half, shrink, level=None, max_nodes=None):
    """Depth first over the levels d-1 .. 0.  A node (x_k .. x_{d-1}) is visited iff every partial distance
    perp + sum_{i >= j} (x_i - c_i)^2 r_i, j = d-1 .. k, is <= level[j] * N (level None: 1), and — with `half` — the first
    non-zero coefficient from the top is positive or all are zero.  The children of a node are found by stepping away
    from floor(c) in both directions while the (convex) distance stays within the bound.  With `shrink`, N drops to the
    norm of every leaf below it as soon as the leaf is met (the zero vector of a `half` walk excepted)."""
    d = len(B)
    mu, r = _gso(B)
    lev = [Fraction(1)] * d if level is None else [Fraction(v) for v in level]
    assert len(lev) == d
    if tc is None:
        tc, perp = [Fraction(0)] * d, Fraction(0)
    bound = [lv * N for lv in lev]
    out, x, nodes = [], [0] * d, [0]
    mut = [[mu[j][k] for j in range(d)] for k in range(d)]  # mut[k][j] = mu(j, k), j > k

    def visit(k, pd, zero_prefix):
        c = tc[k]
        row = mut[k]
        for j in range(k + 1, d):
            if x[j]:
                c = c - x[j] * row[j]
        rk = r[k]
        lo = _floor(c)
        for step, v in ((-1, lo), (1, lo + 1)):
            while True:
                if half and zero_prefix and v < 0:
                    break
                a = v - c
                nd = pd + a * a * rk
                if nd > bound[k]:
                    break
                nodes[0] += 1
                assert max_nodes is None or nodes[0] <= max_nodes, "the tree is larger than the exact reference is meant for"
                x[k] = v
                if k:
                    visit(k - 1, nd, zero_prefix and v == 0)
                elif not (half and zero_prefix and v == 0):
                    assert nd.denominator == 1  # |xB - t|^2 is an integer
                    nv = int(nd)
                    out.append((nv, tuple(x)))
                    if shrink and nv < bound[0]:
                        for i in range(d):
                            bound[i] = lev[i] * nv
                v += step
        x[k] = 0

    visit(d - 1, Fraction(perp), True)
    return sorted(out), nodes[0]


def short_exact(B, N, rows=None, level=None, max_nodes=None):
    """Every non-zero x with |xB|^2 <= N (one of +-x: the first non-zero coefficient from the top is positive), as
    (norm, x) sorted, and the number of visited nodes.  rows=k: the first k rows only.  level: [d] rational factors, the
    bound of level j is level[j] * N (a pruned tree)."""
    return _walk(_ints(B, rows), int(N), None, None, True, False, level, max_nodes)


def near_exact(B, t, N, max_nodes=None):
    """Every x with |xB - t|^2 <= N for the integer vector t, the zero difference included."""
    B = _ints(B)
    mu, r = _gso(B)
    tc, perp = _target_coord(B, mu, r, [int(v) for v in t])
    return _walk(B, int(N), tc, perp, False, False, None, max_nodes)


def lambda1_exact(B, rows=None, max_nodes=None):
    """(the minimal non-zero squared norm, all minimal x (one of +-x), nodes): the walk starts at the shortest row's
    norm and shrinks its bound to every shorter vector it meets."""
    B = _ints(B, rows)
    N = min(sum(v * v for v in row) for row in B)
    found, nodes = _walk(B, N, None, None, True, True, None, max_nodes)
    m = found[0][0]
    return m, [x for nv, x in found if nv == m], nodes


def closest_exact(B, t, max_nodes=None):
    """(the minimal |xB - t|^2, all x that reach it, nodes): starts at the distance of the nearest-plane point."""
    B = _ints(B)
    t = [int(v) for v in t]
    d = len(B)
    mu, r = _gso(B)
    tc, perp = _target_coord(B, mu, r, t)
    x = [0] * d
    for k in range(d - 1, -1, -1):
        c = tc[k] - sum((x[j] * mu[j][k] for j in range(k + 1, d)), Fraction(0))
        x[k] = _floor(c + Fraction(1, 2))
    N = sum((sum(x[i] * B[i][j] for i in range(d)) - t[j]) ** 2 for j in range(len(t)))
    found, nodes = _walk(B, N, tc, perp, False, True, None, max_nodes)
    m = found[0][0]
    return m, [x for nv, x in found if nv == m], nodes


def d_eff_exact(B):
    """last_useful_index (svpcvp.cpp:32-43) on the exact r_ii: 1 + the last i > 0 with r_ii <= 2 r_00, else 1."""
    _, r = _gso(_ints(B))
    d_eff = 1
    for i in range(1, len(r)):
        if r[i] <= 2 * r[0]:
            d_eff = i + 1
    return d_eff


def vector_of(B, x, t=None):
    """x B (- t) in Python integers."""
    n = len(B[0])
    v = [sum(int(x[i]) * int(B[i][j]) for i in range(len(B))) for j in range(n)]
    return v if t is None else [a - int(b) for a, b in zip(v, t)]


def partial_distances(B, x):
    """[pd_0 .. pd_{d-1}] of the coefficient vector x, pd_k = sum_{i >= k} (x_i - c_i)^2 r_i: exact rationals."""
    B = _ints(B)
    d = len(B)
    mu, r = _gso(B)
    pd, acc = [Fraction(0)] * d, Fraction(0)
    for k in range(d - 1, -1, -1):
        a = x[k] + sum((x[j] * mu[j][k] for j in range(k + 1, d)), Fraction(0))
        acc = acc + a * a * r[k]
        pd[k] = acc
    return pd


def target_perp(B, t):
    """|t - (its projection on the span of B)|^2: the part of every distance |xB - t|^2 that no x changes (0 for
    d = n), an exact rational."""
    B = _ints(B)
    mu, r = _gso(B)
    return _target_coord(B, mu, r, [int(v) for v in t])[1]
