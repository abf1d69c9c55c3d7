"""An exact reference for the solvers of quadratic forms: the rational LDL^T of an integer Gram matrix and a
Fincke-Pohst enumeration over it.  No GPU, no float: every comparison is between rationals, every norm that is returned
is a Python integer.  The conventions are exact_lattice.py's — one of each pair +-x (the first non-zero coefficient
from the top is positive), lists sorted by (norm, x), `nodes` counts every visited tree node (the zero leaf included),
a node cap — so that short_exact_form(B B^T, N) equals exact_lattice.short_exact(B, N) as a list.  It shares nothing
with the kernels or with tests/svp_gram_model.py.

  ldl_exact(G)                                        -> (mu, r): G = L D L^T, L = 1 + mu (lower), D = diag(r), Fractions
  short_exact_form(G, N, rows=None, level=None, max_nodes=None) -> ([(norm, x)], nodes)   0 < x G x^T <= N
  lambda1_exact_form(G, rows=None, max_nodes=None)    -> (norm, [x], nodes)   the minimum and every minimal vector
  d_eff_exact_form(G)                                 -> last_useful_index (svpcvp.cpp:32-43) on the exact r_ii
  sqnorm(G, x)                                        -> x G x^T

G is [d][d] Python integers, symmetric and positive definite (anything else: ValueError).
"""
from fractions import Fraction

_ldl_cache = {}


def _ints(G, rows=None):
    G = [[int(v) for v in row] for row in G]
    if rows is not None:
        G = [row[:rows] for row in G[:rows]]
    return G


def ldl_exact(G):
    G = _ints(G)
    key = tuple(tuple(row) for row in G)
    if key not in _ldl_cache:
        d = len(G)
        if any(len(row) != d for row in G) or any(G[i][j] != G[j][i] for i in range(d) for j in range(i)):
            raise ValueError("the form is not a symmetric square matrix")
        mu = [[Fraction(0)] * d for _ in range(d)]
        r = [Fraction(0)] * d
        rr = [[Fraction(0)] * d for _ in range(d)]  # r(i, j) = g_ij - sum_{k < j} mu(j, k) r(i, k)
        for i in range(d):
            for j in range(i + 1):
                v = Fraction(G[i][j]) - sum((mu[j][k] * rr[i][k] for k in range(j)), Fraction(0))
                rr[i][j] = v
                if j < i:
                    mu[i][j] = v / r[j]
            r[i] = rr[i][i]
            if r[i] <= 0:
                raise ValueError("the form is not positive definite (r_%d%d = %s)" % (i, i, r[i]))
        _ldl_cache[key] = (mu, r)
    return _ldl_cache[key]


def sqnorm(G, x):
    d = len(x)
    return sum(int(x[i]) * int(G[i][j]) * int(x[j]) for i in range(d) for j in range(d) if x[i] and x[j])


def _floor(c):
    return c.numerator // c.denominator


def _walk(G, N, shrink, level=None, max_nodes=None):
    """Depth first over the levels d-1 .. 0.  A node (x_k .. x_{d-1}) is visited iff every partial norm
    sum_{i >= j} (x_i + sum_{l > i} mu(l, i) x_l)^2 r_i, j = d-1 .. k, is <= level[j] * N (level None: 1) and the first
    non-zero coefficient from the top is positive or all are zero.  With `shrink`, N drops to the norm of every leaf
    below it as soon as the leaf is met."""
    d = len(G)
    mu, r = ldl_exact(G)
    lev = [Fraction(1)] * d if level is None else [Fraction(v) for v in level]
    assert len(lev) == d
    bound = [lv * N for lv in lev]
    out, x, nodes = [], [0] * d, [0]
    mut = [[mu[j][k] for j in range(d)] for k in range(d)]  # mut[k][j] = mu(j, k), j > k

    def visit(k, pd, zero_prefix):
        c = Fraction(0)
        row = mut[k]
        for j in range(k + 1, d):
            if x[j]:
                c = c - x[j] * row[j]
        rk = r[k]
        lo = _floor(c)
        for step, v in ((-1, lo), (1, lo + 1)):
            while True:
                if zero_prefix and v < 0:
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
                elif not (zero_prefix and v == 0):
                    assert nd.denominator == 1  # x G x^T is an integer
                    nv = int(nd)
                    out.append((nv, tuple(x)))
                    if shrink and nv < bound[0]:
                        for i in range(d):
                            bound[i] = lev[i] * nv
                v += step
        x[k] = 0

    visit(d - 1, Fraction(0), True)
    return sorted(out), nodes[0]


def short_exact_form(G, N, rows=None, level=None, max_nodes=None):
    """Every non-zero x with x G x^T <= N (one of +-x), as (norm, x) sorted, and the number of visited nodes.  rows=k:
    the leading k x k form only.  level: [d] rational factors, the bound of level j is level[j] * N (a pruned tree)."""
    return _walk(_ints(G, rows), int(N), False, level, max_nodes)


def lambda1_exact_form(G, rows=None, max_nodes=None):
    """(the minimal non-zero value, all minimal x (one of +-x), nodes): the walk starts at the smallest diagonal entry
    and shrinks its bound to every shorter vector it meets."""
    G = _ints(G, rows)
    N = min(G[i][i] for i in range(len(G)))
    found, nodes = _walk(G, N, True, None, max_nodes)
    m = found[0][0]
    return m, [x for nv, x in found if nv == m], nodes


def d_eff_exact_form(G):
    """last_useful_index (svpcvp.cpp:32-43) on the exact r_ii: 1 + the last i > 0 with r_ii <= 2 r_00, else 1."""
    _, r = ldl_exact(G)
    d_eff = 1
    for i in range(1, len(r)):
        if r[i] <= 2 * r[0]:
            d_eff = i + 1
    return d_eff
