"""Inputs and exact checkers for the width classes of the reduction kernels (tests/test_wide_cases_cpu.py shows on the
CPU that they are what they claim to be; tests/test_width_classes_gpu.py launches the kernels on them).

Every reduction kernel is a template on NQ, the number of 64-wide chunks a lane holds: NQ = (max(d, n) + 63) / 64 for
the GSO side, (n + 63) / 64 for the Householder side, 1 .. 4.  Two families of inputs reach the wide instantiations:

  short-wide  d x n with d <= 40 rows and 128 .. 256 columns: NQ is decided by n alone, a lane's entries of mu / r / R
              (indexed by row) stay in its first register, the column chunks are all in use.  Row i is
              [e_i | a_i u + E | a'_i u' + E']: an identity, a planted rank-one part on the columns below the last chunk
              and ANOTHER one on the last chunk (a, a' ~ 1e5, u, u' small), noise E, E' of +-1000 on every column.  The
              short vectors of such a lattice are the combinations c with c.a ~ 0 AND c.a' ~ 0 (a simultaneous
              knapsack) weighed by the noise: LLL has hundreds of swaps to do, BKZ improves on it, every column
              counts, and without the last chunk it is another lattice.  u' is scaled so that the last chunk (a single
              column at n = 129 and n = 193) carries at least a quarter of every row's squared norm.
  tall        the committed reduced bases of 180 and 200 rows (NQ 3 and 4), perturbed the way
              test_nq4_lll_matches_oracle does: _unreduced_copy(base, 2, seed), then 24 exchanges of neighbouring
              rows, at least 4 of them with i >= 64 (NQ - 1); three seeds, so a launch holds three lattices.

The checkers are exact: lattice equality in integers, the reference's reducedness predicates (is_lll_reduced,
lll.cpp:226-257; is_hlll_reduced, hlll.cpp:507-585) on the rational Gram-Schmidt of the basis (short-wide) or on its
Cholesky factor at 300 bits (tall) with the parameters taken at the exact value of the doubles the call passes."""
import functools
import math
import os
from fractions import Fraction

import numpy as np

import conftest as C
import ftx_cases as F

SHORT_WIDE = ((16, 128), (16, 129), (20, 192), (20, 193), (24, 256))   # LLL and HLLL
SHORT_WIDE_BKZ = ((40, 129), (40, 193))
SHORT_WIDE_BKZS = ((40, 128),) + SHORT_WIDE_BKZ   # bkz_strategies: no other input of the suite has 65 .. 128 columns
SHORT_BATCH = 5
TALL = {3: "basis_q180_seed0_lll_bkz20.txt", 4: "basis_q200_seed7_lll.txt.gz"}
TALL_SEEDS = {3: (5, 6, 7), 4: (2, 4, 15)}
TALL_EXCHANGES, TALL_UPPER = 24, 4
PREC = 300   # bits of the tall family's Cholesky factor


def nq_of(d, n):
    return (max(d, n) + 63) // 64


def last_chunk(d, n):
    """first row / column index of the last 64-wide chunk"""
    return 64 * (nq_of(d, n) - 1)


# ---- short-wide ------------------------------------------------------------------------------------------------------
def short_wide(d, n, lattice):
    """lattice number `lattice` of shape d x n (module docstring), seeded from (d, n, lattice)"""
    assert d < n and d <= 64 < n
    rng = np.random.default_rng([d, n, lattice])
    lo = last_chunk(d, n)
    sign = lambda size: rng.choice(np.array([-1, 1]), size=size)  # noqa: E731
    a = sign(d) * rng.integers(50000, 100001, size=d)
    a2 = sign(d) * rng.integers(50000, 100001, size=d)
    u = sign(lo - d) * rng.integers(1, 4, size=lo - d)
    # |u'|^2 >= 2 |u|^2: with |a'_i| >= |a_i| / 2 the last chunk then has (|u'|^2 / 4) / (|u|^2 + |u'|^2 / 4) >= 1/3
    # of the planted part of every row, and the planted part is 1e4 times the noise
    w = n - lo
    s = int(np.ceil(np.sqrt(2.0 * float(np.dot(u, u)) / w)))
    u2 = sign(w) * rng.integers(s, 2 * s + 1, size=w)
    b = np.zeros((d, n), dtype=np.int64)
    b[:, :d] = np.eye(d, dtype=np.int64)
    b[:, d:lo] = np.outer(a, u)
    b[:, lo:] = np.outer(a2, u2)
    b[:, d:] += rng.integers(-1000, 1001, size=(d, n - d))
    return b


def short_wide_batch(d, n, count=SHORT_BATCH):
    return [short_wide(d, n, L) for L in range(count)]


def without_last_chunk(b):
    """the same rows with the columns of the last chunk zeroed"""
    z = b.copy()
    z[:, last_chunk(*b.shape):] = 0
    return z


def last_chunk_share(b):
    """per row: the part of the squared norm that the columns of the last chunk carry"""
    sq = b.astype(np.float64) ** 2
    return sq[:, last_chunk(*b.shape):].sum(axis=1) / sq.sum(axis=1)


# ---- tall ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tall_base(nq):
    from fplll_amd.gso import load_basis_txt
    b = load_basis_txt(os.path.join(C.GOLDEN, TALL[nq]))
    assert b.shape[0] == b.shape[1] and nq_of(*b.shape) == nq
    b.setflags(write=False)
    return b


def tall_exchanges(nq, seed):
    """the 24 positions i of the exchanges (rows i, i + 1): 20 anywhere, 4 in the last chunk, in a seeded order"""
    d = tall_base(nq).shape[0]
    rng = np.random.default_rng([nq, seed])
    pos = np.concatenate([rng.integers(0, d - 1, size=TALL_EXCHANGES - TALL_UPPER),
                          rng.integers(64 * (nq - 1), d - 1, size=TALL_UPPER)])
    return [int(i) for i in rng.permutation(pos)]


def tall(nq, seed):
    from fplll_amd.gso import _unreduced_copy
    b = _unreduced_copy(tall_base(nq), 2, seed)
    for i in tall_exchanges(nq, seed):
        b[[i, i + 1]] = b[[i + 1, i]]
    return b


def tall_batch(nq):
    return [tall(nq, s) for s in TALL_SEEDS[nq]]


# ---- the oracle's answers, computed once -------------------------------------------------------------------------------
def _key(b):
    b = np.ascontiguousarray(b, dtype=np.int64)
    return b.shape, b.tobytes()


def _unkey(key):
    return np.frombuffer(key[1], dtype=np.int64).reshape(key[0])


@functools.lru_cache(maxsize=None)
def _oracle_lll(key, flags):
    o = C.OracleGSO(_unkey(key))
    st, info = o.lll(flags=flags)
    out = o.b
    o.close()
    out.setflags(write=False)
    return int(st), tuple(int(x) for x in info), out


def oracle_lll(b, flags=0):
    """(status, info, reduced basis) of the C oracle's LLLReduction::lll; cached, the basis read-only"""
    return _oracle_lll(_key(b), int(flags))


@functools.lru_cache(maxsize=None)
def _oracle_hlll(key):
    st, out, info = C.oracle_hlll(_unkey(key))
    out.setflags(write=False)
    return int(st), tuple(int(x) for x in info), out


def oracle_hlll(b):
    """(status, info = (swaps, iterations), reduced basis) of the C oracle's HLLLReduction::hlll; cached"""
    return _oracle_hlll(_key(b))


def nodes64(info):
    return (int(info[1]) & 0xffffffff) | ((int(info[2]) & 0xffffffff) << 32)


@functools.lru_cache(maxsize=None)
def _oracle_bkz(key, beta, max_loops):
    o = C.OracleGSO(_unkey(key))
    st, info = o.bkz(beta, max_loops=max_loops)
    out = o.b
    o.close()
    out.setflags(write=False)
    return int(st), int(info[0]), nodes64(info), out


def oracle_bkz(b_lll, beta, max_loops=0):
    """(status, tours, nodes, basis) of the oracle's BKZ with empty strategies on an LLL-reduced basis; cached"""
    return _oracle_bkz(_key(b_lll), int(beta), int(max_loops))


@functools.lru_cache(maxsize=None)
def strategies(which):
    S = C.load_bkz_fixture(os.path.join(C.GOLDEN, "bkzs_q64_b40_%s.json" % which))["strategies"]
    return S


@functools.lru_cache(maxsize=None)
def _oracle_bkzs(key, beta, which, seed):
    o = C.OracleGSO(_unkey(key))
    st, info = o.bkz_param(beta, 0.99, 0.51, 0x4 | 0x80, 1, 1.1, strategies(which), seed)
    out = o.b
    o.close()
    out.setflags(write=False)
    return int(st), nodes64(info), int(info[3]), int(info[4]), out


def oracle_bkzs(b_lll, beta, which, seed=17):
    """(status, nodes, enumeration calls, rerandomisations, basis) of the oracle's one BKZ tour with the strategies of
    bkzs_q64_b40_<which>, BKZ_MAX_LOOPS | BKZ_GH_BND, on an LLL-reduced basis; cached"""
    return _oracle_bkzs(_key(b_lll), int(beta), which, int(seed))


# ---- exact checkers ----------------------------------------------------------------------------------------------------
def bareiss_det(m):
    """determinant of a square integer matrix, fraction-free (every division is exact)"""
    a = [[int(x) for x in row] for row in m]
    n = len(a)
    sign, prev = 1, 1
    for k in range(n - 1):
        if a[k][k] == 0:
            piv = next((r for r in range(k + 1, n) if a[r][k] != 0), None)
            if piv is None:
                return 0
            a[k], a[piv] = a[piv], a[k]
            sign = -sign
        akk, rk = a[k][k], a[k]
        for i in range(k + 1, n):
            ri, aik = a[i], a[i][k]
            a[i] = [0] * (k + 1) + [(ri[j] * akk - aik * rk[j]) // prev for j in range(k + 1, n)]
        prev = akk
    return sign * a[n - 1][n - 1] if n else 1


def _matmul_exact(u, b):
    """u b in exact integers.  A bound on every partial sum picks the arithmetic: below 2^53 the double-precision product
    is exact (every partial sum is an integer a double holds), below 2^62 the int64 one, Python integers otherwise."""
    u, b = np.asarray(u), np.asarray(b)
    if u.dtype != object and b.dtype != object:
        bound = int(np.abs(u).max(initial=0)) * int(np.abs(b).max(initial=0)) * u.shape[1]
        if bound < 2 ** 53:
            return (u.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)
        if bound < 2 ** 62:
            return u.astype(np.int64) @ b.astype(np.int64)
    return u.astype(object).dot(b.astype(object))


def _matmul_equals(u, b, want):
    got = _matmul_exact(u, b)
    return bool(np.array_equal(got, np.asarray(want).astype(got.dtype)))


def solve_left_exact(b_in, b_out):
    """The unique rational U with U b_in = b_out on the row space of b_in (d <= n independent rows), as (numerators
    [d][d], common denominator), or None if b_in is not of full row rank.  Fraction-free Gauss-Jordan (Bareiss: every
    division is exact) on [G | (b_out b_in^T)^T], G = b_in b_in^T the Gram matrix, which has rank d exactly when d
    columns of b_in are independent: d columns' worth of equations, and no pivoting (its leading minors are positive).
    The caller checks the remaining equations (U b_in = b_out on every column)."""
    b_in = np.asarray(b_in, dtype=np.int64)
    b_out = np.asarray(b_out, dtype=np.int64)
    d = b_in.shape[0]
    G = _matmul_exact(b_in, b_in.T)
    Ct = _matmul_exact(b_in, b_out.T)   # (b_out b_in^T)^T
    A = [[int(x) for x in G[i]] + [int(x) for x in Ct[i]] for i in range(d)]
    prev = 1
    for k in range(d):
        akk, rk = A[k][k], A[k]
        if akk <= 0:
            return None
        for i in range(d):
            if i != k:
                ri, aik = A[i], A[i][k]
                A[i] = [(akk * x - aik * y) // prev for x, y in zip(ri, rk)]
        prev = akk
    # now A = [det G . 1 | det G . U^T]
    return [[A[i][d + j] for i in range(d)] for j in range(d)], prev


@functools.lru_cache(maxsize=256)
def _same_lattice(key_in, key_out):
    b_in, b_out = _unkey(key_in), _unkey(key_out)
    if b_in.shape != b_out.shape:
        return False
    sol = solve_left_exact(b_in, b_out)
    if sol is None:
        return False
    num, den = sol
    if any(v % den for row in num for v in row):
        return False
    U = np.array([[v // den for v in row] for row in num], dtype=object)
    return _matmul_equals(U, b_in.astype(object), b_out.astype(object)) and abs(bareiss_det(U)) == 1


def same_lattice(b_in, b_out):
    """The rows of b_out generate the lattice of the d <= n independent rows of b_in: b_out = U b_in with U integral
    and |det U| = 1, all in exact integers — test_dd_gpu._same_lattice without its restriction to square bases.  U
    comes from elimination on d independent columns' worth of equations (solve_left_exact), is then checked on EVERY
    column (U b_in = b_out) and for its determinant (Bareiss)."""
    return _same_lattice(_key(b_in), _key(b_out))


def same_lattice_square(base, b_out):
    """Lattice equality of two SQUARE non-singular bases (the tall family: 180 and 200 rows, where exact elimination
    takes minutes): each basis is an INTEGRAL combination of the other.  The two integer matrices are proposed in
    floating point (solve, round) and verified in exact integers — V base = b_out and W b_out = base —, so a wrong
    proposal can only make the check fail; together they give W V = 1, hence |det V| = 1."""
    base = np.asarray(base, dtype=np.int64)
    b_out = np.asarray(b_out, dtype=np.int64)
    if base.shape != b_out.shape or base.shape[0] != base.shape[1]:
        return False
    try:
        V = np.rint(np.linalg.solve(base.astype(np.float64).T, b_out.astype(np.float64).T).T)
        W = np.rint(np.linalg.solve(b_out.astype(np.float64).T, base.astype(np.float64).T).T)
    except np.linalg.LinAlgError:
        return False
    if not (np.all(np.isfinite(V)) and np.all(np.isfinite(W))) or max(np.abs(V).max(), np.abs(W).max()) > 2.0 ** 52:
        return False
    return _matmul_equals(V.astype(np.int64), base, b_out) and _matmul_equals(W.astype(np.int64), b_out, base)


class ExactGSO:
    """mu(i,j), j < i, and r(i,i) of an integer basis in a field where the predicates below are decided exactly
    (fractions) or to 300 bits (mpmath: from the Cholesky factor L of the Gram matrix, mu(i,j) = L(i,j) / L(j,j),
    r(i,i) = L(i,i)^2); `num` converts the call's double parameters into that field without rounding."""

    def __init__(self, mu, r, num, L=None):
        self.mu, self.r, self.num, self.L = mu, r, num, L
        self.d = len(r)


@functools.lru_cache(maxsize=64)
def _rational_gso(key):
    mu, r = F.exact_gso(_unkey(key))
    return ExactGSO(mu, [r[i][i] for i in range(len(r))], Fraction)


def cholesky_fixed(b, prec=PREC):
    """ftx_cases.cholesky_rfactor(b, prec) — the exact R-factor of the integer basis b, rows L[i][0..i] as mpf — by the
    same recurrence in FIXED point on Python integers (values scaled by 2^(prec + 128), every quotient and square root
    rounded down): a 200 x 200 basis takes half a second where the mpmath loop takes five.  Pinned to
    ftx_cases.cholesky_rfactor at 300 bits in tests/test_wide_cases_cpu.py."""
    mp = F.mp
    sh = prec + 128
    rows = [[int(x) for x in row] for row in b]
    g = _matmul_exact(np.array(rows, dtype=object), np.array(rows, dtype=object).T)
    L = []
    for i in range(len(rows)):
        Li = []
        for j in range(i):
            Lj = L[j]
            Li.append(((int(g[i][j]) << (2 * sh)) - sum(map(int.__mul__, Li, Lj))) // Lj[j])
        rad = (int(g[i][i]) << (2 * sh)) - sum(x * x for x in Li)
        if rad <= 0:
            raise ValueError("the rows are not independent")
        Li.append(math.isqrt(rad))
        L.append(Li)
    old = mp.mp.prec
    mp.mp.prec = prec
    try:
        return [[mp.ldexp(mp.mpf(x), -sh) for x in Li] for Li in L]
    finally:
        mp.mp.prec = old


@functools.lru_cache(maxsize=64)
def _cholesky(key, prec):
    return cholesky_fixed(_unkey(key), prec)


def cholesky(b, prec=PREC):
    """the exact R-factor of b to `prec` bits (rows L[i][0..i], mpf); cached by the basis"""
    return _cholesky(_key(b), prec)


def exact_gso(b, tall_family=False):
    """ExactGSO of b: rational (ftx_cases.exact_gso) for the short-wide family, from the 300-bit Cholesky factor for the
    tall one"""
    if not tall_family:
        return _rational_gso(_key(b))
    mp = F.mp
    L = cholesky(b)
    old = mp.mp.prec
    mp.mp.prec = PREC
    try:
        mu = [[L[i][j] / L[j][j] for j in range(i)] for i in range(len(L))]
        r = [L[i][i] * L[i][i] for i in range(len(L))]
    finally:
        mp.mp.prec = old
    return ExactGSO(mu, r, mp.mpf, L)


def _at_prec(fn):
    @functools.wraps(fn)
    def wrapped(g, *a, **k):
        if g.num is Fraction:
            return fn(g, *a, **k)
        old = F.mp.mp.prec
        F.mp.mp.prec = PREC + 64
        try:
            return fn(g, *a, **k)
        finally:
            F.mp.mp.prec = old
    return wrapped


@_at_prec
def lll_violation(g, delta=0.99, eta=0.51, which=("size", "lovasz")):
    """None if the basis is (delta, eta)-LLL-reduced by the reference's predicate — |mu(i,j)| <= eta for j < i, and
    r(i,i) >= (delta - mu(i,i-1)^2) r(i-1,i-1) — with NO slack, otherwise the first violation in the reference's
    order: ("size", i, j) or ("lovasz", i).  `which` restricts the check to one of the two conditions."""
    de, et = g.num(delta), g.num(eta)
    for i in range(g.d if "size" in which else 0):
        for j in range(i):
            if abs(g.mu[i][j]) > et:
                return ("size", i, j)
    for i in range(1, g.d if "lovasz" in which else 0):
        m = g.mu[i][i - 1]
        if g.r[i] < (de - m * m) * g.r[i - 1]:
            return ("lovasz", i)
    return None


@_at_prec
def hlll_violation(g, delta=0.99, eta=0.51, theta=0.001, which=("size", "lovasz")):
    """None if the basis is HLLL-reduced by the reference's predicate on its exact R-factor (R(i,j) = mu(i,j)
    sqrt r(j,j), R(i,i) = sqrt r(i,i)): |R(i,j)| <= eta R(j,j) + theta R(i,i) for j < i and delta R(i-1,i-1)^2 <=
    R(i,i-1)^2 + R(i,i)^2.  The first is decided without the square roots: it holds when |mu(i,j)| <= eta, and
    otherwise exactly when (|mu(i,j)| - eta)^2 r(j,j) <= theta^2 r(i,i)."""
    de, et, th = g.num(delta), g.num(eta), g.num(theta)
    for i in range(g.d if "size" in which else 0):
        for j in range(i):
            ex = abs(g.mu[i][j]) - et
            if ex > 0 and ex * ex * g.r[j] > th * th * g.r[i]:
                return ("size", i, j)
    for i in range(1, g.d if "lovasz" in which else 0):
        m = g.mu[i][i - 1]
        if de * g.r[i - 1] > m * m * g.r[i - 1] + g.r[i]:
            return ("lovasz", i)
    return None


# ---- accuracy against the exact factor -----------------------------------------------------------------------------
def r_factor_error(b_out, planes, row_expo):
    """worst |R(i,j) - L(i,j)| / |b_i| over j <= i: R = the sum of the component planes times 2^row_expo[i] (what
    hlll(precision = p) left), L = the exact R-factor of b_out.  An mpf."""
    mp = F.mp
    L = cholesky(b_out)
    old = mp.mp.prec
    mp.mp.prec = PREC
    try:
        worst = mp.mpf(0)
        for i in range(len(L)):
            rown = mp.sqrt(mp.fsum(t * t for t in L[i]))
            sc = mp.mpf(2) ** int(row_expo[i])
            w = max(abs(mp.fsum(mp.mpf(float(p[i, j])) for p in planes) * sc - L[i][j]) for j in range(i + 1))
            worst = max(worst, w / rown)
        return worst
    finally:
        mp.mp.prec = old


def mu_r_error(b_out, mu_planes, r_planes, row_expo):
    """(worst |mu - exact| / max(1, |mu|) over j < i, worst |r(i,j) - exact| / r(i,i) over j <= i) of the planes
    lll_ex(p) kept (stored with the row exponents: mu 2^(e_i - e_j), r 2^(e_i + e_j)) against the exact Gram-Schmidt
    of b_out — mu(i,j) = L(i,j) / L(j,j), r(i,j) = L(i,j) L(j,j) from its exact R-factor: the scales of
    test_dd_gpu.test_lll_mu_and_r_at_53_106_212_bits_against_exact_gram_schmidt."""
    mp = F.mp
    L = cholesky(b_out)
    old = mp.mp.prec
    mp.mp.prec = PREC
    try:
        wm = wr = mp.mpf(0)
        e = [int(x) for x in row_expo]
        for i in range(len(L)):
            rii = L[i][i] * L[i][i]
            for j in range(i + 1):
                got = mp.fsum(mp.mpf(float(p[i, j])) for p in r_planes) * mp.mpf(2) ** (e[i] + e[j])
                wr = max(wr, abs(got - L[i][j] * L[j][j]) / rii)
                if j < i:
                    want = L[i][j] / L[j][j]
                    got = mp.fsum(mp.mpf(float(p[i, j])) for p in mu_planes) * mp.mpf(2) ** (e[i] - e[j])
                    wm = max(wm, abs(got - want) / max(1, abs(want)))
        return wm, wr
    finally:
        mp.mp.prec = old


def reference_gso_planes(b, prec):
    """The reference arithmetic on the same basis, for the cases where the conditioning of the basis and not the
    kernel decides the error: the recurrence of MatGSOInterface::update_gso_row — r(i,j) = g(i,j) - sum_k<j mu(j,k)
    r(i,k), mu(i,j) = r(i,j) / r(j,j), one term after the other — in mpmath with EVERY operation rounded to `prec`
    bits (53 or 106), on the exact integer Gram matrix rounded to `prec` bits.  Returns (mu planes, r planes): prec / 53
    [d][d] arrays of doubles whose sum is the value, the form mu_r_error reads (row exponents 0)."""
    mp = F.mp
    rows = [[int(x) for x in row] for row in b]
    d = len(rows)
    G = _matmul_exact(np.array(rows, dtype=object), np.array(rows, dtype=object).T)
    old = mp.mp.prec
    mp.mp.prec = prec
    try:
        mu = [[None] * i for i in range(d)]
        r = [[None] * (i + 1) for i in range(d)]
        for i in range(d):
            ri = r[i]
            for j in range(i + 1):
                s = mp.mpf(int(G[i][j]))
                for m, x in zip(mu[j] if j < i else mu[i], ri):   # k < j (zip stops at the shorter list)
                    s = s - m * x
                ri[j] = s
                if j < i:
                    mu[i][j] = s / r[j][j]
        planes = prec // 53
        pm = [np.zeros((d, d)) for _ in range(planes)]
        pr = [np.zeros((d, d)) for _ in range(planes)]
        mp.mp.prec = 2 * prec
        for i in range(d):
            for j in range(i + 1):
                for pl, v in ((pr, r[i][j]),) + (((pm, mu[i][j]),) if j < i else ()):
                    for k in range(planes):
                        pl[k][i, j] = float(v)
                        v = v - mp.mpf(pl[k][i, j])
        return pm, pr
    finally:
        mp.mp.prec = old


def reference_gso_error(b, prec):
    """mu_r_error of reference_gso_planes(b, prec): what `prec` bits can give on this basis"""
    pm, pr = reference_gso_planes(b, prec)
    return mu_r_error(b, pm, pr, np.zeros(len(b), dtype=np.int64))


def log2(x):
    return float(F.mp.log(x, 2)) if x else float("-inf")


if __name__ == "__main__":
    # the table REFERENCE_ARITHMETIC of tests/test_width_classes_gpu.py
    for nq_ in sorted(TALL):
        for prec_ in (53, 106):
            errs = [reference_gso_error(oracle_lll(b_)[2], prec_) for b_ in tall_batch(nq_)]
            print("tall%d at %d bits: mu 2^%.1f, r 2^%.1f" % (tall_base(nq_).shape[0], prec_,
                                                            max(log2(e[0]) for e in errs), max(log2(e[1]) for e in errs)))
