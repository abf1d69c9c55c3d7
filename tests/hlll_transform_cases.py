"""The reference for the transformation matrix u that the Householder side carries (fphip_hh_enable_transform), and the
inputs it is checked on: tests/test_hlll_transform_cpu.py shows on the CPU that the reference is sound,
tests/test_hlll_transform_gpu.py compares the device's u with it.

No new oracle is needed: for a basis b_in of full row rank the U with U b_in = b_out is UNIQUE, so the u of the
reference (MatHouseholder(b, u, ...), whose u starts at the identity and takes every row operation b takes) is
determined by the b_out it returns — which the fixtures and the C oracle already provide.

Two exact ways to that U:
  elimination   wide_cases.solve_left_exact (fraction-free Gauss-Jordan on the Gram matrix; None = rank-deficient), then
                the quotient must be integral.  A second at 64 rows, three at 72, a minute and a half at 180
                (measured), so it is used up to ELIMINATION_ROWS rows, and beyond for bases that are not square.
  verification  for SQUARE bases of any size: b_in is shown non-singular by its determinant modulo a prime (a non-zero
                residue proves a non-zero determinant; exact int64 arithmetic), U is PROPOSED in floating point
                (solve, round) and VERIFIED in exact integers (U b_in = b_out on every entry).  A non-singular b_in has
                one solution, so a verified proposal is it; a wrong proposal can only make the check fail.
test_hlll_transform_cpu.py runs both on every square input of up to 72 rows and requires the same matrix."""
import functools
import os

import numpy as np

import conftest as C
import wide_cases as W

ELIMINATION_ROWS = 48
PRIME = 2147483647  # 2^31 - 1: residues and their products stay below 2^62


def nonsingular_mod_p(b, p=PRIME):
    """True if the square integer matrix b has a non-zero determinant modulo p — which proves det b != 0.  (False
    proves nothing.)  Gaussian elimination on residues, int64 throughout."""
    a = np.mod(np.asarray(b, dtype=np.int64), p)
    d = a.shape[0]
    assert a.shape == (d, d)
    for k in range(d):
        nz = np.nonzero(a[k:, k])[0]
        if nz.size == 0:
            return False
        piv = k + int(nz[0])
        if piv != k:
            a[[k, piv]] = a[[piv, k]]
        inv = pow(int(a[k, k]), p - 2, p)
        f = (a[k + 1:, k] * inv) % p
        a[k + 1:, k:] = (a[k + 1:, k:] - (f[:, None] * a[k, k:][None, :]) % p) % p
    return True


def transform_by_elimination(b_in, b_out):
    """The unique U with U b_in = b_out as an object array of Python integers, from wide_cases.solve_left_exact.
    Raises if b_in is rank-deficient, if U is not integral or if it misses an equation."""
    sol = W.solve_left_exact(b_in, b_out)
    assert sol is not None, "b_in is not of full row rank: U is not unique"
    num, den = sol
    assert all(v % den == 0 for row in num for v in row), "the solution is not integral"
    U = np.array([[v // den for v in row] for row in num], dtype=object)
    assert W._matmul_equals(U, np.asarray(b_in).astype(object), np.asarray(b_out).astype(object))
    return U


def transform_by_verification(b_in, b_out):
    """The same U for a SQUARE b_in (module docstring): non-singular modulo a prime, proposed in floating point,
    verified in exact integers."""
    b_in = np.asarray(b_in, dtype=np.int64)
    b_out = np.asarray(b_out, dtype=np.int64)
    assert b_in.shape == b_out.shape and b_in.shape[0] == b_in.shape[1]
    assert nonsingular_mod_p(b_in), "no proof that b_in is non-singular"
    U = np.rint(np.linalg.solve(b_in.astype(np.float64).T, b_out.astype(np.float64).T).T)
    assert np.all(np.isfinite(U)) and np.abs(U).max() < 2.0 ** 52
    U = U.astype(np.int64)
    assert W._matmul_equals(U, b_in, b_out), "the proposed U is not a solution"
    return U.astype(object)


@functools.lru_cache(maxsize=None)
def _unique(key_in, key_out):
    b_in, b_out = W._unkey(key_in), W._unkey(key_out)
    d, n = b_in.shape
    U = transform_by_verification(b_in, b_out) if d == n and d > ELIMINATION_ROWS else transform_by_elimination(b_in, b_out)
    U.setflags(write=False)
    return U


def unique_transform(b_in, b_out):
    """the unique integer U with U b_in = b_out ([d][d] Python integers, read-only); computed once per pair"""
    return _unique(W._key(b_in), W._key(b_out))


def is_unimodular(u):
    """|det u| = 1, exactly.  Up to ELIMINATION_ROWS rows by Bareiss; beyond, an integer W with W u = 1 is proposed in
    floating point and verified in exact integers (det W det u = 1 in integers leaves +-1), with Bareiss as the
    fallback."""
    u = np.asarray(u)
    d = u.shape[0]
    if d > ELIMINATION_ROWS and u.dtype != object:
        try:
            Wm = np.rint(np.linalg.inv(u.astype(np.float64)))
            if np.all(np.isfinite(Wm)) and np.abs(Wm).max() < 2.0 ** 52:
                if W._matmul_equals(Wm.astype(np.int64), u, np.eye(d, dtype=np.int64)):
                    return True
        except np.linalg.LinAlgError:
            pass
    return abs(W.bareiss_det(u)) == 1


def check_transform(u, b_in, b_out, unique=True):
    """what every test asks of a u that started at the identity: u b_in = b_out in exact integers, |det u| = 1, and
    (unique = True: b_out is the reference's) u is the unique solution, hence the reference's u"""
    assert W._matmul_equals(u, b_in, b_out)
    assert is_unimodular(u)
    if unique:
        assert np.array_equal(np.asarray(u).astype(object), unique_transform(b_in, b_out))


def seeded_unimodular(d, seed, additions=20, exchanges=3):
    """the identity after `additions` elementary row additions (row_i += c row_j, c = +-1, +-2) and `exchanges` row
    exchanges: unimodular, small entries, not the identity"""
    rng = np.random.default_rng([d, seed])
    u = np.eye(d, dtype=np.int64)
    for _ in range(additions):
        i, j = (int(x) for x in rng.choice(d, size=2, replace=False))
        u[i] += int(rng.choice(np.array([-2, -1, 1, 2]))) * u[j]
    for _ in range(exchanges):
        i, j = (int(x) for x in rng.choice(d, size=2, replace=False))
        u[[i, j]] = u[[j, i]]
    return u


# ---- the inputs ----------------------------------------------------------------------------------------------------
HLLL_FIXTURES = ("hlll_q40", "hlll_q72", "hlll_r30", "hlll_u24", "hlll_n64")


@functools.lru_cache(maxsize=None)
def hlll_fixture(name):
    return C.load_hlll_fixture(os.path.join(C.GOLDEN, name + ".json"))


def hhsr_pair(f):
    """(b_in, b_out) of an `hhsr` fixture: size_reduce(kappa, ...) rewrites row kappa alone"""
    b_out = f["b_in"].copy()
    b_out[f["kappa"]] = f["b_row"]
    return f["b_in"], b_out


def _qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b


HETEROGENEOUS = ((2, 0), (3, 1), (17, 0), (33, 2), (64, 0), (65, 0), (90, 0))
HETEROGENEOUS_BATCH = 6   # lattices 1 .. 3 on the waves behind the first of a workgroup, 4 and 5 on a second workgroup


def heterogeneous_batch(d, n_extra, count=HETEROGENEOUS_BATCH):
    """`count` different lattices of d x (d + n_extra): the construction and the seeds of
    test_hlll_gpu.py::test_seeded_vs_oracle_heterogeneous_batch, one lattice more"""
    rng = np.random.default_rng(2000 + d)
    n = d + n_extra
    bs = []
    for _ in range(count):
        if n_extra == 0 and d >= 4:
            b = _qary(rng, d, d // 2, int(rng.integers(50, 5000)))
        else:
            b = np.zeros((d, n), dtype=np.int64)
            b[:, :d] = np.eye(d, dtype=np.int64)
            lo = d - 1 if n_extra == 0 else d
            b[:, lo:] += rng.integers(-10**6, 10**6, size=(d, n - lo))
        bs.append(b)
    return bs


def soundness_cases():
    """(name, b_in, reference b_out) of every fixed input of tests/test_hlll_transform_gpu.py"""
    for name in HLLL_FIXTURES:
        f = hlll_fixture(name)
        yield name, f["b_in"], f["b_out"]
    for path in C.hhsr_fixtures():
        f = C.load_hhsr_fixture(path)
        yield (f["name"],) + hhsr_pair(f)
    for d, n in W.SHORT_WIDE:
        for L, b in enumerate(W.short_wide_batch(d, n)):
            yield "short%dx%d[%d]" % (d, n, L), b, W.oracle_hlll(b)[2]
    for nq in sorted(W.TALL):
        for L, b in enumerate(W.tall_batch(nq)):
            yield "tall%d[%d]" % (b.shape[0], L), b, W.oracle_hlll(b)[2]
