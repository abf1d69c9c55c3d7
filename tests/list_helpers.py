"""Shared by the list-mode tests (test_enum_list_*.py): integer bases with known numbers of short vectors, their exact
Gram-Schmidt data, an exact LLL for the Leech basis of the reference's test_list_cvp, and the call that puts sentinels
behind the output arrays of fphip_enum_list.  No GPU needed to import."""
import ctypes
import os
from fractions import Fraction

import numpy as np

import conftest as C

LEECH_FILE = os.path.join(C.GOLDEN, "leech_example_list_cvp_in_lattice.txt")


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def gso_exact(B):
    """(mu, r) of the integer basis B (rows), in rational arithmetic: mu[k][j] for j < k, r[k] = |b*_k|^2."""
    n = len(B)
    bs, mu, r = [], [[Fraction(0)] * n for _ in range(n)], []
    for k in range(n):
        v = [Fraction(x) for x in B[k]]
        for j in range(k):
            mu[k][j] = _dot(B[k], bs[j]) / r[j]
            v = [a - mu[k][j] * b for a, b in zip(v, bs[j])]
        bs.append(v)
        r.append(_dot(v, v))
    return mu, r


def block_of(B):
    """(mut, rdiag) as the enumeration takes them — mut[i][j] = mu(j, i) for j > i — each entry the double nearest to
    the exact rational."""
    mu, r = gso_exact(B)
    n = len(B)
    mut = np.zeros((n, n))
    for k in range(n):
        for j in range(k):
            mut[j, k] = float(mu[k][j])
    return mut, np.array([float(v) for v in r])


def target_of(B, coeffs):
    """The target sum_j coeffs[j] b_j (rational coefficients) in the coordinates the enumeration takes:
    target[i] = coeffs[i] + sum_{j > i} coeffs[j] mu(j, i)."""
    mu, _ = gso_exact(B)
    n = len(B)
    a = [Fraction(c) for c in coeffs]
    return np.array([float(a[i] + sum(a[j] * mu[j][i] for j in range(i + 1, n))) for i in range(n)])


def lll_exact(B, delta=Fraction(3, 4)):
    """Textbook LLL in rational arithmetic (small bases only): returns the reduced integer basis."""
    B = [[int(x) for x in row] for row in B]
    n = len(B)
    bs, mu, r = [None] * n, [[Fraction(0)] * n for _ in range(n)], [Fraction(0)] * n

    def upd(k):
        v = [Fraction(x) for x in B[k]]
        for j in range(k):
            mu[k][j] = _dot(B[k], bs[j]) / r[j]
            v = [a - mu[k][j] * b for a, b in zip(v, bs[j])]
        bs[k], r[k] = v, _dot(v, v)

    upd(0)
    k = 1
    while k < n:
        upd(k)
        for j in range(k - 1, -1, -1):
            q = round(mu[k][j])
            if q:
                B[k] = [a - q * b for a, b in zip(B[k], B[j])]
                for i in range(j):
                    mu[k][i] -= q * mu[j][i]
                mu[k][j] -= q
        if r[k] >= (delta - mu[k][k - 1] ** 2) * r[k - 1]:
            k += 1
        else:
            B[k], B[k - 1] = B[k - 1], B[k]
            upd(k - 1)
            k = max(k - 1, 1)
    return B


def z8_basis():
    """A unimodular basis of Z^8 that is not the identity and whose mu is not zero (and not integral): L U with L
    unit lower and U unit upper triangular."""
    rng = np.random.default_rng(8)
    L = np.tril(rng.integers(-1, 2, size=(8, 8)), -1) + np.eye(8, dtype=np.int64)
    U = np.triu(rng.integers(-1, 2, size=(8, 8)), 1) + np.eye(8, dtype=np.int64)
    B = (L @ U).astype(np.int64)
    assert round(abs(np.linalg.det(B))) == 1
    return [[int(v) for v in row] for row in B]


def d4_basis():
    return [[1, 1, 0, 0], [1, -1, 0, 0], [0, 1, -1, 0], [0, 0, 1, -1]]


def e8_basis():
    """(B, 4): an integer basis of 2 E8 — seven generators of 2 D8 and the doubled glue vector (1/2)^8; determinant 2^8,
    so the sublattice of 2 E8 they span is all of it — and the factor its squared norms carry (minimum 8 = 4 * 2)."""
    B = [[2, 2, 0, 0, 0, 0, 0, 0], [2, -2, 0, 0, 0, 0, 0, 0], [0, 2, -2, 0, 0, 0, 0, 0], [0, 0, 2, -2, 0, 0, 0, 0],
         [0, 0, 0, 2, -2, 0, 0, 0], [0, 0, 0, 0, 2, -2, 0, 0], [0, 0, 0, 0, 0, 2, -2, 0], [1, 1, 1, 1, 1, 1, 1, 1]]
    return B, 4


_leech = {}


def leech_basis():
    """The basis of the reference's test_list_cvp (its data file, a golden here), LLL-reduced; computed once."""
    if "B" not in _leech:
        txt = open(LEECH_FILE).read().replace("[", " ").replace("]", " ")
        v = [int(t) for t in txt.split()]
        assert len(v) == 576
        _leech["B"] = lll_exact([v[24 * i:24 * i + 24] for i in range(24)])
    return _leech["B"]


def records(res):
    """[(dist as hex, x as a tuple of floats)] of a ListResult, in the order it came."""
    return [(float(a).hex(), tuple(float(v) for v in row)) for a, row in zip(res.dist, res.x)]


def bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def canonical(log):
    """The canonical order of a list: distance, then the coefficients from the top level down."""
    return bits(sorted(((a, tuple(x)) for a, x in log), key=lambda t: (t[0], t[1][::-1])))


def raw_list(ctx, mut, rdiag, pruning, radius, target, cap, guard=4):
    """fphip_enum_list with `guard` records of sentinel behind the cap records of both output arrays.  Returns
    (count, dist[cap + guard], x[cap + guard, d], nodes)."""
    from fplll_amd import _lib
    lib = ctx.lib
    mut = np.ascontiguousarray(mut, dtype=np.float64)
    d = mut.shape[0]
    rdiag = np.ascontiguousarray(rdiag, dtype=np.float64)
    lib.fphip_enum_list.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.POINTER(_lib.EnumStats)]
    lib.fphip_enum_list.restype = ctypes.c_int
    SENT = -12345.5
    dist = np.full(cap + guard, SENT)
    x = np.full((cap + guard, d), SENT)
    count = ctypes.c_uint64(0)
    nodes = np.zeros(d + 1, dtype=np.uint64)
    pr = None if pruning is None else np.ascontiguousarray(pruning, dtype=np.float64)
    tg = None if target is None else np.ascontiguousarray(target, dtype=np.float64)
    rc = lib.fphip_enum_list(ctx.handle, d, ctypes.c_double(radius), mut.ctypes.data_as(ctypes.c_void_p),
                             rdiag.ctypes.data_as(ctypes.c_void_p),
                             None if pr is None else pr.ctypes.data_as(ctypes.c_void_p),
                             None if tg is None else tg.ctypes.data_as(ctypes.c_void_p), cap,
                             dist.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count),
                             nodes.ctypes.data_as(ctypes.c_void_p), None)
    assert rc == 0, ctx.last_error()
    return int(count.value), dist, x, nodes, SENT
