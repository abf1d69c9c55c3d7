"""Inputs and exact checkers for the blocked (compact-WY, MFMA) Householder R-factor, hh_blocked_kernel<NQ> behind
fphip_hh_update_R_blocked (tests/test_hh_cases_cpu.py shows on the CPU that they are what they claim to be;
tests/test_hh_blocked_gpu.py launches the kernel on them).

The kernel is a template on NQ = (n + 63) / 64; a PANEL is 16 rows, a TILE 16 columns, the LDS row stride is n rounded up
to a multiple of 32, plus 1.  SHAPES are the smallest d x n that reach every instantiation and every edge of those: fewer
rows than a panel (no MFMA at all), d = 16 k and 16 k +- 1, a last tile / last 64-chunk of ONE column (65, 129, 193), n
at and next to a multiple of 32.  Four seeded families, a different lattice for every (d, n, lattice index):

  qary      the generator of test_rows_kernel_equals_the_column_kernel_bit_for_bit: q in [2^10, 2^30), [I | random] on
            top, dense + q on the diagonal below
  dense     uniform in +-2^s, s per lattice from 8 .. 40: neighbours in one launch differ by up to 2^32 in magnitude
  tri       lower triangular, +-1000 below the diagonal, +-[1, 2^20) on it (every third negative): every reflector is 0,
            R(i,j) = sign(b_jj) b_ij, R(i,i) = |b_ii| EXACTLY — both branches `f3 == 0` and `sigma = -1` at every NQ
  zero_row  a dense lattice with one row set to 0 (not the last one): R row 0, exponent 0, sigma +1, reflector 0

The yardstick is the true R-factor at 300 bits: wide_cases.cholesky (the lower Cholesky factor of the exact integer Gram
matrix) where the rows are independent; for zero_row, whose Gram matrix is singular, true_factor() below."""
import functools
import math

import numpy as np

import ftx_cases as F
import wide_cases as W

SHAPES = {1: ((1, 1), (1, 5), (15, 15), (16, 16), (17, 17), (33, 40), (64, 64)),
          2: ((17, 65), (48, 128), (65, 65), (100, 128)),
          3: ((17, 129), (33, 192), (129, 129)),
          4: ((17, 193), (49, 208), (32, 256))}
ALL_SHAPES = tuple(s for nq in sorted(SHAPES) for s in SHAPES[nq])
BATCH = 7          # lattices 0 .. 5 of a shape, and lattice 0 again at index 6
FAMILY_ORDER = ("dense", "qary", "tri", "zero_row", "qary", "dense")
STRIDE_SHAPES = ((17, 65), (17, 193))
STRIDE_BASES = 8
PREC = W.PREC
SEED = 0          # of every generator below


# ---- the launcher's arithmetic (fphip_hh_update_R_blocked, gso_host.hip), restated ------------------------------------
def nq_of(n):
    return (n + 63) // 64


def panels(d):
    return (d + 15) // 16


def last_tile_width(n):
    """columns of the last 16-column tile that has any (guard `16 * t < n`)"""
    return n - 16 * ((n - 1) // 16)


def last_chunk_width(n):
    """columns of the last 64-wide chunk (guard `c < n`)"""
    return n - 64 * (nq_of(n) - 1)


def lds_stride(n):
    return ((n + 31) & ~31) + 1


def blocks_per_cu(n):
    lds = (16 * lds_stride(n) + 256) * 8
    return min(16, (160 * 1024) // lds)


def grid_of(batch, n, cus):
    return min(batch, cus * blocks_per_cu(n))


# ---- families ---------------------------------------------------------------------------------------------------------
def _rng(family, d, n, lattice):
    return np.random.default_rng([SEED, ("qary", "dense", "tri", "zero_row").index(family), d, n, lattice])


def qary(d, n, lattice):
    rng = _rng("qary", d, n, lattice)
    q = int(rng.integers(1 << 10, 1 << 30))
    k = d // 2
    b = np.zeros((d, n), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, n - k))
    b[k:, :] = rng.integers(-q, q, size=(d - k, n))
    b[k:, :k] = 0
    for r in range(k, d):
        b[r, min(n - 1, r)] += q
    return b


def dense(d, n, lattice, family="dense"):
    rng = _rng(family, d, n, lattice)
    s = int(rng.integers(8, 41))
    return rng.integers(-(1 << s), (1 << s) + 1, size=(d, n), dtype=np.int64)


def tri(d, n, lattice):
    rng = _rng("tri", d, n, lattice)
    b = np.tril(rng.integers(-1000, 1001, size=(d, n), dtype=np.int64), -1)
    diag = rng.integers(1, 1 << 20, size=d, dtype=np.int64)
    diag[2::3] *= -1
    b[np.arange(d), np.arange(d)] = diag
    return b


def zero_row_index(d, n, lattice):
    """the zeroed row: never the last one; in the SECOND panel where d allows (the blocked kernel then takes it through
    the matrix cores and keeps a zero reflector in T), and early enough that true_factor() stays cheap"""
    assert d >= 2
    rng = _rng("zero_row", d, n, 1000 + lattice)
    lo, hi = (16, min(d - 1, 24)) if d >= 18 else (0, d - 1)
    return int(rng.integers(lo, hi))


def zero_row(d, n, lattice):
    b = dense(d, n, lattice, "zero_row")
    b[zero_row_index(d, n, lattice)] = 0
    return b


GENERATORS = {"qary": qary, "dense": dense, "tri": tri, "zero_row": zero_row}


def family_of(d, n, index):
    """family of the lattice at `index` of the launch of shape d x n (index 6 is index 0 again); d = 1 has no room for
    a zero row that is not the last one"""
    fam = FAMILY_ORDER[index % (BATCH - 1)]
    return "tri" if fam == "zero_row" and d < 2 else fam


@functools.lru_cache(maxsize=None)
def _lattice(d, n, lattice):
    b = GENERATORS[family_of(d, n, lattice)](d, n, lattice)
    b.setflags(write=False)
    return b


def launch(d, n):
    """[(family, basis)] of the launch of shape d x n: BATCH entries, read-only, the last one the first again"""
    idx = list(range(BATCH - 1)) + [0]
    return [(family_of(d, n, L), _lattice(d, n, L)) for L in idx]


# ---- the grid-stride launch -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stride_base(d, n, k):
    """base lattice k of 8 (dense and qary in turn; independent rows)"""
    b = (dense if k % 2 == 0 else qary)(d, n, 100 + k)
    b.setflags(write=False)
    return b


def stride_plan(batch, g):
    """(base, addend) per lattice of the grid-stride launch: the bases in turn, one further on every pass of the grid
    (the grid is a multiple of 8 on any device with a multiple of 8 CUs: without the turn a wave would meet the SAME base
    on every pass, and stale LDS would hold the right values); the addend is the lattice's own index, so that all are
    distinct.  Lattices g and g + 1 are lattices 0 and 1 again: the same input on a first and on a second pass."""
    L = np.arange(batch)
    base = (L + L // g) % STRIDE_BASES
    add = L.copy()
    for r in (0, 1):
        if g + r < batch:
            base[g + r], add[g + r] = base[r], add[r]
    return base, add


def stride_batch(d, n, batch, g):
    """[batch][d][n] int64: lattice L = base + addend at (d - 1, n - 1) — the last row, so that rows 0 .. d - 2 of R are
    those of the base, and the last column, alone in its tile and its chunk at n = 65 and 193"""
    base, add = stride_plan(batch, g)
    bases = np.stack([stride_base(d, n, k) for k in range(STRIDE_BASES)])
    bs = bases[base]
    bs[:, d - 1, n - 1] += add
    return bs, base, add


# ---- exact answers ----------------------------------------------------------------------------------------------------
def tri_expected(b):
    """the whole factorisation of a `tri` lattice in integers: tril(R) 2^row_expo, as exact doubles"""
    d = b.shape[0]
    sg = np.where(np.diag(b[:, :d]) < 0, -1, 1).astype(np.int64)
    R = np.tril(b[:, :d] * sg[None, :], -1)
    R[np.arange(d), np.arange(d)] = np.abs(np.diag(b[:, :d]))
    return R.astype(np.float64)


def scaled_tril(R, rexp):
    """tril(R[:, :d]) 2^row_expo[i] (exact: a power of two)"""
    d = R.shape[0]
    return np.ldexp(np.tril(R[:, :d]), np.asarray(rexp, dtype=np.int32)[:, None])


def _with_prec(fn):
    @functools.wraps(fn)
    def wrapped(*a, **k):
        old = F.mp.mp.prec
        F.mp.mp.prec = PREC + 128
        try:
            return fn(*a, **k)
        finally:
            F.mp.mp.prec = old
    return wrapped


@_with_prec
def _zero_row_factor(b, z):
    """True R-factor of a basis whose row z is 0 (the others independent), as the reference defines it: reflector z is
    the identity and sigma_z = +1 (householder.cpp:27-146 on a zero row), so R(i, z), i > z, is the z-th coordinate of
    b_i H_0 .. H_{z-1} = b_i . q with q = H_0 .. H_{z-1} e_z, and the later reflectors never touch that column.  q is a
    unit vector orthogonal to b_0 .. b_{z-1}: tril(R) is the Cholesky factor of the Gram matrix of (b_0 .. b_{z-1}, q,
    b_{z+1} ..) with row z set to 0 afterwards.  The Gram matrix decides everything but q, which depends on the
    reflectors themselves: H_j = 1 - 2 u u^T / |u|^2 maps the row x it is built from to sign(x_j) |x| e_j, u = x -
    sign(x_j) |x| e_j (the reference's v_j is u scaled to |v|^2 = 2).  Rows 0 .. z-1 are taken through that in mpmath at
    428 bits (z <= 24: cheap), the Cholesky recurrence in fixed point like wide_cases.cholesky_fixed."""
    mp = F.mp
    d, n = b.shape
    us = []
    for i in range(z):
        x = [mp.mpf(int(v)) for v in b[i]]
        for j, u in enumerate(us):
            if u is not None:
                s = 2 * mp.fdot(u[j:], x[j:]) / mp.fdot(u[j:], u[j:])
                for c in range(j, n):
                    x[c] -= s * u[c]
        tail = mp.fdot(x[i + 1:], x[i + 1:])
        if tail == 0:
            us.append(None)
            continue
        sg = -1 if x[i] < 0 else 1
        u = [mp.mpf(0)] * n
        u[i] = -tail / (x[i] + sg * mp.sqrt(x[i] * x[i] + tail))   # = x_i - sg |x| without the cancellation
        u[i + 1:] = x[i + 1:]
        us.append(u)
    q = [mp.mpf(0)] * n
    q[z] = mp.mpf(1)
    for j in range(z - 1, -1, -1):
        u = us[j]
        if u is not None:
            s = 2 * mp.fdot(u[j:], q[j:]) / mp.fdot(u[j:], u[j:])
            for c in range(j, n):
                q[c] -= s * u[c]
    sh = PREC + 128
    rows = np.array([[int(v) for v in row] for row in b], dtype=object)
    g = [[int(v) << (2 * sh) for v in row] for row in W._matmul_exact(rows, rows.T)]
    for i in range(d):
        c = int(mp.floor(mp.ldexp(mp.fdot(q, [int(v) for v in b[i]]), 2 * sh))) if i > z else 0
        g[i][z] = g[z][i] = c
    g[z][z] = 1 << (2 * sh)
    L = []
    for i in range(d):
        Li = []
        for j in range(i):
            Lj = L[j]
            Li.append((g[i][j] - sum(map(int.__mul__, Li, Lj))) // Lj[j])
        rad = g[i][i] - sum(x * x for x in Li)
        if rad <= 0:
            raise ValueError("the rows other than row %d are not independent" % z)
        Li.append(math.isqrt(rad))
        L.append(Li)
    L[z] = [0] * (z + 1)
    mp.mp.prec = PREC
    return [[mp.ldexp(mp.mpf(x), -sh) for x in Li] for Li in L]


@functools.lru_cache(maxsize=None)
def _true_factor(key):
    b = W._unkey(key)
    zero = [i for i in range(b.shape[0]) if not b[i].any()]
    if not zero:
        return W.cholesky(b)
    assert len(zero) == 1 and zero[0] < b.shape[0] - 1
    return _zero_row_factor(b, zero[0])


def true_factor(b):
    """rows L[i][0 .. i] (mpf, 300 bits) of the true R-factor of b; cached by the basis"""
    return _true_factor(W._key(b))


def factor_error(b, R, rexp):
    """worst |R(i,j) 2^row_expo[i] - L(i,j)| / |b_i| over j <= i against the true factor (an mpf): what
    wide_cases.r_factor_error(b, (R,), rexp) computes, which this calls where the rows of b are independent.  A zero row
    has no norm to measure against: its R must be 0 exactly (infinite error otherwise)."""
    mp = F.mp
    if all(b[i].any() for i in range(b.shape[0])):
        return W.r_factor_error(b, (R,), rexp)
    L = true_factor(b)
    old = mp.mp.prec
    mp.mp.prec = PREC
    try:
        worst = mp.mpf(0)
        for i in range(len(L)):
            if not b[i].any():
                if np.any(R[i, :i + 1] != 0.0):
                    return mp.inf
                continue
            rown = mp.sqrt(mp.fsum(int(v) * int(v) for v in b[i]))
            sc = mp.mpf(2) ** int(rexp[i])
            w = max(abs(mp.mpf(float(R[i, j])) * sc - L[i][j]) for j in range(i + 1))
            worst = max(worst, w / rown)
        return worst
    finally:
        mp.mp.prec = old


GATE_BITS = 4                 # "the same recurrence summed in another order" 
GATE_FLOOR = 2.0 ** -52       # one ulp of an entry the size of the row norm: where the reference is exact (d = 1)


def gate(err_exact_mode):
    """what the blocked kernel's error may be, given the exact mode's on the same lattice"""
    return 2 ** GATE_BITS * max(err_exact_mode, F.mp.mpf(GATE_FLOOR))


def gram_last_row(b):
    """b_{d-1} . b_j, j = 0 .. d-1, in Python integers"""
    last = [int(v) for v in b[-1]]
    return [sum(x * int(y) for x, y in zip(last, row)) for row in b]


@_with_prec
def last_row_factor(b, Lbase, gbase, add):
    """(last row of the true factor, |last row of the basis|) of b + add e_{d-1} e_{n-1}^T, given the true factor Lbase
    of b — rows 0 .. d-2 are shared — and gbase = gram_last_row(b): the Cholesky recurrence of that one row on Gram
    entries updated in integers"""
    mp = F.mp
    d, n = b.shape
    add = int(add)
    g = [gbase[j] + add * int(b[j, n - 1]) for j in range(d - 1)]
    gdd = gbase[d - 1] + 2 * add * int(b[d - 1, n - 1]) + add * add
    row = []
    for j in range(d - 1):
        row.append((g[j] - mp.fdot(row, Lbase[j][:j])) / Lbase[j][j])
    row.append(mp.sqrt(gdd - mp.fdot(row, row)))
    return row, mp.sqrt(mp.mpf(gdd))


def row_error(Lrow, rown, Rrow, e):
    """|R(i,j) 2^e - L(i,j)| / |b_i|, worst over the row (as a double: 53 bits of an error are plenty)"""
    mp = F.mp
    sc = mp.mpf(2) ** int(e)
    return float(max(abs(mp.mpf(float(x)) * sc - t) for x, t in zip(Rrow, Lrow)) / rown)


# ---- the stated tolerance on mu / r, against the exact Gram-Schmidt --------------------------------------------------------
REDUCED = ("q48", "c3_100", "c3_180", "q200")     # the reduced bases of test_blocked_mfma_mode_agrees_with_exact_mode
REDUCED_AT = 3                                    # index of the unperturbed basis among its five perturbations


@functools.lru_cache(maxsize=None)
def reduced_base(src):
    import conftest as C
    import os
    from fplll_amd.gso import load_basis_txt
    if src == "q48":
        b = C.load_gso_fixture(os.path.join(C.GOLDEN, "gso_q48_p3.json"))["b_out"]
    elif src == "q200":
        b = load_basis_txt(os.path.join(C.GOLDEN, W.TALL[4]))
    else:
        b = W.tall_base(3)[:int(src[3:]), :]
    b = np.ascontiguousarray(b, dtype=np.int64)
    b.setflags(write=False)
    return b


def reduced_launch(src):
    """six lattices: _unreduced_copy(base, 2, seed) for five seeds, the reduced basis itself at REDUCED_AT"""
    from fplll_amd.gso import _unreduced_copy
    b = reduced_base(src)
    bs = [_unreduced_copy(b, 2, seed) for seed in (11, 12, 13, 14, 15)]
    bs.insert(REDUCED_AT, b)
    return np.stack(bs)


@functools.lru_cache(maxsize=None)
def exact_mu_r(src):
    """(mu(i,j), r(i,j) = mu(i,j) r(j,j), R(i,i)) of the reduced basis from wide_cases.exact_gso(b, tall_family=True) —
    the 300-bit Cholesky factor —, each rounded ONCE to a double: 2^-53 relative, against a tolerance of 1e-9"""
    g = W.exact_gso(reduced_base(src), tall_family=True)
    mp = F.mp
    d = g.d
    mu, r, diag = np.zeros((d, d)), np.zeros((d, d)), np.zeros(d)
    old = mp.mp.prec
    mp.mp.prec = PREC
    try:
        for i in range(d):
            diag[i] = float(g.L[i][i])
            for j in range(i + 1):
                r[i, j] = float(g.L[i][j] * g.L[j][j])
                mu[i, j] = float(g.mu[i][j]) if j < i else 1.0
    finally:
        mp.mp.prec = old
    return mu, r, diag


def mu_r_violations(b, R, rexp, src="q48"):
    """number of (i, j), j < i resp. j <= i, where mu = R_ij / R_jj resp. r = R_ij R_jj of the given R-factor misses the
    exact value by more than 1e-9 max(1, |mu|) resp. 1e-9 max(|r|, R_ii R_jj) — the project's stated tolerance and the
    scales of test_blocked_mfma_mode_agrees_with_exact_mode, with the exact Gram-Schmidt on the other side"""
    assert np.array_equal(b, reduced_base(src))
    mu_x, r_x, diag_x = exact_mu_r(src)
    d = b.shape[0]
    Rt = scaled_tril(R, rexp)
    dg = np.diag(Rt)
    low = np.tril(np.ones((d, d), dtype=bool), -1)
    mu, r = Rt / dg[None, :], Rt * dg[None, :]
    bad_mu = np.abs(mu - mu_x) > 1e-9 * np.maximum(1.0, np.abs(mu_x))
    bad_r = np.abs(r - r_x) > 1e-9 * np.maximum(np.abs(r_x), np.outer(diag_x, diag_x))
    return int((bad_mu & low).sum()), int((bad_r & (low | np.eye(d, dtype=bool))).sum())
