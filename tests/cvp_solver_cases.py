"""The closest-vector solver's host-side twin: fixtures, and Python restatements of what the device computes.

  * ``prepare``      the target preparation kernel (csrc/cvp_prepare.hip; closest_vector's Babai loop,
                     svpcvp.cpp:571-597) in the SAME operation order, in IEEE double: numpy element-wise operations
                     over the axis of the targets (one multiply, one add at a time — numpy never contracts), the loops
                     over rows and columns as the kernel has them.  The kernel must agree with it bit for bit.
  * ``babai``        MatGSOInterface::babai (gso_interface.cpp:292-311), likewise.
  * ``prepare_mp``   the same preparation in mpmath at 200 bits on an exact-Gram GSO: what the reference's MPFR run
                     computes up to its own rounding; its roundings are compared with the double ones.
  * ``enumerate_cvp`` a plain double closest-vector enumeration at a fixed radius (the uniqueness condition of the
                     solver fixtures).
  * ``gso_double``   a double Gram-Schmidt of an integer basis for the CPU tests (the GPU tests feed ``prepare`` the
                     device's own mu / r / row exponents).
"""
import glob
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_PASSES = 0x100
I63 = 2**63


def load(name):
    p = os.path.join(GOLDEN, name)
    with (gzip.open(p, "rt") if p.endswith(".gz") else open(p)) as f:
        return json.load(f)


def solver_fixtures():
    """[(name, fixture)] of tests/golden/cvpsolve_*.json (closest_vector_ref_driver's records), sorted."""
    return [(os.path.basename(p), load(os.path.basename(p)))
            for p in sorted(glob.glob(os.path.join(GOLDEN, "cvpsolve_*.json")))]


def basis_of(fx):
    return np.array(fx["basis"], dtype=np.int64)


def targets_of(fx):
    return np.array([t["target"] for t in fx["targets"]], dtype=np.int64)


def overflow_case():
    """(b, true mu, true r_ii, targets) of a 2 x 2 basis and three targets of which the first leaves the 63-bit
    range: b = (1, 0), (2^20, 1) (its Gram matrix is exact in double); the target (0, 2^50) has the coordinate 2^50
    along row 1, and 2^50 times the entry 2^20 is 2^70.  The other two stay in range ((5, 7) and the origin)."""
    b = np.array([[1, 0], [2**20, 1]], dtype=np.int64)
    mu, rd = true_values(*gso_double(b), None)
    return b, mu, rd, np.array([[0, 2**50], [5, 7], [0, 0]], dtype=np.int64)


def gso_double(b):
    """(mu, r) in double from the exact integer Gram matrix: r(i,j) = g(i,j) - sum_{k<j} mu(j,k) r(i,k)."""
    bo = np.asarray(b).astype(object)
    d = bo.shape[0]
    g = bo.dot(bo.T)
    mu = np.zeros((d, d))
    r = np.zeros((d, d))
    for i in range(d):
        for j in range(i + 1):
            acc = float(g[i, j])
            for k in range(j):
                acc -= mu[j, k] * r[i, k]
            r[i, j] = acc
            if j < i:
                mu[i, j] = acc / r[j, j]
    return mu, r


def true_values(mu_st, r_st, rexp):
    """The stored mu / r of a GSO with row exponents -> the true mu [d][d] (strictly lower) and r_ii [d]
    (get_mu_exp / get_r_exp: mu 2^(e_i - e_j), r 2^(2 e_i)); rexp None: no exponents."""
    mu_st = np.asarray(mu_st, dtype=np.float64)
    d = mu_st.shape[0]
    e = np.zeros(d, dtype=np.int64) if rexp is None else np.asarray(rexp, dtype=np.int64)
    mu = np.tril(np.ldexp(mu_st, (e[:, None] - e[None, :]).astype(np.int32)), -1)
    rd = np.ldexp(np.ascontiguousarray(np.diag(np.asarray(r_st, dtype=np.float64))), (2 * e).astype(np.int32))
    return mu, rd


def round_away(x):
    """round(): the nearest integer, ties away from zero (mpfr_round); x - trunc(x) is exact in double."""
    x = np.asarray(x, dtype=np.float64)
    tr = np.trunc(x)
    return tr + np.where(np.abs(x - tr) >= 0.5, np.copysign(1.0, x), 0.0)


def _fits63(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) < 9223372036854775808.0  # (False for a NaN)


def descent_of(mu, rd, tc):
    """The rounding descent from target_coord [T][d] (prepare_enumeration's operand order): (x [T][d], dist [T])."""
    T, d = tc.shape
    x = np.zeros((T, d))
    dist = np.zeros(T)
    for k in range(d - 1, -1, -1):
        nc = tc[:, k].copy()
        for j in range(k + 1, d):
            nc = nc - x[:, j] * mu[j, k]
        x[:, k] = round_away(nc)
        alpha = x[:, k] - nc
        dist = dist + alpha * alpha * rd[k]
    return x, dist


def prepare(b, mu, rd, targets, max_passes=MAX_PASSES):
    """cvp_prepare_kernel, restated.  b int [d][n]; mu, rd: the TRUE values (true_values); targets int [T][n].
    Returns dict(coef int64 [T][d], target_coord [T][d], descent [T], status [T], passes [T])."""
    bo = np.asarray(b).astype(object)
    bf = np.asarray(b, dtype=np.int64).astype(np.float64)
    d, n = bf.shape
    tg = np.asarray(targets).astype(object).copy()
    T = tg.shape[0]
    coef = np.zeros((T, d), dtype=object)
    tcoord = np.zeros((T, d))
    status = np.zeros(T, dtype=np.int32)
    passes = np.zeros(T, dtype=np.int32)
    prev = {}  # target -> the x of its pass before
    for p in range(max_passes + 1):
        act = np.nonzero(status == 0)[0]
        if len(act) == 0:
            break
        if p >= max_passes:
            status[act] = -1
            break
        passes[act] += 1
        v = tg[act].astype(np.float64)
        c = np.zeros((len(act), d))
        for i in range(d):
            acc = np.zeros(len(act))
            for j in range(n):
                acc = acc + v[:, j] * bf[i, j]
            for j in range(i):
                acc = acc - mu[i, j] * c[:, j]
            c[:, i] = acc
        for i in range(d):
            c[:, i] = c[:, i] / rd[i]
        x = c.copy()
        for i in range(d - 1, -1, -1):
            x[:, i] = round_away(x[:, i])
            for j in range(i):
                x[:, j] = x[:, j] - mu[i, j] * x[:, i]
        with np.errstate(invalid="ignore"):
            small = np.all((x >= -1.0) & (x <= 1.0), axis=1)
        for a, t in enumerate(act):
            # a pass that would undo the one before (x == -x_before: the loop alternates between two targets, as on a
            # target exactly halfway between two lattice points) ends the loop like a small x does
            undo = t in prev and bool(np.all(x[a] == -prev[t]))
            prev[t] = x[a].copy()
            if small[a] or undo:
                status[t] = 1
                tcoord[t] = c[a]
                continue
            ok = bool(np.all(_fits63(x[a])))
            if ok:
                ci = np.array([int(u) for u in x[a]], dtype=object)
                nk = coef[t] + ci
                ok = all(-I63 <= int(u) < I63 for u in nk)
                cur = tg[t].copy()
                for i in range(d):
                    if not ok:
                        break
                    if ci[i] == 0:
                        continue
                    prod = ci[i] * bo[i]
                    cur = cur - prod
                    ok = all(-I63 <= int(u) < I63 for u in prod) and all(-I63 <= int(u) < I63 for u in cur)
                if ok:
                    coef[t] = nk
                    tg[t] = cur
            if not ok:
                status[t] = -2
    good = status == 1
    coef[~good] = 0
    tcoord[~good] = 0.0
    _, desc = descent_of(mu, rd, tcoord)
    desc[~good] = 0.0
    return dict(coef=coef.astype(np.int64), target_coord=tcoord, descent=desc, status=status, passes=passes)


def babai(mu, v, start=0, dimension=-1):
    """cvp_babai_kernel, restated: v [T][dimension] doubles -> (w int64 [T][dimension], status [T])."""
    d = mu.shape[0]
    if dimension == -1:
        dimension = d - start
    x = np.array(v, dtype=np.float64).reshape(-1, dimension).copy()
    for i in range(dimension - 1, -1, -1):
        x[:, i] = np.rint(x[:, i])
        for j in range(i):
            x[:, j] = x[:, j] - mu[start + i, start + j] * x[:, i]
    ok = np.all(_fits63(x), axis=1)
    w = np.zeros(x.shape, dtype=np.int64)
    w[ok] = x[ok].astype(np.int64)
    return w, np.where(ok, 1, -2).astype(np.int32)


def prepare_mp(b, target, prec=200, max_passes=MAX_PASSES):
    """The preparation of ONE target in mpmath at `prec` bits on the GSO of the exact Gram matrix.  Returns
    dict(coef [d] ints, descent_x [d] ints, passes, margin) — margin: the smallest distance of a value that was
    rounded (every pass's nearest-plane centres, the descent's) to a half-integer."""
    import mpmath as mp
    with mp.workprec(prec):
        bo = [[int(u) for u in row] for row in np.asarray(b).astype(object)]
        d, n = len(bo), len(bo[0])
        g = [[sum(bo[i][k] * bo[j][k] for k in range(n)) for j in range(d)] for i in range(d)]
        mu = [[mp.mpf(0)] * d for _ in range(d)]
        r = [[mp.mpf(0)] * d for _ in range(d)]
        for i in range(d):
            for j in range(i + 1):
                acc = mp.mpf(g[i][j])
                for k in range(j):
                    acc -= mu[j][k] * r[i][k]
                r[i][j] = acc
                if j < i:
                    mu[i][j] = acc / r[j][j]
        margin = [mp.mpf(1)]

        def rnd(c):
            fl = mp.floor(c)
            margin[0] = min(margin[0], abs(c - fl - mp.mpf(0.5)))
            return int(mp.floor(c + mp.mpf(0.5))) if c >= 0 else -int(mp.floor(-c + mp.mpf(0.5)))

        def gscoords(t):
            c = []
            for i in range(d):
                acc = mp.mpf(sum(t[j] * bo[i][j] for j in range(n)))
                for j in range(i):
                    acc -= mu[i][j] * c[j]
                c.append(acc)
            return [c[i] / r[i][i] for i in range(d)]

        t = [int(u) for u in target]
        coef = [0] * d
        passes = 0
        while True:
            passes += 1
            assert passes <= max_passes
            c = gscoords(t)
            x = list(c)
            xi = [0] * d
            for i in range(d - 1, -1, -1):
                xi[i] = rnd(x[i])
                for j in range(i):
                    x[j] -= mu[i][j] * xi[i]
            if all(-1 <= u <= 1 for u in xi):
                break
            for i in range(d):
                coef[i] += xi[i]
                for j in range(n):
                    t[j] -= xi[i] * bo[i][j]
        dx = [0] * d
        for k in range(d - 1, -1, -1):
            nc = c[k]
            for j in range(k + 1, d):
                nc -= dx[j] * mu[j][k]
            dx[k] = rnd(nc)
        return dict(coef=coef, descent_x=dx, passes=passes, margin=float(margin[0]))


def enumerate_cvp(mu, rd, tc, R, max_nodes=200000):
    """Every x with sum_i (x_i - c_i)^2 r_ii <= R, c_i = tc_i - sum_{j>i} x_j mu(j,i), in double (depth first, the
    partial distances cut at R).  Returns [(dist, x tuple)] sorted; asserts the tree stays below max_nodes."""
    d = len(rd)
    mu = [[float(u) for u in row] for row in mu]
    rd = [float(u) for u in rd]
    tc = [float(u) for u in tc]
    out = []
    x = [0.0] * d
    count = [0]

    def visit(k, pd):
        c = tc[k]
        for j in range(k + 1, d):
            if x[j]:
                c -= x[j] * mu[j][k]
        base = float(np.floor(c))
        for step, v0 in ((-1.0, base), (1.0, base + 1.0)):
            v = v0
            while True:
                nd = pd + (v - c) * (v - c) * rd[k]
                if not nd <= R:
                    break
                count[0] += 1
                assert count[0] <= max_nodes, "the tree is larger than this restatement is meant for"
                x[k] = v
                if k == 0:
                    out.append((nd, tuple(x)))
                else:
                    visit(k - 1, nd)
                v += step
        x[k] = 0.0

    visit(d - 1, 0.0)
    return sorted(out)
