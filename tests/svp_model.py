"""The shortest-vector kernel (fplll_amd/csrc/svp_wave.hip) restated in Python: the same double operations in the same
order (Python floats are IEEE doubles, every multiply and add separate), Python integers for the norms, the same node
counting.  The model of the kernel as gram_lll_model.py is the model of the Gram LLL: the GPU tests ask the WAVE route
for this module's sol_coord, norm and nodes bit for bit, fed with the device's own mu / r / row exponents.

  solve(b, mu, rdiag, rexp, pruning=None, row_expo=True)
      b      [d][n] integers; mu [d][d], rdiag [d], rexp [d]: the STORED values of the device GSO (true mu(i,j) =
             mu[i][j] 2^(rexp[i] - rexp[j]), true r_ii = rdiag[i] 2^(2 rexp[i]))
      ->     dict(status, sol_coord, vec, norm, nodes, d_eff, i0, improvements)
  gso_of(b)  mu, rdiag, rexp (all zero) of an integer basis from exact rationals, rounded once: for the CPU tests
"""
import math
from fractions import Fraction

INT64_MAX = 2**63 - 1
INT_MIN = -(2**31)
MARGIN = 1.0 + 2.0**-30  # the heuristic margin of the solvers: not a proved bound


def ldexp(x, e):
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.copysign(math.inf, x)


def fexponent(x):
    """FP_NR<double>::exponent(): ilogb(x) + 1, and INT_MIN + 1 for zero (gso_wave.h)."""
    return INT_MIN + 1 if x == 0.0 else math.frexp(x)[1]


def round_away(c):
    """round(): ties away from zero."""
    a = abs(c)
    f = math.floor(a)
    if a - f >= 0.5:  # (exact: a and f are doubles less than one apart, or a is an integer)
        f += 1.0
    return math.copysign(f, c) if f != 0.0 else 0.0


def fits64(v):
    return -(2**63) <= v <= INT64_MAX


def radius_of(norm):
    return float(norm - 1) * MARGIN


def gso_of(b):
    d = len(b)
    bs, mu, r = [], [[0.0] * d for _ in range(d)], [0.0] * d
    for i in range(d):
        v = [Fraction(int(x)) for x in b[i]]
        for j in range(i):
            m = sum(Fraction(int(x)) * y for x, y in zip(b[i], bs[j])) / sum(y * y for y in bs[j])
            mu[i][j] = float(m)
            v = [x - m * y for x, y in zip(v, bs[j])]
        bs.append(v)
        r[i] = float(sum(y * y for y in v))
    return mu, r, [0] * d


def last_useful_index(rdiag, rexp, row_expo=True):
    """svpcvp.cpp:32-43 on the true r_ii, in the kernel's arithmetic: r_ii 2^(2 (e_i - e_0)) <= 2 r_00."""
    d = len(rdiag)
    e = [int(v) if row_expo else 0 for v in rexp]
    r00x2 = rdiag[0] * 2.0
    d_eff = 1
    for i in range(1, d):
        de = max(min(2 * (e[i] - e[0]), 4000), -4000)
        if ldexp(rdiag[i], de) <= r00x2:
            d_eff = i + 1
    return d_eff


def solve(b, mu, rdiag, rexp, pruning=None, row_expo=True):
    b = [[int(v) for v in row] for row in b]
    d, n = len(b), len(b[0])
    out = dict(status=1, sol_coord=[0] * d, vec=[0] * n, norm=0, nodes=0, d_eff=0, i0=0, improvements=0)
    # 1. exact row norms (non-negative addends: one of the kernel's partial sums overflows exactly when the total does)
    rn = [sum(v * v for v in row) for row in b]
    if any(v > INT64_MAX for v in rn):
        out["status"] = -2
        return out
    # 2. last_useful_index, 3. get_basis_min
    e = [int(v) if row_expo else 0 for v in rexp]
    rdiag = [float(v) for v in rdiag]
    d_eff = last_useful_index(rdiag, e, True)
    i0 = 0
    for i in range(1, d_eff):
        if rn[i] < rn[i0]:
            i0 = i
    nbest = rn[i0]
    best_x = [1 if i == i0 else 0 for i in range(d)]
    best_v = list(b[i0])
    out.update(d_eff=d_eff, i0=i0)
    radius0 = radius_of(nbest)
    if d_eff >= 2 and radius0 > 0.0:
        bs = d_eff
        # 4. normalisation
        ne = max(max(min(2 * e[i] + fexponent(rdiag[i]), 2**31 - 1) for i in range(bs)), -1)
        rd = [ldexp(rdiag[i], 2 * e[i] - ne) for i in range(bs)]
        prn = [float(pruning[i]) if pruning is not None else 1.0 for i in range(bs)]
        maxdist = ldexp(radius0, -ne)
        pb = [p * maxdist for p in prn]
        mu_blk = [[ldexp(float(mu[k][j]), e[k] - e[j]) for j in range(k)] for k in range(bs)]
        xs, cs, pds = [0.0] * bs, [0.0] * bs, [0.0] * bs
        dxs, ddxs, cnt = [0] * bs, [0] * bs, [0] * bs
        S = [0.0] * bs
        stk = {}
        k, nd, done = bs, 0.0, False
        state = dict(status=1, done=False)

        def candidate():
            nonlocal nbest, best_x, best_v, maxdist, pb
            v = [0] * n
            ovf = False
            for i in range(bs):
                xi = xs[i]
                if xi == 0.0:
                    continue
                if not abs(xi) < 9223372036854775808.0:
                    ovf = True
                    break
                lx = int(xi)
                for j in range(n):
                    p = lx * b[i][j]
                    s = v[j] + p
                    ovf = ovf or not fits64(p) or not fits64(s)
                    v[j] = s
            nv = sum(x * x for x in v)
            if ovf or nv > INT64_MAX:
                state["status"] = -2
                state["done"] = True
                return
            if 0 < nv < nbest:
                nbest = nv
                best_x = [int(x) for x in xs] + [0] * (d - bs)
                best_v = v
                out["improvements"] += 1
                maxdist = ldexp(radius_of(nbest), -ne)
                pb = [p * maxdist for p in prn]
                if nbest == 1:
                    state["done"] = True

        while not done:
            # CHILD chain
            while True:
                kc = k - 1
                c1 = S[kc]
                x1 = round_away(c1)
                a1 = x1 - c1
                n1 = nd + a1 * a1 * rd[kc]
                if not n1 <= pb[kc]:
                    done = k >= bs
                    break
                stk[k] = S[:k]
                s1 = 1 if c1 >= x1 else -1
                cs[kc], xs[kc], pds[kc], dxs[kc], ddxs[kc] = c1, x1, nd, s1, s1
                cnt[kc] += 1
                k, nd = kc, n1
                if k == 0:
                    if nd > 0.0:
                        candidate()
                        done = state["done"]
                    break
                for j in range(k):
                    S[j] = S[j] - x1 * mu_blk[k][j]
            if done:
                break
            # STEP loop
            while True:
                par = stk[k + 1]
                xk, ck, pdk, dxk, ddxk = xs[k], cs[k], pds[k], dxs[k], ddxs[k]
                if pdk != 0.0:
                    xk += float(dxk)
                    ddxk = -ddxk
                    dxk = ddxk - dxk
                else:
                    xk += 1.0
                xs[k], dxs[k], ddxs[k] = xk, dxk, ddxk
                a = xk - ck
                nd = pdk + a * a * rd[k]
                if not nd <= pb[k]:
                    k += 1
                    if k >= bs:
                        done = True
                        break
                    continue
                cnt[k] += 1
                if k == 0:
                    if nd > 0.0:
                        candidate()
                        if state["done"]:
                            done = True
                            break
                    continue
                for j in range(k):
                    S[j] = par[j] - xk * mu_blk[k][j]
                break
        if state["status"] != 1:
            out["status"] = -2
            return out
        out["nodes"] = sum(cnt) - (bs - 1)
    out.update(sol_coord=best_x, vec=best_v, norm=nbest)
    return out


def brute_force_min(b, box=None):
    """The minimal non-zero squared norm of the lattice of b (d <= 8) over a coefficient box bounded from the exact
    Gram matrix: |x_i| <= sqrt(N (G^-1)_ii) for every vector of squared norm <= N, N = the shortest row's."""
    d = len(b)
    G = [[Fraction(sum(int(x) * int(y) for x, y in zip(b[i], b[j]))) for j in range(d)] for i in range(d)]
    # inverse by exact elimination
    A = [row[:] + [Fraction(int(i == j)) for j in range(d)] for i, row in enumerate(G)]
    for c in range(d):
        p = next(r for r in range(c, d) if A[r][c] != 0)
        A[c], A[p] = A[p], A[c]
        A[c] = [v / A[c][c] for v in A[c]]
        for r in range(d):
            if r != c and A[r][c] != 0:
                A[r] = [v - A[r][c] * w for v, w in zip(A[r], A[c])]
    N = min(int(G[i][i]) for i in range(d))
    lim = [math.isqrt(int(N * A[i][d + i])) + 1 for i in range(d)] if box is None else [box] * d
    import numpy as np
    shape = [2 * l + 1 for l in lim[:-1]] + [lim[-1] + 1]  # (one of each pair +-x: the last coefficient >= 0)
    total = int(np.prod(shape))
    assert total <= 4_000_000, "brute force over %d points: choose a smaller or better reduced basis" % total
    x = np.indices(shape, dtype=np.int64).reshape(d, total).T - np.array(lim[:-1] + [0], dtype=np.int64)
    nrm = ((x @ np.array(b, dtype=np.int64)) ** 2).sum(axis=1)  # (entries of the test bases are small: exact in int64)
    return int(nrm[nrm > 0].min())
