"""The N-shortest-vectors kernel for quadratic forms (fplll_amd/csrc/svp_gram.hip) restated in Python: the same double
operations in the same order (every multiply and add separate), the same integer steps for the norms, the same node
counting, the same table.  The walk and the table are svp_best_model.py's (the kernel copies svp_best.hip's loops);
what differs is the input — a Gram matrix, mu and r_ii as fphip_gram_update leaves them, no row exponents, no basis —
and the evaluator:

  * the "row norms" are the diagonal g_ii (a diagonal entry <= 0: status 0);
  * the rows are cut on r_ii directly; an r_ii among the rows walked that is <= 0 or not finite: status 0;
  * a candidate's norm is N = x G x^T by the kernel's steps (form_norm below): every |x_i| below 2^57, y_j = sum_i x_i
    g_ij (below 2^126 in absolute value: exact in 128 bits), y_j = yh_j 2^64 + yl_j, N = 2^64 sum_j x_j yh_j + sum_j x_j
    yl_j (both sums exact in 128 bits).  Status -2: N beyond 63 bits, or a coefficient of 2^57 and more.  A negative N
    is not accepted.

  solve(G, mu, rdiag, max_sols, bound_sq=None, pruning=None)
      -> dict(status, found, sol_coord [K][d], norm [K], nodes, d_eff, insertions, B0)
"""
from svp_model import INT64_MAX, MARGIN, fexponent, ldexp, round_away

COEF_LIMIT = 2.0**57
I128_MAX = 2**127 - 1


def _fmax(a, b):
    """fmax(): the other argument where one is a NaN."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def form_norm(G, x, bs):
    """(ok, N) of the kernel's evaluator on the first bs variables: ok False = status -2.  The 128-bit steps are
    asserted to stay in range — the bound the kernel relies on."""
    if any(not abs(float(v)) < COEF_LIMIT for v in x[:bs]):
        return False, 0
    xl = [int(v) for v in x[:bs]]
    Hs = Ls = 0
    for j in range(bs):
        y = 0
        for i in range(bs):
            if xl[i] == 0:
                continue
            y += xl[i] * G[i][j]
            assert abs(y) <= I128_MAX
        yh, yl = y >> 64, y & (2**64 - 1)  # floor division: yh signed, yl unsigned
        assert abs(xl[j] * yh) <= I128_MAX and abs(xl[j] * yl) <= I128_MAX
        Hs += xl[j] * yh
        Ls += xl[j] * yl
        assert abs(Hs) <= I128_MAX and abs(Ls) <= I128_MAX
    T = Hs + (Ls >> 64)
    low = Ls & (2**64 - 1)
    assert T * 2**64 + low == sum(xl[i] * G[i][j] * xl[j] for i in range(bs) for j in range(bs))
    if T < 0:
        return True, -1  # (a negative norm: any negative value, the table refuses it)
    if T != 0 or low > INT64_MAX:
        return False, 0
    return True, low


def rows_kept(rdiag, radius0=None):
    """The kernel's row cut on r_ii: without a bound r_ii <= 2 r_00; with one the threshold max(2 r_00, radius0)."""
    r00x2 = rdiag[0] * 2.0
    thr = r00x2 if radius0 is None else _fmax(r00x2, radius0)
    d_eff = 1
    for i in range(1, len(rdiag)):
        if rdiag[i] <= thr:
            d_eff = i + 1
    return d_eff


def solve(G, mu, rdiag, max_sols, bound_sq=None, pruning=None, update_status=1):
    G = [[int(v) for v in row] for row in G]
    d, K = len(G), int(max_sols)
    assert 1 <= K <= 64 and 1 <= d <= 64 and all(len(row) == d for row in G)
    out = dict(status=1, found=0, sol_coord=[[0] * d for _ in range(K)], norm=[0] * K, nodes=0, d_eff=0, insertions=0,
               B0=0)
    # 1. the diagonal
    rn = [G[i][i] for i in range(d)]
    if update_status != 1 or any(v <= 0 for v in rn):
        out["status"] = 0
        return out
    # 2. the bound, 3. the rows cut
    rdiag = [float(v) for v in rdiag]
    bnd = int(bound_sq) if bound_sq else 0
    if bnd > 0:
        B0 = bnd
        d_eff = rows_kept(rdiag, float(B0) * MARGIN)
    else:
        d_eff = rows_kept(rdiag)
        B0 = min(rn[:d_eff])
    out.update(d_eff=d_eff, B0=B0)
    bs = d_eff
    if any(not (rdiag[i] > 0.0 and rdiag[i] <= 1.79769313486231570815e+308) for i in range(bs)):
        out["status"] = 0
        return out
    radius0 = float(B0) * MARGIN
    tn, recs = [], []  # the table: norms sorted, the coefficient records in the same order
    if radius0 > 0.0:
        ne = max(max(fexponent(rdiag[i]) for i in range(bs)), -1)
        rd = [ldexp(rdiag[i], -ne) for i in range(bs)]
        prn = [float(pruning[i]) if pruning is not None else 1.0 for i in range(bs)]
        maxdist = ldexp(radius0, -ne)
        pb = [p * maxdist for p in prn]
        mu_blk = [[float(mu[k][j]) for j in range(k)] for k in range(bs)]
        xs, cs, pds = [0.0] * bs, [0.0] * bs, [0.0] * bs
        dxs, ddxs, cnt = [0] * bs, [0] * bs, [0] * bs
        S = [0.0] * bs
        stk = {}
        k, nd, done = bs, 0.0, False
        state = dict(status=1, done=False)

        def candidate():
            nonlocal maxdist, pb
            ok, nv = form_norm(G, xs, bs)
            if not ok:
                state["status"] = -2
                state["done"] = True
                return
            full = len(tn) == K
            if nv > 0 and nv <= B0 and (not full or nv < tn[K - 1]):
                p = sum(1 for t in tn if t <= nv)  # behind every kept entry with norm <= nv
                tn.insert(p, nv)
                recs.insert(p, [int(x) for x in xs] + [0] * (d - bs))
                if len(tn) > K:
                    tn.pop()
                    recs.pop()
                out["insertions"] += 1
                if len(tn) == K:
                    worst = tn[K - 1]
                    if worst == 1:
                        state["done"] = True
                        return
                    maxdist = ldexp(float(worst - 1) * MARGIN, -ne)
                    pb = [p * maxdist for p in prn]

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
            out["insertions"] = 0
            return out
        out["nodes"] = sum(cnt) - (bs - 1)
    out["found"] = len(tn)
    for j, (nv, x) in enumerate(zip(tn, recs)):
        out["sol_coord"][j], out["norm"][j] = x, nv
    return out


def gso_of_form(G):
    """mu [d][d], rdiag [d] of a positive definite integer form from exact rationals (exact_form.ldl_exact), rounded
    once: for the CPU tests."""
    import exact_form as XF
    mu, r = XF.ldl_exact(G)
    d = len(G)
    return [[float(mu[i][j]) if j < i else 0.0 for j in range(d)] for i in range(d)], [float(v) for v in r]

