"""The N-shortest-vectors kernel (fplll_amd/csrc/svp_best.hip) restated in Python: the same double operations in the
same order (every multiply and add separate), Python integers for the norms, the same node counting, the same table.
The walk is svp_model.py's (the kernel copies svp_wave.hip's loops); what differs is the start — the radius
(double)B0 (1 + 2^-30), inclusive, nothing seeded —, the rows cut under a caller's bound, and the evaluator: a table of at
most K norms sorted, ties in discovery order, the radius (worst - 1) (1 + 2^-30) once it is full.  The GPU tests ask the
WAVE route for this module's found, sol_coord, vec, norm and nodes bit for bit, fed with the device's own mu / r / row
exponents.

  solve(b, mu, rdiag, rexp, max_sols, bound_sq=None, pruning=None, row_expo=True, mutate=None)
      -> dict(status, found, sol_coord [K][d], vec [K][n], norm [K], nodes, d_eff, insertions, B0)
  mutate: None, or one of three deliberate mistakes the CPU tests must catch:
      "radius_at_worst"    the radius of a full table at worst instead of worst - 1
      "reference_row_cut"  the reference's 2 r_00 row cut under a caller's bound
      "ties_in_front"      a candidate inserted in front of the kept entries of its norm
"""
import svp_model as M
from svp_model import INT64_MAX, MARGIN, fexponent, fits64, ldexp, round_away


def rows_kept(rdiag, rexp, row_expo, radius0=None):
    """The kernel's row cut on the true r_ii, in its arithmetic (everything relative to row 0's exponent): without a
    bound svp_model.last_useful_index; with one the threshold max(2 r_00, radius0 2^(-2 e_0))."""
    if radius0 is None:
        return M.last_useful_index(rdiag, rexp, row_expo)
    d = len(rdiag)
    e = [int(v) if row_expo else 0 for v in rexp]
    r00x2 = rdiag[0] * 2.0
    thr = max(r00x2, ldexp(radius0, max(min(-2 * e[0], 4000), -4000)))
    d_eff = 1
    for i in range(1, d):
        de = max(min(2 * (e[i] - e[0]), 4000), -4000)
        if ldexp(rdiag[i], de) <= thr:
            d_eff = i + 1
    return d_eff


def solve(b, mu, rdiag, rexp, max_sols, bound_sq=None, pruning=None, row_expo=True, mutate=None):
    assert mutate in (None, "radius_at_worst", "reference_row_cut", "ties_in_front")
    b = [[int(v) for v in row] for row in b]
    d, n, K = len(b), len(b[0]), int(max_sols)
    assert 1 <= K <= 64
    out = dict(status=1, found=0, sol_coord=[[0] * d for _ in range(K)], vec=[[0] * n for _ in range(K)], norm=[0] * K,
               nodes=0, d_eff=0, insertions=0, B0=0)
    # 1. exact row norms
    rn = [sum(v * v for v in row) for row in b]
    if any(v > INT64_MAX for v in rn):
        out["status"] = -2
        return out
    # 2. the bound, 3. the rows cut
    e = [int(v) if row_expo else 0 for v in rexp]
    rdiag = [float(v) for v in rdiag]
    bnd = int(bound_sq) if bound_sq else 0
    if bnd > 0:
        B0 = bnd
        d_eff = rows_kept(rdiag, e, True, None if mutate == "reference_row_cut" else float(B0) * MARGIN)
    else:
        d_eff = rows_kept(rdiag, e, True)
        B0 = min(rn[:d_eff])
    out.update(d_eff=d_eff, B0=B0)
    radius0 = float(B0) * MARGIN
    tn, recs = [], []  # the table: norms sorted, the records (coefficients, vector) in the same order
    if radius0 > 0.0:
        bs = d_eff
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
            nonlocal maxdist, pb
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
            full = len(tn) == K
            if nv > 0 and nv <= B0 and (not full or nv < tn[K - 1]):
                if mutate == "ties_in_front":
                    p = sum(1 for t in tn if t < nv)
                else:
                    p = sum(1 for t in tn if t <= nv)  # behind every kept entry with norm <= nv
                tn.insert(p, nv)
                recs.insert(p, ([int(x) for x in xs] + [0] * (d - bs), v))
                if len(tn) > K:
                    tn.pop()
                    recs.pop()
                out["insertions"] += 1
                if len(tn) == K:
                    worst = tn[K - 1]
                    if worst == 1:
                        state["done"] = True
                        return
                    maxdist = ldexp(float(worst if mutate == "radius_at_worst" else worst - 1) * MARGIN, -ne)
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
    for j, (nv, (x, v)) in enumerate(zip(tn, recs)):
        out["sol_coord"][j], out["vec"][j], out["norm"][j] = x, v, nv
    return out
