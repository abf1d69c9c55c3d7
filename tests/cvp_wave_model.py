"""The closest-vector wave kernel (fplll_amd/csrc/cvp_wave.hip) and the host's completion of its outputs (the WAVE
route of fphip_closest_vector_ex) restated in Python: the same double operations in the same order (Python floats are
IEEE doubles, every multiply and add separate), Python integers for the exact distances, the same node counting.  The
GPU tests ask the WAVE route for this module's sol_coord, norm, nodes, dist and status bit for bit, fed with the
device's own true mu / r_ii and the device's own preparation.

  walk(mu, rd, tc, radius, on_leaf, max_nodes=0)
      the walk proper.  mu [d][d] (strictly lower: mu[i][j] = mu(i,j), j < i) and rd [d]: the TRUE values; tc [d]: the
      root's centre row (target_coord); radius: every level's bound.  on_leaf(x, nd, radius) is called for every leaf
      within the bound (x: d floats, nd: its walk distance, radius: the bound as it stands) and returns None (go on),
      a float (the new radius) or STOP.  max_nodes > 0: the budget, tested at the top of every pass of the STEP loop.
      -> dict(status 1 | 2 (the budget ended the walk), nodes, plain (accepted nodes per level))
  solve(b, mu, rd, targets-or-prepared, max_nodes=0)
      the kernel's evaluator on exact integers and what the host does around it, built on cvp_solver_cases.prepare
      (a dict is taken as the outputs of a preparation — the device's, in the GPU tests).
      -> dict(sol_coord [T][d] ints, dist [T], norm [T] ints, nodes [T], status [T], found [T])

The keyword switches half_tree, strict and ties_even are three deliberate mistakes (the shortest-vector walk's
half-tree step at partial distance 0, `<` for `<=` at the bound, ties rounded to even): tests/test_cvp_wave_cpu.py
shows that its cases notice each of them.
"""
import math

import numpy as np

import cvp_solver_cases as S
from svp_model import INT64_MAX, fits64, round_away

MARGIN = 2.0**-30  # the heuristic margin of the solvers: not a proved bound
NODE_LIMIT = 2
STOP = "stop"


def _round_even(c):
    f = math.floor(c)
    r = c - f
    if r > 0.5 or (r == 0.5 and f % 2.0 != 0.0):
        f += 1.0
    return f


def walk(mu, rd, tc, radius, on_leaf, max_nodes=0, half_tree=False, strict=False, ties_even=False):
    d = len(rd)
    mu = [[float(v) for v in row] for row in mu]
    rd = [float(v) for v in rd]
    rnd = _round_even if ties_even else round_away
    within = (lambda v, bound: v < bound) if strict else (lambda v, bound: v <= bound)
    xs, cs, pds = [0.0] * d, [0.0] * d, [0.0] * d
    dxs, ddxs, plain = [0] * d, [0] * d, [0] * d
    S_ = [float(v) for v in tc]
    stk = {}
    k, nd, done, nodes, status = d, 0.0, False, 0, 1

    def leaf():
        nonlocal radius, done
        r = on_leaf(list(xs), nd, radius)
        if r is STOP:
            done = True
        elif r is not None:
            radius = r

    while not done:
        # CHILD chain
        while True:
            kc = k - 1
            c1 = S_[kc]
            x1 = rnd(c1)
            a1 = x1 - c1
            n1 = nd + a1 * a1 * rd[kc]
            if not within(n1, radius):
                done = k >= d
                break
            stk[k] = S_[:k]
            s1 = 1 if c1 >= x1 else -1
            cs[kc], xs[kc], pds[kc], dxs[kc], ddxs[kc] = c1, x1, nd, s1, s1
            plain[kc] += 1
            nodes += 1
            k, nd = kc, n1
            if k == 0:
                leaf()
                break
            for j in range(k):
                S_[j] = S_[j] - x1 * mu[k][j]
        if done:
            break
        # STEP loop
        while True:
            if max_nodes and nodes >= max_nodes:
                status, done = NODE_LIMIT, True
                break
            par = stk[k + 1]
            xk, ck, pdk, dxk, ddxk = xs[k], cs[k], pds[k], dxs[k], ddxs[k]
            if half_tree and pdk == 0.0:
                xk += 1.0
            else:
                xk += float(dxk)
                ddxk = -ddxk
                dxk = ddxk - dxk
            xs[k], dxs[k], ddxs[k] = xk, dxk, ddxk
            a = xk - ck
            nd = pdk + a * a * rd[k]
            if not within(nd, radius):
                k += 1
                if k >= d:
                    done = True
                    break
                continue
            plain[k] += 1
            nodes += 1
            if k == 0:
                leaf()
                if done:
                    break
                continue
            for j in range(k):
                S_[j] = par[j] - xk * mu[k][j]
            break
    return dict(status=status, nodes=nodes, plain=plain)


def _sub_rows(v, coefs, b):
    """v - sum coefs_i b_i in the kernel's order (rows ascending, a zero coefficient skipped); None: a product or a
    difference beyond 63 bits."""
    v = list(v)
    for i, c in enumerate(coefs):
        if c == 0:
            continue
        for j in range(len(v)):
            p = c * b[i][j]
            s = v[j] - p
            if not fits64(p) or not fits64(s):
                return None
            v[j] = s
    return v


def solve(b, mu, rd, targets, max_nodes=0, **mistakes):
    b = [[int(v) for v in row] for row in np.asarray(b).astype(object)]
    d, n = len(b), len(b[0])
    P = targets if isinstance(targets, dict) else dict(S.prepare(b, mu, rd, targets), targets=targets)
    tg = [[int(v) for v in row] for row in np.asarray(P["targets"]).astype(object)]
    T = len(tg)
    mu = np.asarray(mu, dtype=np.float64)
    rd = np.asarray(rd, dtype=np.float64)
    out = dict(sol_coord=[[0] * d for _ in range(T)], dist=[0.0] * T, norm=[0] * T, nodes=[0] * T,
               status=[int(v) for v in P["status"]], found=[0] * T)
    rd_ok = all(0.0 < float(v) < math.inf for v in rd)
    for t in range(T):
        if out["status"][t] != 1:
            continue
        coef = [int(v) for v in P["coef"][t]]
        tc = [float(v) for v in P["target_coord"][t]]
        desc = float(P["descent"][t])
        best = None  # (N, x, nd)
        if d >= 2 and 0.0 < desc < math.inf and rd_ok:
            tr = _sub_rows(tg[t], coef, b)
            if tr is None:
                out["status"][t] = -2
                continue
            state = dict(ovf=False)

            def on_leaf(x, nd, radius):
                nonlocal best
                v = None
                if all(abs(u) < 9223372036854775808.0 for u in x):
                    v = _sub_rows(tr, [int(u) for u in x], b)
                N = None if v is None else sum(u * u for u in v)
                if N is None or N > INT64_MAX:
                    state["ovf"] = True
                    return STOP
                if best is None or N < best[0]:
                    best = (N, [int(u) for u in x], nd)
                    if N == 0:
                        return STOP
                    return min(nd + nd * MARGIN, radius)
                return None

            w = walk(mu, rd, tc, desc + desc * MARGIN, on_leaf, max_nodes, **mistakes)
            if state["ovf"]:
                out["status"][t] = -2
                continue
            out["status"][t] = w["status"]
            out["nodes"][t] = w["nodes"]
        if best is not None:
            N, x, nd = best
            out["found"][t] = 1
        else:  # the host's fill: the rounding descent (the preparation's loop), its exact distance
            xd, _ = S.descent_of(mu, rd, np.array([tc]))
            if not all(abs(float(v)) < 9223372036854775808.0 for v in xd[0]):
                out["status"][t] = -2
                out["nodes"][t] = 0
                continue
            x, nd, N = [int(v) for v in xd[0]], desc, None
        sol = [c + v for c, v in zip(coef, x)]
        if not all(fits64(v) for v in sol):
            out["status"][t] = -2
            out["nodes"][t] = 0
            continue
        if N is None:
            N = sum((tg[t][j] - sum(sol[i] * b[i][j] for i in range(d))) ** 2 for j in range(n))
            N = N if N <= INT64_MAX else 0
        out["sol_coord"][t], out["dist"][t], out["norm"][t] = sol, nd, N
    return out
