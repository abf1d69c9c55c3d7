"""The exact reference of the solver tests (tests/exact_lattice.py) checked against independent counts, the families
of tests/solver_families.py against their size condition, and the CPU restatements of the solvers — the kernel's model
tests/svp_model.py, cvp_solver_cases.enumerate_cvp — against the exact reference on every family member.  The last
section changes the model in three ways a bit-for-bit comparison with the kernel cannot see and asks that the families
notice each.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import cvp_solver_cases as S
import exact_enum as E
import exact_lattice as X
import list_helpers as H
import solver_families as F
import svp_model as M

ALL = F.names()
CVP_MEMBERS = F.names("scaled_root", "knapsack", "wide")


# ---- 1. the reference against independent counts ---------------------------------------------------------------------
@pytest.mark.parametrize("d,n,seed", [(2, 2, 0), (3, 5, 1), (4, 4, 2), (5, 7, 3), (6, 6, 4), (6, 9, 5)])
def test_minimum_against_brute_force(d, n, seed):
    rng = np.random.default_rng(seed)
    b = H.lll_exact(rng.integers(-40, 41, size=(d, n)).tolist())
    m, xs, _ = X.lambda1_exact(b)
    assert m == M.brute_force_min(b)
    assert xs and all(sum(v * v for v in X.vector_of(b, x)) == m for x in xs)
    lst, _ = X.short_exact(b, m)
    assert [x for _, x in lst] == sorted(xs) and X.short_exact(b, m - 1)[0] == []


@pytest.mark.parametrize("d,R", [(1, 9), (3, 5), (5, 4), (8, 3)])
def test_ball_count_on_zd(d, R):
    """Z^d in the identity basis and (d = 8) in the unimodular basis of the list tests: half of the non-zero points of
    the ball, every one of them once."""
    for b in ([[int(i == j) for j in range(d)] for i in range(d)],) + ((H.z8_basis(),) if d == 8 else ()):
        lst, _ = X.short_exact(b, R)
        assert 2 * len(lst) + 1 == E.ball_count(d, R)
        assert len({x for _, x in lst}) == len(lst)
        t = [3] * d
        assert len(X.near_exact(b, t, R)[0]) == E.ball_count(d, R)  # a lattice point as the target: the whole ball


def _theta(b, N):
    out = {}
    for nv, _ in X.short_exact(b, N)[0]:
        out[nv] = out.get(nv, 0) + 2
    return out


def test_theta_series_of_the_root_lattices():
    """The numbers tests/test_list_vectors_gpu.py states: Z^8 to norm 4, the kissing numbers of D4 and E8; and the
    next shells of D4 (24 again at norm 4) and E8 (2160 at twice the minimum)."""
    assert _theta(H.z8_basis(), 4) == {1: 16, 2: 112, 3: 448, 4: 1136}
    assert _theta(H.d4_basis(), 4) == {2: 24, 4: 24}
    B, scale = H.e8_basis()
    assert _theta(B, 4 * scale) == {2 * scale: 240, 4 * scale: 2160}
    assert X.lambda1_exact(B)[0] == 2 * scale and len(X.lambda1_exact(B)[1]) == 120


def test_rows_and_level_bounds():
    """rows=k is the lattice of the first k rows; level bounds cut the tree and keep only vectors all of whose partial
    distances pass."""
    b = F.basis("knap_d12_b40")
    assert X.short_exact(b, 400, rows=7) == X.short_exact(b[:7], 400)
    full, nf = X.short_exact(b, 400)
    lev = [Fraction(float(v)) for v in E.step_pruning(12)]
    cut, nc = X.short_exact(b, 400, level=lev)
    assert 0 < len(cut) < len(full) and nc < nf and set(cut) <= set(full)
    for nv, x in full:
        pd = X.partial_distances(b, x)
        assert pd[0] == nv
        assert ((nv, x) in cut) == all(pd[k] <= lev[k] * 400 for k in range(12))


def test_closest_point_of_a_halfway_target_has_a_twin():
    b = F.basis("root_d4_s10_x1_0")
    kinds = dict(F.targets("root_d4_s10_x1_0"))
    assert "half" in kinds
    dist, xs, _ = X.closest_exact(b, kinds["half"])
    assert len(xs) >= 2 and len(xs) % 2 == 0 and dist > 0
    lat = X.vector_of(b, (3, -1, 4, 1))
    assert X.closest_exact(b, lat)[:2] == (0, [(3, -1, 4, 1)])


# ---- 2. the families --------------------------------------------------------------------------------------------------
def test_the_families_are_what_the_tests_say():
    fams = {}
    for name in ALL:
        fams.setdefault(F.family(name), []).append(name)
    assert sorted(fams) == ["cut_rows", "knapsack", "lane_edge", "scaled_root", "wide"]
    assert {F.info(k)["log_s"] for k in fams["scaled_root"]} == set(F.SCALES)
    assert {len(F.basis(k)[0]) - len(F.basis(k)) for k in fams["scaled_root"]} == {0, 1, 2, 3}
    assert sorted(len(F.basis(k)[0]) for k in fams["wide"]) == [64, 65, 130, 200, 256]
    assert sorted(len(F.basis(k)) for k in fams["knapsack"]) == [12, 12, 16, 16, 20, 20]
    # entries large enough for row norms near 2^61, where (double)(N - 1) is inexact
    big = [k for k in ALL if F.exact(k)["N0"] > 2**60]
    assert len(big) >= 3 and any(int(float(F.exact(k)["N0"] - 1)) != F.exact(k)["N0"] - 1 for k in big)
    assert F.exact("cut_scaled")["d_eff"] == 4 and F.exact("cut_kept")["d_eff"] == 5 and F.exact("cut_cut")["d_eff"] == 4
    assert F.exact("cut_expo_skew")["d_eff"] == 3 and F.exact("cut_expo_skew")["i0"] == 2
    _, r = H.gso_exact(F.basis("cut_kept"))
    assert r[4] == 2 * r[0]
    _, r = H.gso_exact(F.basis("cut_cut"))
    assert r[4] == 2 * r[0] + 1


@pytest.mark.parametrize("name", ALL)
def test_size_condition_and_reduction(name):
    """At most NODE_CAP nodes at N = (the shortest row's norm) - 1, in the exact tree; the member is LLL-reduced
    (delta 3/4, |mu| <= 1/2) in exact arithmetic, so it is within the solvers' contract."""
    ex = F.exact(name)
    print("%s: %d nodes at N0 - 1, lambda_1 = %d (%d minimal pairs), d_eff = %d" % (
        name, ex["cap_nodes"], ex["lam1"], len(ex["minimal"]) // 2, ex["d_eff"]))
    assert ex["cap_nodes"] <= F.NODE_CAP
    b = F.basis(name)
    mu, r = H.gso_exact(b)
    if F.family(name) != "lane_edge":  # (the steep bases are reduced as they stand but for the planted row d - 2)
        for k in range(1, len(b)):
            assert all(abs(mu[k][j]) <= Fraction(1, 2) for j in range(k))
            assert r[k] >= (Fraction(3, 4) - mu[k][k - 1] ** 2) * r[k - 1]


@pytest.mark.parametrize("name", F.names("cut_rows"))
def test_rows_beyond_d_eff_hold_nothing_shorter(name):
    """SVPM_FAST looks only below last_useful_index: the answer the solver tests ask for is lambda_1 of the first d_eff
    rows.  That IS lambda_1 of the lattice (a vector whose last non-zero coefficient is at row i >= d_eff has norm
    >= r_ii > 2 r_00): checked here on the whole basis, so that the tests ask for the true minimum."""
    ex = F.exact(name)
    true_l1, xs, _ = X.lambda1_exact(F.basis(name))
    assert true_l1 == ex["lam1"]
    assert {tuple(x) for x in xs} | {tuple(-v for v in x) for x in xs} == ex["minimal"]


@pytest.mark.parametrize("name", [k for k in F.names("scaled_root") if F.info(k)["extra"]])
def test_scaled_root_minimum_by_its_own_argument(name):
    """The minimum over the root lattice's minimal vectors, in Python integers, equals the enumeration's; most members
    hold two candidates whose norms differ by at most 4 at a magnitude of s^2."""
    i = F.info(name)
    norms = F.scaled_root_minimum(i["which"], i["log_s"], F.basis(name))
    assert len(norms) == (12 if i["which"] == "d4" else 120)
    assert norms[0] == F.exact(name)["lam1"]


def test_near_ties_exist_at_the_largest_scale():
    gaps = []
    for name in F.names("scaled_root"):
        i = F.info(name)
        if i["extra"] and i["log_s"] >= 27:
            norms = F.scaled_root_minimum(i["which"], i["log_s"], F.basis(name))
            gaps.append(min(b - a for a, b in zip(norms, norms[1:])))
    assert len(gaps) >= 4 and min(gaps) == 0 and max(gaps) <= 4


# ---- 3. the model against the exact reference ------------------------------------------------------------------------
def gso_with_row_exponents(b):
    """The stored mu, r and row exponents of a GSO that keeps one exponent per row (e_i = the bit length of the row's
    largest entry): stored mu(i,j) = mu 2^(e_j - e_i), stored r_ii = r 2^(-2 e_i); exact scalings of svp_model.gso_of."""
    mu, r, _ = M.gso_of(b)
    e = [max(abs(int(v)) for v in row).bit_length() for row in b]
    d = len(b)
    mus = [[math.ldexp(mu[i][j], e[j] - e[i]) for j in range(d)] for i in range(d)]
    return mus, [math.ldexp(r[i], -2 * e[i]) for i in range(d)], e


def gso_of(name, expo=False):
    """svp_model.gso_of of a member (or gso_with_row_exponents), once per process."""
    key = ("gso_of", name, expo)
    if key not in F._exact:
        F._exact[key] = gso_with_row_exponents(F.basis(name)) if expo else M.gso_of(F.basis(name))
    return F._exact[key]


def _model(name, pruning=None, expo=False):
    b = F.basis(name)
    mu, r, e = gso_of(name, expo)
    return M.solve(b, mu, r, e, pruning=pruning)


@pytest.mark.parametrize("name", ALL)
def test_model_returns_the_exact_minimum(name):
    o = _model(name)
    assert o["status"] == 1 and o["d_eff"] == F.exact(name)["d_eff"]
    F.check_shortest(name, o["sol_coord"], o["vec"], o["norm"])


@pytest.mark.parametrize("name", F.names("cut_rows", "knapsack") + ["root_e8_s29_x2_0", "wide_n65"])
def test_model_with_row_exponents_returns_the_exact_minimum(name):
    o = _model(name, expo=True)
    assert o["status"] == 1 and o["d_eff"] == F.exact(name)["d_eff"]
    F.check_shortest(name, o["sol_coord"], o["vec"], o["norm"])


@pytest.mark.parametrize("name", F.PRUNED)
def test_model_pruned_against_the_exact_pruned_tree(name):
    pr = F.pruning_of(name)
    o = _model(name, pruning=pr)
    assert o["status"] == 1
    F.check_pruned(name, pr, o["sol_coord"], o["norm"])


# ---- 3b. the reference's own runs on three members (tests/golden/svpsolve_fam_*.json) ---------------------------------
FAM = ["knap_d20_b40", "cut_scaled", "root_e8_s29_x2_0"]


@pytest.mark.parametrize("name", FAM)
def test_reference_runs_agree_with_the_exact_reference(name):
    """shortest_vector of the reference on the member's basis as it stands (make_svp_solver_fixtures.sh): SVPM_PROVED
    returns the exact minimum and one of the exact minimal vectors.  SVPM_FAST decides in floating point: on the
    knapsack and the cut_rows member it returns the minimum too; on the scaled root lattice, whose 120 shortest
    candidates differ by a few units in 2^61, it returns a lattice vector that is 10 longer than the minimum — the
    device solver, which decides on integers, is asked for the minimum there (test_solvers_exact_gpu.py)."""
    import json
    import os
    fx = json.load(open(os.path.join(S.GOLDEN, "svpsolve_fam_%s.json" % name)))
    b, ex = F.basis(name), F.exact(name)
    assert fx["basis"] == b and fx["d"] == len(b) and fx["n"] == len(b[0])
    for m in ("fast", "proved"):
        assert fx[m]["status"] == 0 and fx[m]["ref_ms"] > 0
        sol = [int(v) for v in fx[m]["sol_coord"]]
        assert sum(v * v for v in X.vector_of(b, sol)) == fx[m]["norm"]
    assert fx["proved"]["norm"] == ex["lam1"] and tuple(int(v) for v in fx["proved"]["sol_coord"]) in ex["minimal"]
    if name == "root_e8_s29_x2_0":
        assert fx["fast"]["norm"] == ex["lam1"] + 10
    else:
        assert fx["fast"]["norm"] == ex["lam1"] and tuple(int(v) for v in fx["fast"]["sol_coord"]) in ex["minimal"]


# ---- 4. closest vectors: the double restatement against the exact reference ------------------------------------------
def closest_exact_of(name, k):
    """closest_exact of target k of a member, once per process."""
    key = ("closest", name, k)
    if key not in F._exact:
        F._exact[key] = X.closest_exact(F.basis(name), F.targets(name)[k][1], max_nodes=F.NODE_CAP)
    return F._exact[key]


@pytest.mark.parametrize("name", CVP_MEMBERS)
def test_enumerate_cvp_agrees_with_closest_exact(name):
    """The targets of the GPU tests: prepare (the Babai loop) brings the target next to the origin, enumerate_cvp lists
    the points within the exact minimal distance (widened by 2^-20), and those whose integer distance is the minimum
    are exactly closest_exact's points."""
    b = np.array(F.basis(name), dtype=object)
    mu, rd = S.true_values(*S.gso_double(b), None)
    tg = F.targets(name)
    assert [k for k, _ in tg][:2] == ["near", "near"]
    P = S.prepare(b, mu, rd, np.array([t for _, t in tg], dtype=object))
    for k, (kind, t) in enumerate(tg):
        dist, xs, nodes = closest_exact_of(name, k)
        assert P["status"][k] == 1
        inside = float(dist - X.target_perp(F.basis(name), t))
        found = S.enumerate_cvp(mu, rd, P["target_coord"][k], inside * (1.0 + 2.0**-20) + 2.0**-20 * float(rd.min()))
        got = set()
        for _, x in found:
            full = tuple(int(v) + int(c) for v, c in zip(x, P["coef"][k]))
            if sum(v * v for v in X.vector_of(F.basis(name), full, t)) == dist:
                got.add(full)
        assert got == set(xs), (name, kind)
        if kind == "half":
            assert len(xs) >= 2


# ---- 5. mutations of the model that the kernel's bit-for-bit tests cannot see ----------------------------------------
def _mutant_radius(monkeypatch):
    """radius N instead of N - 1, and `<=` taken as an improvement: the model's text with those two places changed,
    compiled as a module of its own (svp_model itself stays as it is)."""
    import inspect
    import types
    src = inspect.getsource(M)
    for old, new in (("float(norm - 1) * MARGIN", "float(norm) * MARGIN"), ("if 0 < nv < nbest:", "if 0 < nv <= nbest:")):
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    mod = types.ModuleType("svp_model_radius_mutant")
    exec(compile(src, "svp_model_radius_mutant", "exec"), mod.__dict__)
    return mod.solve


def _mutant_stored_r(monkeypatch):
    """last_useful_index on the stored r instead of the true r."""
    real = M.last_useful_index
    monkeypatch.setattr(M, "last_useful_index", lambda rdiag, rexp, row_expo=True: real(rdiag, [0] * len(rdiag), row_expo))
    return M.solve


def _mutant_pruning_end(monkeypatch):
    """pruning indexed from the other end."""
    real = M.solve
    return lambda b, mu, rdiag, rexp, pruning=None, row_expo=True: real(
        b, mu, rdiag, rexp, None if pruning is None else list(pruning)[::-1], row_expo)


def _failures(solve):
    """The family members on which `solve` misses a check against the exact reference."""
    bad = []
    for name in ALL:
        b = F.basis(name)
        for expo in (False, True):
            if expo and name not in F.names("cut_rows"):
                continue
            mu, r, e = gso_of(name, expo)
            try:
                o = solve(b, mu, r, e)
                assert o["status"] == 1 and o["d_eff"] == F.exact(name)["d_eff"]
                F.check_shortest(name, o["sol_coord"], o["vec"], o["norm"])
            except AssertionError:
                bad.append((name, "expo" if expo else "plain"))
    for name in F.PRUNED:
        b = F.basis(name)
        mu, r, e = gso_of(name)
        pr = F.pruning_of(name)
        try:
            o = solve(b, mu, r, e, pruning=pr)
            F.check_pruned(name, pr, o["sol_coord"], o["norm"])
        except AssertionError:
            bad.append((name, "pruned"))
    return bad


@pytest.mark.parametrize("mutant", [None, _mutant_radius, _mutant_stored_r, _mutant_pruning_end],
                         ids=["unchanged", "radius_N_and_ties", "stored_r", "pruning_reversed"])
def test_the_families_notice_a_changed_model(mutant, monkeypatch):
    bad = _failures(M.solve if mutant is None else mutant(monkeypatch))
    print("%s: fails on %s" % (mutant.__name__ if mutant else "unchanged", bad))
    assert (bad == []) if mutant is None else (len(bad) >= 1)
