"""The three device solvers — shortest_vector (both routes and AUTO), short_vectors / theta_series / vectors_near,
closest_vector(s) — against an exact integer reference (tests/exact_lattice.py: rational Fincke-Pohst enumeration, no
float) on the families of tests/solver_families.py: scaled root lattices with near-tied minima at norms up to 2^61,
knapsack bases, wide bases of every columns-per-lane class, bases whose last rows last_useful_index cuts, d = 63, 64.
The WAVE route's other tests (test_svp_solver_gpu.py) compare it with a model that restates it; these ask what neither
can see of the other: that nothing shorter (closer, missing from the list) exists."""
from fractions import Fraction

import numpy as np
import pytest

import conftest as C
import cvp_solver_cases as S
import exact_lattice as X
import list_helpers as H
import solver_families as F

pytestmark = pytest.mark.gpu

ALL = F.names()
LIST_MEMBERS = F.names("scaled_root", "knapsack", "wide")
_state = {}


def _np(b):
    return np.array(b, dtype=np.int64)


def _solve(ctx, b, route, **kw):
    """One lattice through MatGSOBatch.shortest_vector: (sol, vec, norm, nodes, status, last_kernel_ms)."""
    from fplll_amd.gso import MatGSOBatch
    row_expo = kw.pop("row_expo", True)
    b = _np(b)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1], row_expo=row_expo)
    try:
        g.set_basis(b)
        sol, vec, norm, nodes, st = g.shortest_vector(route=route, **kw)
        ms = g.last_kernel_ms
    finally:
        g.close()
    return sol[0], vec[0], int(norm[0]), int(nodes[0]), int(st[0]), ms


# ---- shortest_vector --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_shortest_vector_is_the_exact_minimum(ctx, name):
    """Every member, WAVE, ENUM and AUTO: status 1, the exact minimum, sol_coord one of the exact minimal vectors (up
    to sign; the first minimal row where nothing is strictly shorter), vec = sol_coord b in Python integers.
    Catches: a radius that cuts the minimum, a norm decided in double, a tie taken as an improvement."""
    for route in ("wave", "enum", "auto"):
        sol, vec, norm, nodes, st, _ = _solve(ctx, F.basis(name), route)
        C.note(lambda: ("%s %s: norm %d, %d nodes" % (name, route, norm, nodes),))
        assert st == 1, (name, route, st)
        F.check_shortest(name, sol, vec, norm)


@pytest.mark.parametrize("route", ["wave", "enum"])
@pytest.mark.parametrize("name", F.PRUNED)
def test_pruned_calls_against_the_exact_pruned_tree(ctx, name, route):
    """step pruning from 1 (level 0) to 3/4 (the top level): the answer is a node of the exact pruned tree and the
    exact pruned tree below its norm is empty (solver_families.check_pruned).  knap_d12_b30 has d_eff = 11 < d.
    Catches: pruning indexed from the other end, bounds not rescaled on an improvement, on either route."""
    pr = F.pruning_of(name)
    sol, vec, norm, nodes, st, _ = _solve(ctx, F.basis(name), route, pruning=pr)
    assert st == 1
    F.check_pruned(name, pr, sol, norm)
    assert [int(v) for v in vec] == X.vector_of(F.basis(name), [int(v) for v in sol])


@pytest.mark.parametrize("row_expo", [True, False])
@pytest.mark.parametrize("name", F.names("cut_rows"))
def test_cut_rows_with_and_without_row_exponents(ctx, name, row_expo):
    """d_eff < d, the boundary r_ii = 2 r_00 (kept) / 2 r_00 + 1 (cut), rows with exponents far apart; on both routes.
    The answer asked is lambda_1 of the first d_eff rows, which test_solvers_exact_cpu.py shows to be the lattice's."""
    for route in ("enum", "wave"):
        sol, vec, norm, nodes, st, _ = _solve(ctx, F.basis(name), route, row_expo=row_expo)
        assert st == 1
        F.check_shortest(name, sol, vec, norm)
        assert not any(int(v) for v in sol[F.exact(name)["d_eff"]:])


def test_enum_route_on_a_second_context(ctx):
    import fplll_amd
    e2 = fplll_amd.Context(0)
    try:
        for name in ("knap_d20_b40", "root_e8_s29_full_0", "cut_scaled", "wide_n130"):
            sol, vec, norm, nodes, st, _ = _solve(ctx, F.basis(name), "enum", ectx=e2)
            assert st == 1
            F.check_shortest(name, sol, vec, norm)
    finally:
        e2.close()


@pytest.mark.parametrize("name", ["knap_d16_b40", "root_e8_s20_x3_0"])
def test_reduce_true_on_an_unreduced_copy(ctx, name):
    """The same lattice in a basis that needs reducing again: the same norm, and coefficients that are valid in the
    CALLER's basis."""
    from fplll_amd.gso import _unreduced_copy
    from fplll_amd.svp import shortest_vector
    b_in = _unreduced_copy(_np(F.basis(name)))
    assert not np.array_equal(b_in, _np(F.basis(name)))
    for route in ("auto", "enum"):
        sol, vec, norm = shortest_vector(ctx, b_in, reduce=True, route=route)
        assert norm == F.exact(name)["lam1"]
        v = X.vector_of(b_in.tolist(), [int(t) for t in sol])
        assert v == [int(t) for t in vec] and sum(t * t for t in v) == norm


# ---- the mixed AUTO batch ---------------------------------------------------------------------------------------------
# FPHIP_SVP_WAVE_MAX_NODES between the node estimates of the two groups.  Measured on the MI355X, one single-lattice
# AUTO call per limit (last_kernel_ms == 0: no WAVE launch), the limit bisected to 2 %:
#   easy (lattices 0, 3, 6, 8, 10):  the estimates lie in (13.5, 14.1]
#   hard (lattices 4, 7, 1, 9):      in (43.1, 43.7], (81.3, 82.4], (123.5, 125.2], (285.2, 289.0]
# (the same figures as the estimate's restatement tests/perf/svp_solver_bench.py::gh_nodes gives on the exact r_ii).
MIXED_LIMIT = "25"


def _mixed_exact():
    if "mixed" not in _state:
        bs, roles = F.mixed_batch()
        want = {}
        for k, role in enumerate(roles):
            if role in ("easy", "hard"):
                de = X.d_eff_exact(bs[k])
                m, xs, _ = X.lambda1_exact(bs[k], rows=de)
                pad = (0,) * (16 - de)
                want[k] = (m, {tuple(x) + pad for x in xs} | {tuple(-v for v in x) + pad for x in xs})
        _state["mixed"] = want
    return _state["mixed"]


def test_auto_route_takes_both_routes_in_one_call(ctx, monkeypatch):
    """Lattices [1, 10) of a batch of 11: easy and hard ones interleaved, one beyond 63 bits, one with two equal rows.
    Which route AUTO gives a lattice is seen from single-lattice calls (last_kernel_ms is 0 when nothing went to the
    kernel).  In the one call over the range: the kernel ran, the easy lattices carry the kernel's deterministic node
    counts and the hard ones the enumerator's, every good lattice has its exact minimum, the bad ones zero outputs,
    and nothing is written behind the range.  Catches: a take mask indexed by the lattice instead of the place in the
    range, the kernel writing a lattice it was told to skip, the host's fill overwriting the kernel's."""
    from fplll_amd.gso import MatGSOBatch
    from test_svp_solver_gpu import _raw_call
    bs, roles = F.mixed_batch()
    want = _mixed_exact()
    first, count = F.MIXED_FIRST, F.MIXED_COUNT
    monkeypatch.setenv("FPHIP_SVP_WAVE_MAX_NODES", MIXED_LIMIT)
    g = MatGSOBatch(ctx, len(bs), 16, 17)
    try:
        g.set_basis(_np(bs))
        single = {}
        for k in range(first, first + count):
            if roles[k] in ("easy", "hard"):
                auto = g.shortest_vector(first=k, count=1, route="auto")
                ms = g.last_kernel_ms
                wave = g.shortest_vector(first=k, count=1, route="wave")
                enum = g.shortest_vector(first=k, count=1, route="enum")
                single[k] = dict(waved=ms > 0.0, auto=int(auto[3][0]), wave=int(wave[3][0]), enum=int(enum[3][0]))
                assert (ms > 0.0) == (roles[k] == "easy"), (k, roles[k], ms)
                assert single[k]["auto"] == (single[k]["wave"] if roles[k] == "easy" else single[k]["enum"])
        rc, a, SENT = _raw_call(g, first, count, "auto")
        ms = g.last_kernel_ms
    finally:
        g.close()
    C.note(lambda: ("mixed batch: %s" % {k: (roles[k], v) for k, v in single.items()},))
    assert rc == 0 and ms > 0.0  # the kernel ran ...
    hard = [k for k in single if roles[k] == "hard"]
    assert any(single[k]["enum"] != single[k]["wave"] for k in hard)  # ... and a route is seen from the node counts
    for w in range(count):
        k = first + w
        sol, vec = [int(v) for v in a["sol"][w]], [int(v) for v in a["vec"][w]]
        if roles[k] == "big":
            assert int(a["st"][w]) == -2 and not any(sol) and not any(vec) and int(a["norm"][w]) == 0 and int(a["nodes"][w]) == 0
        elif roles[k] == "equal":
            assert int(a["st"][w]) == 0 and not any(sol) and not any(vec) and int(a["norm"][w]) == 0 and int(a["nodes"][w]) == 0
        else:
            assert int(a["st"][w]) == 1 and int(a["norm"][w]) == want[k][0], (k, roles[k])
            assert tuple(sol) in want[k][1] and vec == X.vector_of(bs[k], sol)
            assert int(a["nodes"][w]) == single[k]["wave" if roles[k] == "easy" else "enum"], (k, roles[k])
    assert (a["sol"][count:] == SENT).all() and (a["vec"][count:] == SENT).all() and (a["norm"][count:] == SENT).all()
    assert (a["nodes"][count:] == 77).all() and (a["st"][count:] == SENT).all()


# ---- short_vectors / theta_series / vectors_near ---------------------------------------------------------------------
def _half(x):
    """One of +-x: the first non-zero coefficient from the top positive (exact_lattice's rule)."""
    x = tuple(int(v) for v in x)
    for v in reversed(x):
        if v:
            return x if v > 0 else tuple(-u for u in x)
    return x


def _same_list(b, got, want, target=None, signed=False):
    """count, the sorted list of (norm, coefficients) and the vectors of a device list against the exact list."""
    count, coef, vec, norm = got
    assert count == len(want) == len(norm), (count, len(want))
    pick = (lambda x: tuple(int(v) for v in x)) if signed else _half
    assert sorted((int(nv), pick(x)) for nv, x in zip(norm, coef)) == sorted((nv, pick(x)) for nv, x in want)
    assert list(norm) == sorted(norm)
    for x, v, nv in zip(coef, vec, norm):
        w = X.vector_of(b, [int(t) for t in x], target)
        assert [int(t) for t in v] == w and sum(t * t for t in w) == int(nv)


@pytest.mark.parametrize("name", LIST_MEMBERS)
def test_short_vectors_equal_the_exact_list(ctx, name):
    """Bounds that EQUAL a norm: lambda_1, lambda_1 - 1 (nothing), the second and third distinct norms of the lattice.
    At s = 2^29 they sit where (double)bound_sq is inexact and the tied norms differ by a few units in 2^61.
    Catches: a radius below the bound, the filter on a double, a vector lost or doubled at the boundary."""
    from fplll_amd.svp import short_vectors, theta_series
    b = F.basis(name)
    norms, lst = F.norms_exact(name)
    assert norms[0] == F.exact(name)["lam1"]
    assert short_vectors(ctx, _np(b), norms[0] - 1, reduce=False)[0] == 0
    for N in norms:
        _same_list(b, short_vectors(ctx, _np(b), N, reduce=False), [(nv, x) for nv, x in lst if nv <= N])
    theta = {}
    for nv, _ in lst:
        theta[nv] = theta.get(nv, 0) + 2
    assert theta_series(ctx, _np(b), norms[-1], reduce=False) == theta


def _near_case(name, k):
    """(t, d0 = the exact closest distance, the exact list within d0 + lambda_1 / 4) of target k of a member."""
    key = ("near", name, k)
    if key not in _state:
        b, t = F.basis(name), F.targets(name)[k][1]
        d0, xs, _ = X.closest_exact(b, t, max_nodes=F.NODE_CAP)
        lst, _ = X.near_exact(b, t, d0 + F.exact(name)["lam1"] // 4, max_nodes=F.NODE_CAP)
        _state[key] = (t, d0, xs, lst)
    return _state[key]


@pytest.mark.parametrize("name", LIST_MEMBERS)
def test_vectors_near_equal_the_exact_list(ctx, name):
    """Targets = lattice points plus offsets in [-6, 6], and (where the member has a lattice vector with even entries)
    a target exactly halfway between two lattice points.  Bounds: the exact closest distance d0 (every closest point
    and nothing else; the halfway target has at least two), d0 - 1 (nothing), and the largest distance within
    d0 + lambda_1 / 4."""
    from fplll_amd.svp import vectors_near
    b = F.basis(name)
    for k, (kind, t) in enumerate(F.targets(name)):
        if kind == "far":
            continue
        t, d0, xs, lst = _near_case(name, k)
        tt = np.array(t, dtype=np.int64)
        if d0 > 0:
            assert vectors_near(ctx, _np(b), tt, d0 - 1, reduce=False)[0] == 0, (name, kind)
        for N in (d0, lst[-1][0]):
            _same_list(b, vectors_near(ctx, _np(b), tt, N, reduce=False), [(nv, x) for nv, x in lst if nv <= N], t, signed=True)
        if kind == "half":
            assert len(xs) >= 2


# ---- closest_vector(s) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LIST_MEMBERS)
def test_closest_vectors_are_exact_closest_points(ctx, name):
    """Near, far (coefficients around 2^30) and halfway targets in one call: status 1, the distance of the answer —
    in Python integers — is closest_exact's, and the answer is one of the exact closest points (where they tie, any)."""
    from fplll_amd.gso import MatGSOBatch
    b = F.basis(name)
    tg = F.targets(name)
    g = MatGSOBatch(ctx, 1, len(b), len(b[0]))
    try:
        g.set_basis(_np(b))
        sol, dist, st = g.closest_vector(np.array([t for _, t in tg], dtype=np.int64))
    finally:
        g.close()
    for k, (kind, t) in enumerate(tg):
        key = ("closest", name, k)
        if key not in F._exact:
            F._exact[key] = X.closest_exact(b, t, max_nodes=F.NODE_CAP)
        d0, xs, _ = F._exact[key]
        assert int(st[k]) == 1, (name, kind, int(st[k]))
        x = tuple(int(v) for v in sol[k])
        got = sum(v * v for v in X.vector_of(b, x, t))
        assert got == d0, (name, kind, got, d0)
        assert x in set(xs), (name, kind)
        inside = float(d0 - X.target_perp(b, t))  # (the enumeration's distance: to the target's projection on the span)
        assert abs(float(dist[k]) - inside) <= 1e-9 * max(1.0, inside)


def test_halfway_target_ends_the_babai_loop_like_the_restatement(ctx):
    """root_e8_s20_full_0's halfway target: the preparation's nearest-plane loop alternates between two targets (x, -x,
    x, ...).  The kernel leaves the loop at the first pass that would undo the one before — status 1 after 3 passes,
    not -1 after 256 — and equals tests/cvp_solver_cases.prepare bit for bit, as on every other target."""
    from fplll_amd.gso import MatGSOBatch
    name = "root_e8_s20_full_0"
    b, tg = F.basis(name), F.targets(name)
    t = np.array([v for _, v in tg], dtype=np.int64)
    g = MatGSOBatch(ctx, 1, len(b), len(b[0]))
    try:
        g.set_basis(_np(b))
        assert g.update_gso()[0] == 1
        mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0))
        coef, tc, desc, st = g.cvp_prepare(t)
    finally:
        g.close()
    P = S.prepare(_np(b), mu, rd, t)
    k = [kind for kind, _ in tg].index("half")
    assert list(st) == list(P["status"]) == [1] * len(tg) and P["passes"][k] == 3
    assert np.array_equal(coef, P["coef"])
    assert np.array_equal(tc.view(np.uint64), P["target_coord"].view(np.uint64))
    assert np.array_equal(desc.view(np.uint64), P["descent"].view(np.uint64))


# ---- the margin in use ------------------------------------------------------------------------------------------------
MARGIN = 2.0 ** -30


@pytest.mark.parametrize("family", ["scaled_root", "knapsack", "wide"])
def test_margin_in_use(ctx, family):
    """Every record the raw list call returns on the device's own mu / r, at a radius of the third distinct norm (with
    the margin): the enumeration's double distance against the exact integer norm.  The largest relative deviation per
    family is printed (DESIGN.md 3f and profiles/svp_solver.md hold the table) and must stay within 2^-30, the
    condition under which the solvers' margin suffices."""
    from fplll_amd.gso import MatGSOBatch
    worst, where, records = 0.0, None, 0
    for name in F.names(family):
        b = F.basis(name)
        d = len(b)
        norms, lst = F.norms_exact(name)
        g = MatGSOBatch(ctx, 1, d, len(b[0]))
        try:
            g.set_basis(_np(b))
            assert g.update_gso()[0] == 1
            mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0))
        finally:
            g.close()
        radius = float(norms[-1]) * (1.0 + MARGIN)
        count, dist, x, _, _ = H.raw_list(ctx, np.ascontiguousarray(mu.T), rd, None, radius, None, 4096)
        assert len(lst) <= count <= 4096, (name, count, len(lst))
        dev = 0.0
        for k in range(count):
            nv = sum(v * v for v in X.vector_of(b, [int(v) for v in x[k]]))
            assert nv > 0
            dev = max(dev, float(abs(Fraction(float(dist[k])) - nv) / nv))  # (exact up to the last division)
        records += count
        C.note(lambda: ("margin in use: %-22s d=%d, %d bits, %d records, largest relative deviation %.3g = %.3g x 2^-30"
                        % (name, d, max(abs(v) for r in b for v in r).bit_length(), count, dev, dev / MARGIN),))
        if dev > worst:
            worst, where = dev, name
    C.note(lambda: ("margin in use: family %s: %d records, largest relative deviation %.3g (%s) = %.3g x 2^-30"
                    % (family, records, worst, where, worst / MARGIN),))
    assert worst <= MARGIN, (family, where, worst)
