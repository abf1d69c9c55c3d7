"""The closest-vector wave route on the GPU (fphip_closest_vector_ex, cvp_wave.hip): the kernel against its model
(tests/cvp_wave_model.py) bit for bit — fed with the device's own true mu / r_ii and the device's own preparation —,
against the exact integer closest points (tests/exact_lattice.py) and the reference's recorded answers; ties, the
grid-stride loop, the statuses, determinism and the declines.  Every call passes a finite node budget: a wrong walk ends
as status 2 and a failed assertion, not as a long launch."""
import ctypes

import numpy as np
import pytest

import conftest as C
import cvp_solver_cases as S
import cvp_wave_model as M
import exact_lattice as X
import solver_families as F

pytestmark = pytest.mark.gpu

BUDGET = 4_000_000
FAMILY = F.names("scaled_root", "knapsack", "wide") + ["steep_63", "steep_64"]
FIXTURES = dict(S.solver_fixtures())


def _np(b):
    return np.array(b, dtype=np.int64)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _both(ctx, b, tg, row_expo=True, max_nodes=BUDGET):
    """One WAVE call over all targets and the model on the device's own GSO and preparation: (device dict, model)."""
    from fplll_amd.gso import MatGSOBatch
    b, tg = _np(b), _np(tg)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1], row_expo=row_expo)
    try:
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0) if row_expo else None)
        coef, tc, desc, st = g.cvp_prepare(tg)
        sol, dist, norm, nodes, status = g.closest_vector(tg, route="wave", max_nodes=max_nodes, full=True)
    finally:
        g.close()
    model = M.solve(b, mu, rd, dict(coef=coef, target_coord=tc, descent=desc, status=st, targets=tg), max_nodes=max_nodes)
    return dict(sol=sol, dist=dist, norm=norm, nodes=nodes, status=status), model


def _assert_equal(dev, model, what):
    assert [int(v) for v in dev["status"]] == model["status"], what
    assert [[int(v) for v in row] for row in dev["sol"]] == model["sol_coord"], what
    assert [int(v) for v in dev["norm"]] == model["norm"], what
    assert [int(v) for v in dev["nodes"]] == model["nodes"], what
    assert _same_bits(dev["dist"], model["dist"]), what


def _assert_exact(name, dev):
    b = F.basis(name)
    for k, (kind, t) in enumerate(F.targets(name)):
        key = ("closest", name, k)  # (shared with the other solver tests: computed once per process)
        if key not in F._exact:
            F._exact[key] = X.closest_exact(b, t, max_nodes=F.NODE_CAP)
        d0, xs, _ = F._exact[key]
        x = tuple(int(v) for v in dev["sol"][k])
        assert int(dev["status"][k]) == 1 and int(dev["norm"][k]) == d0, (name, kind, int(dev["norm"][k]), d0)
        assert x in set(xs) and sum(v * v for v in X.vector_of(b, x, t)) == d0, (name, kind)


# ---- kernel == model, and the exact answers --------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY)
def test_kernel_equals_the_model_and_the_exact_closest_points(ctx, name):
    """Every target of a member in one call (near, far, halfway).  wide_n64 / n65 / n130 / n200, n256 are the four
    columns-per-lane instantiations; steep_63 / steep_64 the lane edge.  sol_coord, norm, nodes, dist and status are
    the model's bit for bit; norm is closest_exact's distance and the answer one of its closest points."""
    tg = [t for _, t in F.targets(name)]
    dev, model = _both(ctx, F.basis(name), tg)
    C.note(lambda: ("%s: nodes %s" % (name, [int(v) for v in dev["nodes"]]),))
    _assert_equal(dev, model, name)
    _assert_exact(name, dev)


def test_kernel_equals_the_model_without_row_exponents(ctx):
    name = "knap_d16_b40"
    dev, model = _both(ctx, F.basis(name), [t for _, t in F.targets(name)], row_expo=False)
    _assert_equal(dev, model, name)
    _assert_exact(name, dev)


# ---- the recorded fixtures -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["wave", "auto"])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_sol_coord(ctx, name, route):
    """The reference's closest_vector answers, the lattice-point target (not walked, distance 0) and the far ones
    included; the near:10 target of q36 is a tree of 1.2 million nodes."""
    from fplll_amd.gso import MatGSOBatch
    fx = FIXTURES[name]
    b, tg = S.basis_of(fx), S.targets_of(fx)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        sol, dist, norm, nodes, st = g.closest_vector(tg, route=route, max_nodes=BUDGET, full=True)
    finally:
        g.close()
    assert list(st) == [1] * len(tg)
    assert [[int(v) for v in s] for s in sol] == [[int(v) for v in t["sol_coord"]] for t in fx["targets"]]
    for k, t in enumerate(fx["targets"]):
        diff = sol[k].astype(object).dot(b.astype(object)) - tg[k].astype(object)
        assert int(norm[k]) == sum(int(v) ** 2 for v in diff)
        if t["kind"] == "lattice":
            assert int(norm[k]) == 0 and dist[k] == 0.0 and int(nodes[k]) == 0


# ---- ties and edges --------------------------------------------------------------------------------------------------
def test_a_256_way_tie_keeps_the_first_candidate(ctx):
    """2 I_8 around (1, .., 1): 256 closest points at distance 8, all of them candidates (510 nodes); the first wins."""
    dev, model = _both(ctx, 2 * np.eye(8, dtype=np.int64), np.ones((1, 8), dtype=np.int64))
    _assert_equal(dev, model, "tie")
    assert int(dev["norm"][0]) == 8 and int(dev["nodes"][0]) == 510 and list(dev["sol"][0]) == [1] * 8


def test_two_rows_and_one_row(ctx):
    b = np.array([[3, 1], [1, 4]], dtype=np.int64)
    tg = np.array([[7, 9], [4, 5], [-30, 11]], dtype=np.int64)
    dev, model = _both(ctx, b, tg)
    _assert_equal(dev, model, "two rows")
    for k in range(3):
        d0, xs, _ = X.closest_exact(b.tolist(), tg[k].tolist())
        assert int(dev["norm"][k]) == d0 and tuple(int(v) for v in dev["sol"][k]) in set(xs)
    assert int(dev["nodes"][0]) >= 2 and int(dev["nodes"][1]) == 0  # (4, 5) is a lattice point: not walked
    dev, model = _both(ctx, np.array([[5, 0, 0]], dtype=np.int64), np.array([[12, 1, 0], [13, 0, 0]], dtype=np.int64))
    _assert_equal(dev, model, "one row")
    assert [list(s) for s in dev["sol"]] == [[2], [3]] and list(dev["norm"]) == [5, 4] and list(dev["nodes"]) == [0, 0]


# ---- the grid-stride loop --------------------------------------------------------------------------------------------
def test_grid_stride_and_partial_workgroups(ctx, monkeypatch):
    """One workgroup (FPHIP_CVP_WAVE_GRID=1: four waves) over T = 1, 3, 64, 65, 257 targets: every row equals the
    result of its own T = 1 call.  Catches: a target skipped or solved twice, outputs indexed by the wave instead of
    the target, state left over from the target before."""
    from fplll_amd.gso import MatGSOBatch
    name = "knap_d12_b30"
    b = _np(F.basis(name))
    rng = np.random.default_rng(1230)
    base = [t for _, t in F.targets(name)]
    for _ in range(7 - len(base)):
        c = rng.integers(-8, 9, size=b.shape[0])
        base.append([int(v) for v in c.astype(object).dot(b.astype(object)) + rng.integers(-6, 7, size=b.shape[1])])
    base = _np(base)
    monkeypatch.setenv("FPHIP_CVP_WAVE_GRID", "1")
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        single = [g.closest_vector(base[k:k + 1], route="wave", max_nodes=BUDGET, full=True) for k in range(len(base))]
        assert all(int(s[4][0]) == 1 for s in single) and len({int(s[3][0]) for s in single}) > 1
        for T in (1, 3, 64, 65, 257):
            pick = [k % len(base) for k in range(T)]
            out = g.closest_vector(base[pick], route="wave", max_nodes=BUDGET, full=True)
            for a, name_ in zip(range(5), ("sol", "dist", "norm", "nodes", "status")):
                want = np.concatenate([single[k][a] for k in pick])
                assert np.array_equal(out[a], want), (T, name_)
    finally:
        g.close()


# ---- statuses --------------------------------------------------------------------------------------------------------
def test_overflowing_target_gives_minus_two_and_spares_the_others(ctx):
    b, _, _, tg = S.overflow_case()
    dev, model = _both(ctx, b, tg)
    _assert_equal(dev, model, "overflow")
    assert list(dev["status"]) == [-2, 1, 1] and not dev["sol"][0].any() and int(dev["norm"][0]) == 0
    assert list(dev["sol"][1]) == [5 - 7 * 2**20, 7] and list(dev["norm"][1:]) == [0, 0]


def test_budget_in_the_wave_route_and_in_auto(ctx, monkeypatch):
    """knap_d20_b30's first near target (about 2 000 nodes).  WAVE under max_nodes = 500: status 2, the model's nodes
    and best so far.  AUTO with 500 nodes per target from the environment: status 1, the exact closest point, and
    nodes of both stages together."""
    from fplll_amd.gso import MatGSOBatch
    name = "knap_d20_b30"
    b, t = F.basis(name), F.targets(name)[0][1]
    dev, model = _both(ctx, b, [t], max_nodes=500)
    _assert_equal(dev, model, "budget")
    assert int(dev["status"][0]) == M.NODE_LIMIT and 500 <= int(dev["nodes"][0]) < 520
    d0, xs, _ = X.closest_exact(b, t, max_nodes=F.NODE_CAP)
    assert int(dev["norm"][0]) == sum(v * v for v in X.vector_of(b, [int(v) for v in dev["sol"][0]], t)) >= d0
    monkeypatch.setenv("FPHIP_CVP_WAVE_NODES_PER_TARGET", "500")
    g = MatGSOBatch(ctx, 1, len(b), len(b[0]))
    try:
        g.set_basis(_np(b))
        sol, dist, norm, nodes, st = g.closest_vector(_np([t]), route="auto", full=True)
    finally:
        g.close()
    assert int(st[0]) == 1 and int(norm[0]) == d0 and tuple(int(v) for v in sol[0]) in set(xs)
    assert int(nodes[0]) >= int(dev["nodes"][0])
    C.note(lambda: ("auto under 500 nodes per target: %d nodes in both stages, the wave stage %d"
                    % (int(nodes[0]), int(dev["nodes"][0])),))


def test_two_calls_give_identical_arrays(ctx):
    from fplll_amd.gso import MatGSOBatch
    fx = FIXTURES["cvpsolve_q24.json"]
    b = S.basis_of(fx)
    tg = np.concatenate([S.targets_of(fx)] * 13)  # 65 targets: more than one workgroup, a partial one
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        one = g.closest_vector(tg, route="wave", max_nodes=BUDGET, full=True)
        two = g.closest_vector(tg, route="wave", max_nodes=BUDGET, full=True)
    finally:
        g.close()
    for a, c in zip(one, two):
        assert np.array_equal(a, c)
    assert _same_bits(one[1], two[1]) and list(one[4]) == [1] * 65


# ---- declines --------------------------------------------------------------------------------------------------------
def test_declines(ctx):
    """The WAVE route at 72 rows, CVPM_PROVED and an unknown route: declined with a text, nothing launched (the kernel
    time of the object stays what loading the basis left)."""
    from fplll_amd import _lib
    from fplll_amd.enumeration import Unsupported
    from fplll_amd.gso import MatGSOBatch
    b = 1000 * np.eye(72, dtype=np.int64)
    tg = np.full((2, 72), 3, dtype=np.int64)
    g = MatGSOBatch(ctx, 1, 72, 72)
    try:
        g.set_basis(b)
        before = g.last_kernel_ms
        with pytest.raises(Unsupported, match="WAVE route takes at most 64 rows"):
            g.closest_vector(tg, route="wave", max_nodes=BUDGET)
        with pytest.raises(Unsupported, match="CVPM_PROVED.*CVPM_FAST only"):
            g.closest_vector(tg, route="wave", method=2, max_nodes=BUDGET)
        with pytest.raises(ValueError, match="route"):
            g.closest_vector(tg, route="fastest", max_nodes=BUDGET)
        fn = _lib.bind_closest_vector_ex(g.lib)
        sol, st = np.zeros((2, 72), dtype=np.int64), np.zeros(2, dtype=np.int32)
        rc = fn(g.h, None, 0, 2, tg.ctypes.data_as(ctypes.c_void_p), 0, 7, BUDGET, sol.ctypes.data_as(ctypes.c_void_p),
                None, None, None, st.ctypes.data_as(ctypes.c_void_p))
        assert rc == _lib.FPHIP_ERROR and "unknown route" in ctx.last_error()
        assert g.last_kernel_ms == before
        # AUTO at 72 rows goes the ENUM route: the planted points
        sol, dist, st = g.closest_vector(tg, route="auto", max_nodes=BUDGET)
        assert list(st) == [1, 1] and not sol.any()
    finally:
        g.close()
