"""The shortest-vector solver on the GPU (fplll_amd.svp.shortest_vector, MatGSOBatch.shortest_vector,
fphip_shortest_vector): both routes against shortest_vector runs of the reference itself (tests/golden/svpsolve_*.json,
its example pair, its rank-defect matrix), the WAVE route against the kernel's model (tests/svp_model.py fed with the
device's own mu / r / row exponents: sol_coord, norm and nodes bit for bit), the batch mechanics of the kernel, and the
declined calls.  Each case names the mistake it catches."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import conftest as C
import list_helpers as H
import svp_model as M

pytestmark = pytest.mark.gpu

FIXTURES = {os.path.basename(p)[:-5]: json.load(open(p)) for p in sorted(glob.glob(os.path.join(C.GOLDEN, "svpsolve_q*.json")))}
_cache = {}


def _example_in():
    txt = open(os.path.join(C.GOLDEN, "example_svp_in.txt")).read().replace("[", " ").replace("]", " ")
    return np.array([int(t) for t in txt.split()], dtype=np.int64).reshape(20, 21)


def _example_out():
    txt = open(os.path.join(C.GOLDEN, "example_svp_out.txt")).read().replace("[", " ").replace("]", " ")
    return [int(t) for t in txt.split()]


def _ints(a):
    return [int(v) for v in a]


def _check(b, sol, vec, norm):
    """vec == sol_coord b and |vec|^2 == norm in Python integers, sol_coord != 0."""
    b = np.asarray(b).astype(object)
    v = np.array(_ints(sol), dtype=object).dot(b)
    assert _ints(v) == _ints(vec)
    assert sum(int(t) ** 2 for t in vec) == int(norm)
    assert any(_ints(sol))


def _wave_and_model(ctx, b, pruning=None, row_expo=True):
    """One lattice: the WAVE route, and the model on the device's own GSO.  Returns (device outputs, model)."""
    from fplll_amd.gso import MatGSOBatch
    b = np.ascontiguousarray(b, dtype=np.int64)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1], row_expo=row_expo)
    try:
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        mu, r, e = g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0)
        out = g.shortest_vector(route="wave", pruning=pruning)
    finally:
        g.close()
    m = M.solve(b.tolist(), mu.tolist(), np.diag(r).tolist(), [int(v) for v in e], pruning=pruning, row_expo=row_expo)
    return out, m


def _same_as_model(out, m):
    sol, vec, norm, nodes, st = out
    assert int(st[0]) == m["status"]
    assert _ints(sol[0]) == m["sol_coord"], "sol_coord"
    assert _ints(vec[0]) == m["vec"] and int(norm[0]) == m["norm"], "vec / norm"
    assert int(nodes[0]) == m["nodes"], "nodes"


def _reduced(ctx, d, n, seed, span=60):
    """A seeded d x n basis, LLL-reduced on the device; cached for the module."""
    from fplll_amd.gso import lll_reduction
    key = (d, n, seed, span)
    if key not in _cache:
        rng = np.random.default_rng(1000 * d + 7 * n + seed)
        b, _, status, _ = lll_reduction(ctx, rng.integers(-span, span + 1, size=(d, n)), with_u=False)
        assert status == 1
        _cache[key] = b
    return _cache[key]


def _steep(d):
    """d x d, 40 (+ a little) on the diagonal and entries in {-1, 0, 1} elsewhere: r_ii all about 1600, so
    last_useful_index keeps every row and the tree within radius ~ 37^2 has a few thousand nodes.  Row d - 2 is the
    shortest but hidden: b_{d-2} += b_{d-1}, so the answer needs the coefficient of the LAST row (lane d - 1)."""
    rng = np.random.default_rng(d)
    b = np.diag([40 + (i % 5) for i in range(d)]).astype(np.int64) + rng.integers(-1, 2, size=(d, d))
    b[d - 2, d - 2] = 37
    b[d - 2] += b[d - 1]
    return b


# ---- 1. the reference's answers, both routes -------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["wave", "enum"])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_norm_on_every_fixture(ctx, name, route):
    """status 1, the reference's norm exactly (FAST == PROVED in every fixture), vec = sol_coord b, |vec|^2 = norm.
    Catches: a radius that cuts the shortest vector, a stale best after an improvement, a declined small ENUM call."""
    from fplll_amd.gso import MatGSOBatch
    fx = FIXTURES[name]
    b = np.array(fx["basis"], dtype=np.int64)
    g = MatGSOBatch(ctx, 1, fx["d"], fx["n"])
    try:
        g.set_basis(b)
        sol, vec, norm, nodes, st = g.shortest_vector(route=route)
    finally:
        g.close()
    C.note(lambda: ("%s %s: norm %d, %d nodes (reference: %.1f ms on one core)" % (name, route, norm[0], nodes[0],
                                                                                   fx["fast"]["ref_ms"]),))
    assert int(st[0]) == 1 and int(norm[0]) == fx["fast"]["norm"] == fx["proved"]["norm"]
    _check(b, sol[0], vec[0], norm[0])
    _cache[("norm", name, route)] = int(norm[0])


def test_routes_agree_on_every_fixture(ctx):
    """WAVE and ENUM end on the same norm (the vector may differ where minima tie: the parallel walk's order)."""
    from fplll_amd.svp import shortest_vector
    for name, fx in sorted(FIXTURES.items()):
        got = {}
        for route in ("wave", "enum"):
            if ("norm", name, route) not in _cache:
                _cache[("norm", name, route)] = shortest_vector(ctx, fx["basis"], reduce=False, route=route)[2]
            got[route] = _cache[("norm", name, route)]
        assert got["wave"] == got["enum"], name


@pytest.mark.parametrize("route", ["auto", "wave", "enum"])
def test_reference_example_pair_with_reduction(ctx, route):
    """example_svp_in (20 x 21, not reduced) with reduce=True: the norm of example_svp_out, and sol_coord is expressed
    in the CALLER's basis through u.  Catches: coefficients left in the reduced basis."""
    from fplll_amd.svp import shortest_vector
    b_in = _example_in()
    sol, vec, norm = shortest_vector(ctx, b_in, reduce=True, route=route)
    assert norm == sum(t * t for t in _example_out())
    _check(b_in, sol, vec, norm)


def test_rank_defect_matrix_and_the_list_path(ctx):
    """The 4 x 4 matrix of the reference's test_rank_defect reduces and solves; and on it and on every fixture up to
    d = 32 an independent device path agrees that nothing is shorter: theta_series up to the norm has one key."""
    from fplll_amd.svp import shortest_vector, theta_series
    rd = np.array(json.load(open(os.path.join(C.GOLDEN, "svp_rank_defect.json")))["basis"], dtype=np.int64)
    sol, vec, norm = shortest_vector(ctx, rd)
    _check(rd, sol, vec, norm)
    assert list(theta_series(ctx, rd, norm)) == [norm]
    for name, fx in sorted(FIXTURES.items()):
        if fx["d"] <= 32:
            assert list(theta_series(ctx, fx["basis"], fx["fast"]["norm"], reduce=False)) == [fx["fast"]["norm"]], name


PREFIX_ROWS = 60


def test_enum_route_on_a_prefix_of_the_bkz20_basis(ctx):
    """The first rows of the BKZ-20 basis of dimension 180 (tests/golden/basis_q180_seed0_lll_bkz20.txt), n = 180
    columns.  72 rows were asked for if their tree finishes within a test's few seconds: it does not (the
    Gaussian-heuristic estimate at radius |b_0|^2 is 1.4e15 nodes at 72 rows, 5e12 at 66 — measured: 49 s — and 4e10 at
    60), so this is the largest even prefix that does: 60 rows, 1.7e10 nodes, 0.7 s.  No reference ran on it: the
    answer is checked by its own integers, against the rows of the basis, and by the list path (theta_series up to
    the norm has one key: nothing shorter exists).  The rows above 64 are test_enum_route_above_64_rows' business."""
    from fplll_amd.svp import theta_series
    from fplll_amd.gso import MatGSOBatch, load_basis_txt
    b = np.ascontiguousarray(load_basis_txt(os.path.join(C.GOLDEN, "basis_q180_seed0_lll_bkz20.txt"))[:PREFIX_ROWS], dtype=np.int64)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        sol, vec, norm, nodes, st = g.shortest_vector(route="enum")
    finally:
        g.close()
    C.note(lambda: ("prefix of %d rows, enum: norm %d, %d nodes" % (PREFIX_ROWS, norm[0], nodes[0]),))
    assert int(st[0]) == 1 and 0 < int(norm[0]) <= min(sum(int(t) ** 2 for t in r) for r in b)
    _check(b, sol[0], vec[0], norm[0])
    assert list(theta_series(ctx, b, int(norm[0]), reduce=False)) == [int(norm[0])]


def test_enum_route_above_64_rows(ctx):
    """72 x 72, 1000 on the diagonal and entries in [-20, 20] elsewhere; row 70 is the shortest (900 on its diagonal)
    but hidden: b_70 += b_71.  The answer b_70 - b_71 needs the coefficients of the levels >= 64, which come back
    through the enumerator's top walk; every other vector is longer (two rows combined: about 2e6 > 1e6).  AUTO above
    64 rows is ENUM; the WAVE route declines the object."""
    from fplll_amd.enumeration import Unsupported
    from fplll_amd.gso import MatGSOBatch
    rng = np.random.default_rng(72)
    b = 1000 * np.eye(72, dtype=np.int64) + rng.integers(-20, 21, size=(72, 72))
    b[70, 70] = 900
    want = sum(int(t) ** 2 for t in b[70])
    assert want < min(sum(int(t) ** 2 for t in r) for k, r in enumerate(b) if k != 70)
    b[70] += b[71]
    g = MatGSOBatch(ctx, 1, 72, 72)
    try:
        g.set_basis(b)
        for route in ("enum", "auto"):
            sol, vec, norm, nodes, st = g.shortest_vector(route=route)
            assert int(st[0]) == 1 and int(norm[0]) == want
            assert [abs(v) for v in _ints(sol[0])] == [0] * 70 + [1, 1] and int(sol[0][70]) == -int(sol[0][71])
            _check(b, sol[0], vec[0], norm[0])
        with pytest.raises(Unsupported, match="at most 64 rows"):
            g.shortest_vector(route="wave")
    finally:
        g.close()


# ---- 2. the WAVE route is the model, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_degenerate_dimensions(ctx, d):
    """d = 1: nothing to walk; d = 2, 3: loops of one and two levels.  Catches: a walk entered with one row, the
    node compensation d - 1 on a tree of a handful of nodes."""
    b = [[7, 2, 1, 0]] if d == 1 else H.lll_exact(np.random.default_rng(d).integers(-30, 31, size=(d, 4)).tolist())
    out, m = _wave_and_model(ctx, b)
    _same_as_model(out, m)
    assert int(out[2][0]) == M.brute_force_min(b) if d > 1 else int(out[2][0]) == 54


@pytest.mark.parametrize("d", [63, 64])
def test_lane_edge(ctx, d):
    """Rows up to lane 63, the answer b_{d-2} - b_{d-1} uses the last lane.  Catches: an off-by-one in the lane masks
    (lane < k, readlane of level d - 1), the LDS triangle's size at d = 64.  The norm is the exact minimum of the
    lattice (tests/exact_lattice.py on the same basis): the model is not the only witness."""
    import solver_families as F
    b = _steep(d)
    assert b.tolist() == F.basis("steep_%d" % d)
    out, m = _wave_and_model(ctx, b)
    _same_as_model(out, m)
    assert m["d_eff"] == d and m["improvements"] >= 1 and m["sol_coord"][d - 1] != 0
    _check(b, out[0][0], out[1][0], out[2][0])
    F.check_shortest("steep_%d" % d, out[0][0], out[1][0], out[2][0])


@pytest.mark.parametrize("n", [64, 65, 130, 200])
def test_every_width_class(ctx, n):
    """d = 16 with n = 64, 65, 130, 200 columns: one case per columns-per-lane class, three with a partial last column
    group.  Catches: a column beyond n read or written, a norm that misses the last group.  The norm is the exact
    minimum of the first d_eff rows (rational enumeration, tests/exact_lattice.py) and sol_coord one of its minimal
    vectors."""
    import exact_lattice as X
    b = _reduced(ctx, 16, n, 0)
    out, m = _wave_and_model(ctx, b)
    _same_as_model(out, m)
    _check(b, out[0][0], out[1][0], out[2][0])
    de = X.d_eff_exact(b.tolist())
    lam1, xs, _ = X.lambda1_exact(b.tolist(), rows=de, max_nodes=200000)
    assert m["d_eff"] == de and int(out[2][0]) == lam1
    sol = tuple(_ints(out[0][0]))
    assert not any(sol[de:]) and (sol[:de] in xs or tuple(-v for v in sol[:de]) in xs)


def test_pruned_walk(ctx):
    """Linear pruning on d = 32: the level bound is pruning[k] * radius, also after the radius shrinks.  Catches: the
    bounds not rescaled on an improvement, pruning indexed from the wrong end."""
    b = FIXTURES["svpsolve_q32_s1"]["basis"]
    pr = [0.4 + 0.6 * (k + 1) / 32 for k in range(32)]
    out, m = _wave_and_model(ctx, b, pruning=pr)
    _same_as_model(out, m)
    full, mf = _wave_and_model(ctx, b)
    _same_as_model(full, mf)
    assert int(out[3][0]) < int(full[3][0])


def test_no_walk_cases(ctx):
    """N0 = 1: the radius (N0 - 1) is 0, e_i0 is the answer and no node is counted.  A basis that already holds the
    shortest vector (fixture q24_s2): the walk runs, nothing is STRICTLY shorter, the answer is e_i0 and the nodes are
    those of a walk without an improvement.  Catches: a tie taken as an improvement, a walk at radius 0."""
    out, m = _wave_and_model(ctx, [[1, 0, 0], [0, 3, 1], [0, 1, 4]])
    _same_as_model(out, m)
    assert _ints(out[0][0]) == [1, 0, 0] and int(out[2][0]) == 1 and int(out[3][0]) == 0
    fx = FIXTURES["svpsolve_q24_s2"]
    out, m = _wave_and_model(ctx, fx["basis"])
    _same_as_model(out, m)
    assert m["improvements"] == 0 and sum(abs(v) for v in _ints(out[0][0])) == 1 and int(out[3][0]) > 0
    assert int(out[2][0]) == fx["fast"]["norm"]


@pytest.mark.parametrize("row_expo", [True, False])
def test_rows_cut_by_last_useful_index(ctx, row_expo):
    """The last two rows are 2^20 times the others: d_eff = 4 < d = 6, their coefficients stay 0 — decided on the TRUE
    r_ii.  Catches: the stored r compared without the row exponents (they differ by 20 here)."""
    top = [[10, 1, 0, 0, 1, 0], [0, 10, 1, 0, 0, 1], [1, 0, 10, 1, 0, 0], [0, 1, 0, 10, 1, 0]]
    b = top + [[(1 << 20) * v for v in row] for row in ([1, -2, 0, 3, 5, 1], [2, 0, -1, 1, 1, 4])]
    out, m = _wave_and_model(ctx, b, row_expo=row_expo)
    _same_as_model(out, m)
    assert m["d_eff"] == 4 and _ints(out[0][0])[4:] == [0, 0]
    assert int(out[2][0]) == _wave_and_model(ctx, top, row_expo=row_expo)[1]["norm"]


def test_tied_minima(ctx):
    """D4 (24 minimal vectors) and E8 (240): the first of minimal norm in depth-first order, as the model walks it."""
    for b, want in ((H.d4_basis(), 2), (H.lll_exact(H.e8_basis()[0]), 8), (H.e8_basis()[0], 8)):
        out, m = _wave_and_model(ctx, b)
        _same_as_model(out, m)
        assert int(out[2][0]) == want


# ---- 3. batch mechanics -----------------------------------------------------------------------------------------------
def _batch_case(ctx):
    """19 different 16 x 65 bases and their one-lattice results."""
    if "batch" not in _cache:
        bs = np.stack([_reduced(ctx, 16, 65, s) for s in range(19)])
        single = [_wave_and_model(ctx, b)[0] for b in bs]
        _cache["batch"] = (bs, single)
    return _cache["batch"]


@pytest.mark.parametrize("count", [1, 5, 19])
def test_batches_equal_single_runs(ctx, count, monkeypatch):
    """1, 5 (more than the four waves of a workgroup) and 2 * 8 + 3 lattices on a grid shrunk to two workgroups of four
    waves (FPHIP_SVP_WAVE_GRID=2): the grid-stride loop goes round twice and a third, partial time.  Catches: LDS shared
    between the waves of a workgroup, per-lattice state kept across the loop, a lattice index that ignores the grid."""
    from fplll_amd.gso import MatGSOBatch
    bs, single = _batch_case(ctx)
    if count == 19:
        monkeypatch.setenv("FPHIP_SVP_WAVE_GRID", "2")
    g = MatGSOBatch(ctx, count, 16, 65)
    try:
        g.set_basis(bs[:count])
        sol, vec, norm, nodes, st = g.shortest_vector(route="wave")
        again = g.shortest_vector(route="wave")
    finally:
        g.close()
    for k in range(count):
        s1 = single[k]
        assert int(st[k]) == 1 and np.array_equal(sol[k], s1[0][0]) and np.array_equal(vec[k], s1[1][0])
        assert int(norm[k]) == int(s1[2][0]) and int(nodes[k]) == int(s1[3][0])
    for a, b in zip((sol, vec, norm, nodes, st), again):  # two runs give identical arrays
        assert np.array_equal(a, b)


def _raw_call(g, first, count, route, guard=2, method=0, flags=0, null=None):
    """fphip_shortest_vector with `guard` lattices of sentinel behind the count lattices of every output array."""
    from fplll_amd import _lib
    fn = _lib.bind_shortest_vector(g.lib)
    SENT = -77
    arrs = dict(sol=np.full((count + guard, g.d), SENT, dtype=np.int64), vec=np.full((count + guard, g.n), SENT, dtype=np.int64),
                norm=np.full(count + guard, SENT, dtype=np.int64), nodes=np.full(count + guard, 77, dtype=np.uint64),
                st=np.full(count + guard, SENT, dtype=np.int32))
    ptr = {k: (None if k == null else v.ctypes.data_as(ctypes.c_void_p)) for k, v in arrs.items()}
    rc = fn(g.h, None, first, count, method, flags, None, _lib.SVP_ROUTES[route], ptr["sol"], ptr["vec"], ptr["norm"],
            ptr["nodes"], ptr["st"])
    return rc, arrs, SENT


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_sub_range_leaves_the_rest_untouched(ctx, route):
    """first_lattice = 2, count = 3 of a batch of 7: the outputs are those of lattices 2, 3, 4, in places 0, 1, 2, and
    nothing is written behind them.  Catches: outputs indexed by the lattice instead of the place in the range."""
    from fplll_amd.gso import MatGSOBatch
    bs, single = _batch_case(ctx)
    g = MatGSOBatch(ctx, 7, 16, 65)
    try:
        g.set_basis(bs[:7])
        rc, a, SENT = _raw_call(g, 2, 3, route)
    finally:
        g.close()
    assert rc == 0
    for w in range(3):
        s1 = single[2 + w]
        assert int(a["st"][w]) == 1 and int(a["norm"][w]) == int(s1[2][0])
        if route == "wave":
            assert np.array_equal(a["sol"][w], s1[0][0]) and np.array_equal(a["vec"][w], s1[1][0])
            assert int(a["nodes"][w]) == int(s1[3][0])
        _check(bs[2 + w], a["sol"][w], a["vec"][w], a["norm"][w])
    assert (a["sol"][3:] == SENT).all() and (a["vec"][3:] == SENT).all() and (a["norm"][3:] == SENT).all()
    assert (a["nodes"][3:] == 77).all() and (a["st"][3:] == SENT).all()


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_overflowing_lattice_spares_its_neighbours(ctx, route):
    """Lattice 1 of 3 has a row with entries 2^62: status -2 and zero outputs for it, the neighbours as alone."""
    from fplll_amd.gso import MatGSOBatch
    bs, single = _batch_case(ctx)
    bad = bs[:3].copy()
    bad[1, 5, :] = 0
    bad[1, 5, 3] = 2**62
    bad[1, 5, 64] = 2**62
    g = MatGSOBatch(ctx, 3, 16, 65)
    try:
        g.set_basis(bad)
        sol, vec, norm, nodes, st = g.shortest_vector(route=route)
    finally:
        g.close()
    assert _ints(st) == [1, -2, 1]
    assert not sol[1].any() and not vec[1].any() and int(norm[1]) == 0 and int(nodes[1]) == 0
    for k in (0, 2):
        assert int(norm[k]) == int(single[k][2][0])
        _check(bad[k], sol[k], vec[k], norm[k])
    from fplll_amd import _lib
    from fplll_amd.svp import shortest_vector_batch
    with pytest.raises(_lib.HipError, match="lattice 1 .*-2"):
        shortest_vector_batch(ctx, bad, reduce=False, route=route)


def test_auto_route_splits_a_batch_by_the_node_estimate(ctx, monkeypatch):
    """FPHIP_SVP_WAVE_MAX_NODES: below every estimate all lattices go to the enumerator, above every estimate all to
    the kernel; the norms are the same either way and the kernel's node counts show who walked."""
    from fplll_amd.gso import MatGSOBatch
    bs, single = _batch_case(ctx)
    g = MatGSOBatch(ctx, 5, 16, 65)
    try:
        g.set_basis(bs[:5])
        monkeypatch.setenv("FPHIP_SVP_WAVE_MAX_NODES", "1e30")
        wave = g.shortest_vector(route="auto")
        monkeypatch.setenv("FPHIP_SVP_WAVE_MAX_NODES", "1e-30")
        enum = g.shortest_vector(route="auto")
    finally:
        g.close()
    for k in range(5):
        assert int(wave[2][k]) == int(enum[2][k]) == int(single[k][2][0])
        assert int(wave[3][k]) == int(single[k][3][0])  # the kernel's count: the deterministic walk
        _check(bs[k], enum[0][k], enum[1][k], enum[2][k])


# ---- 4. declined calls ------------------------------------------------------------------------------------------------
def test_declined_calls_launch_nothing(ctx):
    """SVPM_PROVED, SVP_DUAL, SVP_OVERRIDE_BND, the WAVE route with 65 rows, a NULL output: FPHIP_UNSUPPORTED (or an
    error) with a text, and not one output is written."""
    from fplll_amd import _lib
    from fplll_amd.enumeration import Unsupported
    from fplll_amd.gso import MatGSOBatch
    bs, _ = _batch_case(ctx)
    g = MatGSOBatch(ctx, 2, 16, 65)
    try:
        g.set_basis(bs[:2])
        for kw, text in ((dict(method=_lib.SVPM_PROVED), "SVPM_FAST only"), (dict(flags=_lib.SVP_DUAL), "SVP_DUAL"),
                         (dict(flags=_lib.SVP_OVERRIDE_BND), "SVP_OVERRIDE_BND"), (dict(method=1), "SVPM_FAST only")):
            rc, a, SENT = _raw_call(g, 0, 2, "auto", **kw)
            assert rc == _lib.FPHIP_UNSUPPORTED and text in ctx.last_error()
            assert all((v == (77 if k == "nodes" else SENT)).all() for k, v in a.items())
            with pytest.raises(Unsupported, match=text):
                g.shortest_vector(**kw)
        for null in ("sol", "vec", "norm", "nodes", "st"):
            rc, a, SENT = _raw_call(g, 0, 2, "wave", null=null)
            assert rc == _lib.FPHIP_ERROR and "required" in ctx.last_error()
            assert all((v == (77 if k == "nodes" else SENT)).all() for k, v in a.items())
        rc, a, SENT = _raw_call(g, 1, 2, "wave")  # a range beyond the batch
        assert rc == _lib.FPHIP_ERROR and "outside the batch" in ctx.last_error()
    finally:
        g.close()
    g = MatGSOBatch(ctx, 1, 65, 65)
    try:
        g.set_basis(np.eye(65, dtype=np.int64) * 3)
        rc, a, SENT = _raw_call(g, 0, 1, "wave")
        assert rc == _lib.FPHIP_UNSUPPORTED and "at most 64 rows" in ctx.last_error()
        assert all((v == (77 if k == "nodes" else SENT)).all() for k, v in a.items())
    finally:
        g.close()
