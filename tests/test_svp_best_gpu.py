"""The N-shortest-vectors solver on the GPU (fplll_amd.svp.shortest_vectors, MatGSOBatch.shortest_vectors,
fphip_shortest_vectors): the WAVE route against the kernel's model (tests/svp_best_model.py fed with the device's own
mu / r / row exponents: found, sol_coord, vec, norm, nodes and status bit for bit) and against the exact rational
enumeration, the batch mechanics of the kernel, the ENUM route's norms against the exact answers, the AUTO route, the
recorded N-best runs of the reference (tests/golden/svpbest_*.json), and the declined calls."""
import ctypes
import glob
import json
import math
import os

import numpy as np
import pytest

import conftest as C
import exact_lattice as X
import list_helpers as H
import solver_families as F
import svp_best_model as BM

pytestmark = pytest.mark.gpu

FIXTURES = {os.path.basename(p)[:-5]: json.load(open(p)) for p in sorted(glob.glob(os.path.join(C.GOLDEN, "svpsolve_q*.json")))}
REF_FIXTURES = sorted(glob.glob(os.path.join(C.GOLDEN, "svpbest_*.json")))
_cache = {}


def _np(b):
    return np.ascontiguousarray(np.array(b, dtype=object).astype(np.int64))


def _ints(a):
    return [int(v) for v in a]


def _rows(a):
    return [[int(v) for v in r] for r in a]


def _call(ctx, b, K, bound=None, pruning=None, row_expo=True, route="wave", want_gso=False):
    """One lattice through MatGSOBatch.shortest_vectors: (found, sol [K][d], vec [K][n], norm [K], nodes, status) and,
    for the model, the device's own mu / r / row exponents."""
    from fplll_amd.gso import MatGSOBatch
    b = _np(b)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1], row_expo=row_expo)
    try:
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        gso = (g.get_mu_matrix(0).tolist(), np.diag(g.get_r_matrix(0)).tolist(), _ints(g.row_expo(0))) if want_gso else None
        found, sol, vec, norm, nodes, st = g.shortest_vectors(K, bound_sq=bound, pruning=pruning, route=route)
    finally:
        g.close()
    out = dict(found=int(found[0]), sol_coord=_rows(sol[0]), vec=_rows(vec[0]), norm=_ints(norm[0]), nodes=int(nodes[0]),
               status=int(st[0]))
    return (out, gso) if want_gso else out


def _wave_is_the_model(ctx, b, K, bound=None, pruning=None, row_expo=True):
    out, (mu, r, e) = _call(ctx, b, K, bound, pruning, row_expo, want_gso=True)
    m = BM.solve(_rows(b), mu, r, e, K, bound_sq=bound, pruning=pruning, row_expo=row_expo)
    for key in ("status", "found", "norm", "sol_coord", "vec", "nodes"):
        assert out[key] == m[key], key
    return out, m


def _valid(b, o):
    """Every returned record is distinct modulo +-, non-zero, with vec = sol_coord b and |vec|^2 = norm in Python
    integers; sorted by norm; entries beyond found are zero."""
    b = _rows(b)
    seen = set()
    for j in range(len(o["norm"])):
        x, v, nv = o["sol_coord"][j], o["vec"][j], o["norm"][j]
        if j >= o["found"]:
            assert not any(x) and not any(v) and nv == 0
            continue
        assert X.vector_of(b, x) == v and sum(t * t for t in v) == nv > 0
        assert j == 0 or o["norm"][j - 1] <= nv
        assert tuple(x) not in seen and tuple(-t for t in x) not in seen
        seen.add(tuple(x))


def _exact_q24(bound):
    if ("q24", bound) not in _cache:
        _cache[("q24", bound)] = [nv for nv, _ in X.short_exact(FIXTURES["svpsolve_q24_s1"]["basis"], bound)[0]]
    return _cache[("q24", bound)]


# ---- 1. the WAVE route is the model, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_degenerate_dimensions(ctx, d):
    """d = 1: the multiples of b_0 (a walk of one level); d = 2, 3: loops of one and two levels."""
    b = [[7, 2, 1, 0]] if d == 1 else H.lll_exact(np.random.default_rng(d).integers(-30, 31, size=(d, 4)).tolist())
    N0 = min(sum(v * v for v in r) for r in b)
    for K, bound in ((4, None), (5, 9 * N0), (2, 100 * N0)):
        out, m = _wave_is_the_model(ctx, b, K, bound)
        _valid(b, out)
        want = [nv for nv, _ in X.short_exact(b, bound or N0, rows=None if bound else m["d_eff"])[0]]
        assert out["norm"][:out["found"]] == want[:K]
    if d == 1:
        assert _call(ctx, b, 5, 54 * 9)["norm"] == [54, 216, 486, 0, 0]


@pytest.mark.parametrize("d", [63, 64])
def test_lane_edge(ctx, d):
    """Rows up to lane 63 at the third distinct norm: records that use the last lane, the LDS triangle at d = 64."""
    name = "steep_%d" % d
    b = F.basis(name)
    norms3, lst = F.norms_exact(name, 3)
    out, m = _wave_is_the_model(ctx, b, 64, norms3[2])
    assert out["norm"][:out["found"]] == [nv for nv, _ in lst][:64] and m["d_eff"] == d
    assert any(x[d - 1] != 0 for x in out["sol_coord"][:out["found"]])
    _valid(b, out)


@pytest.mark.parametrize("n", [64, 65, 130, 200, 256])
def test_every_width_class(ctx, n):
    """The wide members: one case per columns-per-lane class, three with a partial last column group, K = 5 and 64 at
    the third norm.  Catches: a column beyond n read or written, the final vec pass missing a group."""
    name = "wide_n%d" % n
    b = F.basis(name)
    norms3, lst = F.norms_exact(name, 3)
    for K in (5, 64):
        out, _ = _wave_is_the_model(ctx, b, K, norms3[2])
        assert out["norm"][:out["found"]] == [nv for nv, _ in lst][:K]
        _valid(b, out)


@pytest.mark.parametrize("bound", [3181, 3817])
@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_table_sizes_above_and_below_the_number_of_vectors(ctx, K, bound):
    """svpsolve_q24_s1: 26 vectors within 3181 (K = 63, 64 never fill: the radius never shrinks; K = 1, 2 do) and 233
    within 3817 (every K fills and shrinks).  Catches: the worst read from the wrong lane, the shift at rank K - 1."""
    b = FIXTURES["svpsolve_q24_s1"]["basis"]
    out, m = _wave_is_the_model(ctx, b, K, bound)
    want = _exact_q24(bound)
    assert out["found"] == min(K, len(want)) and out["norm"][:out["found"]] == want[:K]
    _valid(b, out)


def test_known_shells(ctx):
    """Z^8 (reduced): K = 8 keeps the eight of norm 1 and stops, K = 16 finds 8, bound 2 with K = 64 fills on the last
    vector; D4: twelve of norm 2, five, and 12 + 12 within 4; 2 E8: 64 of the 120 of norm 8."""
    z8 = H.lll_exact(H.z8_basis())
    assert _wave_is_the_model(ctx, z8, 8)[0]["norm"] == [1] * 8
    assert _wave_is_the_model(ctx, z8, 16)[0]["found"] == 8
    out, m = _wave_is_the_model(ctx, z8, 64, 2)
    assert out["norm"] == [1] * 8 + [2] * 56 and m["insertions"] == 64
    d4 = H.d4_basis()
    assert _wave_is_the_model(ctx, d4, 12)[0]["norm"] == [2] * 12
    assert _wave_is_the_model(ctx, d4, 5)[0]["norm"] == [2] * 5
    for K in (24, 64):
        out, _ = _wave_is_the_model(ctx, d4, K, 4)
        assert out["found"] == 24 and out["norm"][:24] == [2] * 12 + [4] * 12
    e8 = H.lll_exact(H.e8_basis()[0])
    out, _ = _wave_is_the_model(ctx, e8, 64)
    assert out["norm"] == [8] * 64
    _valid(e8, out)


@pytest.mark.parametrize("name", F.PRUNED)
def test_pruned_walk(ctx, name):
    """The level bound is pruning[k] * radius, also after the radius shrinks; found may stay below K."""
    b = F.basis(name)
    norms3, _ = F.norms_exact(name, 3)
    out, _ = _wave_is_the_model(ctx, b, 5, norms3[2], pruning=F.pruning_of(name))
    _valid(b, out)
    _wave_is_the_model(ctx, b, 3, None, pruning=F.pruning_of(name))


def test_pruning_can_leave_nothing(ctx):
    out, _ = _wave_is_the_model(ctx, H.d4_basis(), 4, pruning=[0.01] * 4)
    assert out["status"] == 1 and out["found"] == 0 and out["norm"] == [0] * 4


@pytest.mark.parametrize("row_expo", [True, False])
@pytest.mark.parametrize("name", F.names("cut_rows"))
def test_rows_cut_with_and_without_a_callers_bound(ctx, name, row_expo):
    """The cut_* members, row exponents on and off: the default bound cuts the rows last_useful_index cuts (on the TRUE
    r_ii), a caller's bound at the third norm keeps every row whose r_ii is within it."""
    b = F.basis(name)
    ex = F.exact(name)
    out, m = _wave_is_the_model(ctx, b, 8, None, row_expo=row_expo)
    assert m["d_eff"] == ex["d_eff"]
    assert out["norm"][:out["found"]] == [nv for nv, _ in X.short_exact(b, ex["N0"], rows=ex["d_eff"])[0]][:8]
    norms3, lst = F.norms_exact(name, 3)
    out, m = _wave_is_the_model(ctx, b, 64, norms3[2], row_expo=row_expo)
    assert out["norm"][:out["found"]] == [nv for nv, _ in lst][:64]
    _valid(b, out)


def test_row_cut_generalisation(ctx):
    """[[3, 0], [1, 5]] with bound 100: nine vectors (the reference's 2 r_00 rule would give three); cut_cut with bound
    577: 17 vectors, one of them on the last row."""
    out, _ = _wave_is_the_model(ctx, [[3, 0], [1, 5]], 64, 100)
    assert out["norm"][:out["found"]] == [9, 26, 29, 36, 41, 50, 74, 81, 89]
    out, _ = _wave_is_the_model(ctx, F.basis("cut_cut"), 64, 577)
    assert out["found"] == 17 and sum(1 for x in out["sol_coord"][:17] if x[4]) == 1


# ---- 2. the WAVE route against the exact answers ----------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names("scaled_root"))
def test_scaled_roots_against_the_exact_list(ctx, name):
    """Norms near 2^61 with near-tied minima, K = 5 at the third distinct norm: the five smallest exact norms."""
    b = F.basis(name)
    norms3, lst = F.norms_exact(name, 3)
    out = _call(ctx, b, 5, norms3[2])
    assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in lst][:5]
    _valid(b, out)


# ---- 3. batch mechanics -----------------------------------------------------------------------------------------------
def _batch_case(ctx):
    """19 reduced 16 x 65 bases, their per-lattice bounds (the default, N0 + N0 / 8 and N0 + N0 / 3 in turn: mixed
    `found` under a table of K = 6) and their one-lattice results.  Cached."""
    from fplll_amd.gso import lll_reduction
    if "batch" not in _cache:
        bs = []
        for s in range(19):
            rng = np.random.default_rng(1000 * 16 + 7 * 65 + s)
            b, _, status, _ = lll_reduction(ctx, rng.integers(-60, 61, size=(16, 65)), with_u=False)
            assert status == 1
            bs.append(b)
        bs = np.stack(bs)
        bounds = []
        for k in range(19):
            N0 = int(min((bs[k].astype(object) ** 2).sum(axis=1)))
            bounds.append((0, N0 + N0 // 8, N0 + N0 // 3)[k % 3])
        single = [_call(ctx, bs[k], 6, bounds[k] or None) for k in range(19)]
        _cache["batch"] = (bs, bounds, single)
    return _cache["batch"]


def _same_as_single(arrs, w, s1):
    found, sol, vec, norm, nodes, st = arrs
    assert int(st[w]) == s1["status"] and int(found[w]) == s1["found"] and _ints(norm[w]) == s1["norm"]
    assert _rows(sol[w]) == s1["sol_coord"] and _rows(vec[w]) == s1["vec"] and int(nodes[w]) == s1["nodes"]


@pytest.mark.parametrize("count", [1, 5, 19])
def test_batches_equal_single_runs(ctx, count, monkeypatch):
    """1, 5 and 2 * 8 + 3 lattices on a grid of two workgroups of four waves (FPHIP_SVP_WAVE_GRID=2), per-lattice
    bounds, mixed found; two calls give identical arrays.  Catches: LDS or table state shared between waves or kept
    across the grid-stride loop, the bound indexed by the lattice, records written into a neighbour's slots."""
    from fplll_amd.gso import MatGSOBatch
    bs, bounds, single = _batch_case(ctx)
    assert len({s["found"] for s in single}) > 1
    monkeypatch.setenv("FPHIP_SVP_WAVE_GRID", "2")
    g = MatGSOBatch(ctx, count, 16, 65)
    try:
        g.set_basis(bs[:count])
        arrs = g.shortest_vectors(6, bound_sq=bounds[:count], route="wave")
        again = g.shortest_vectors(6, bound_sq=bounds[:count], route="wave")
    finally:
        g.close()
    for k in range(count):
        _same_as_single(arrs, k, single[k])
    for a, b in zip(arrs, again):
        assert np.array_equal(a, b)


def _raw_call(g, first, count, K, route, guard=2, bound=None, method=0, flags=0, null=None):
    """fphip_shortest_vectors with `guard` lattices of sentinel behind the count lattices of every output array."""
    from fplll_amd import _lib
    fn = _lib.bind_shortest_vectors(g.lib)
    SENT = -77
    m = count + guard
    arrs = dict(found=np.full(m, SENT, dtype=np.int32), sol=np.full((m, K, g.d), SENT, dtype=np.int64),
                vec=np.full((m, K, g.n), SENT, dtype=np.int64), norm=np.full((m, K), SENT, dtype=np.int64),
                nodes=np.full(m, 77, dtype=np.uint64), st=np.full(m, SENT, dtype=np.int32))
    ptr = {k: (None if k == null else v.ctypes.data_as(ctypes.c_void_p)) for k, v in arrs.items()}
    bd = None if bound is None else np.ascontiguousarray(bound, dtype=np.int64)
    rc = fn(g.h, None, first, count, K, None if bd is None else bd.ctypes.data_as(ctypes.c_void_p), method, flags, None,
            _lib.SVP_ROUTES[route], ptr["found"], ptr["sol"], ptr["vec"], ptr["norm"], ptr["nodes"], ptr["st"])
    return rc, arrs, SENT


def _untouched(a, SENT, start=0):
    return all((v[start:] == (77 if k == "nodes" else SENT)).all() for k, v in a.items())


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_sub_range_leaves_the_rest_untouched(ctx, route):
    """first_lattice = 2, count = 3 of a batch of 7: the outputs are those of lattices 2, 3, 4 in places 0, 1, 2 with
    THEIR bounds (bound_sq is indexed by the place in the range), and nothing is written behind them."""
    from fplll_amd.gso import MatGSOBatch
    bs, bounds, single = _batch_case(ctx)
    g = MatGSOBatch(ctx, 7, 16, 65)
    try:
        g.set_basis(bs[:7])
        rc, a, SENT = _raw_call(g, 2, 3, 6, route, bound=bounds[2:5])
    finally:
        g.close()
    assert rc == 0
    for w in range(3):
        s1 = single[2 + w]
        assert int(a["st"][w]) == 1 and int(a["found"][w]) == s1["found"] and _ints(a["norm"][w]) == s1["norm"]
        if route == "wave":
            assert _rows(a["sol"][w]) == s1["sol_coord"] and _rows(a["vec"][w]) == s1["vec"] and int(a["nodes"][w]) == s1["nodes"]
        _valid(bs[2 + w], dict(found=int(a["found"][w]), sol_coord=_rows(a["sol"][w]), vec=_rows(a["vec"][w]), norm=_ints(a["norm"][w])))
    assert _untouched(a, SENT, 3)


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_overflowing_lattice_spares_its_neighbours(ctx, route):
    """Lattice 1 of 3 has a row with entries 2^62: status -2 and zero outputs for it, the neighbours as alone."""
    from fplll_amd.gso import MatGSOBatch
    bs, bounds, single = _batch_case(ctx)
    bad = bs[:3].copy()
    bad[1, 5, :] = 0
    bad[1, 5, 3] = 2**62
    bad[1, 5, 64] = 2**62
    g = MatGSOBatch(ctx, 3, 16, 65)
    try:
        g.set_basis(bad)
        found, sol, vec, norm, nodes, st = g.shortest_vectors(6, bound_sq=bounds[:3], route=route)
    finally:
        g.close()
    assert _ints(st) == [1, -2, 1]
    assert int(found[1]) == 0 and not sol[1].any() and not vec[1].any() and not norm[1].any() and int(nodes[1]) == 0
    for k in (0, 2):
        assert int(found[k]) == single[k]["found"] and _ints(norm[k]) == single[k]["norm"]
    from fplll_amd import _lib
    from fplll_amd.svp import shortest_vectors_batch
    with pytest.raises(_lib.HipError, match="lattice 1 .*-2"):
        shortest_vectors_batch(ctx, bad, 6, reduce=False, route=route)


# ---- 4. agreement with shortest_vector --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_one_vector_has_the_norm_of_shortest_vector(ctx, name):
    """K = 1 at the default bound on the recorded q-ary bases: the norm of shortest_vector(route="wave") — and of the
    reference."""
    from fplll_amd.svp import shortest_vector, shortest_vectors
    b = FIXTURES[name]["basis"]
    found, sol, vec, norm = shortest_vectors(ctx, b, 1, reduce=False, route="wave")
    assert found == 1 and int(norm[0]) == shortest_vector(ctx, b, reduce=False, route="wave")[2] == FIXTURES[name]["fast"]["norm"]


# ---- 5. the ENUM route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names("knapsack", "wide"))
def test_enum_route_against_the_exact_list(ctx, name):
    """The K norms are the exact ones (which of several vectors tied at the cut are kept is the parallel walk's)."""
    b = F.basis(name)
    norms3, lst = F.norms_exact(name, 3)
    for K in (5, 64):
        out = _call(ctx, b, K, norms3[2], route="enum")
        assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in lst][:K]
        _valid(b, out)
    ex = F.exact(name)
    out = _call(ctx, b, 4, None, route="enum")
    assert out["norm"][:out["found"]] == [nv for nv, _ in X.short_exact(b, ex["N0"], rows=ex["d_eff"])[0]][:4]


@pytest.mark.parametrize("bound", [3181, 3817])
def test_enum_route_partial_fill_and_shrink(ctx, bound):
    b = FIXTURES["svpsolve_q24_s1"]["basis"]
    want = _exact_q24(bound)
    for K in (8, 64):
        out = _call(ctx, b, K, bound, route="enum")
        assert out["found"] == min(K, len(want)) and out["norm"][:out["found"]] == want[:K]
        _valid(b, out)


def test_enum_route_above_64_rows(ctx):
    """A 72-row steep basis with K = 4 and a bound a sixth above the shortest row (46 vectors within it): the first is
    the hidden b_70 - b_71, which needs the coefficients of the levels >= 64; the norms are short_exact's on the same
    basis.  AUTO above 64 rows is ENUM; the WAVE route declines the object."""
    from fplll_amd.enumeration import Unsupported
    b = F.steep(72)
    N0 = min(sum(v * v for v in r) for r in b)
    bound = N0 + N0 // 6
    want = [nv for nv, _ in X.short_exact(b, bound, max_nodes=F.NODE_CAP)[0]]
    assert len(want) >= 4
    out = _call(ctx, b, 4, bound, route="enum")
    assert out["status"] == 1 and out["norm"] == want[:4]
    _valid(b, out)
    assert any(x[71] != 0 for x in out["sol_coord"])
    assert _call(ctx, b, 4, bound, route="auto")["norm"] == want[:4]  # (AUTO above 64 rows is ENUM)
    with pytest.raises(Unsupported, match="at most 64 rows"):
        _call(ctx, b, 4, bound, route="wave")


# ---- 6. the AUTO route -------------------------------------------------------------------------------------------------
def _gh_nodes(rd, r2):
    """The enumerator's Gaussian-heuristic node estimate (estimate_levels, enum_host.hip) at the squared radius r2."""
    d, tot, sumlog = len(rd), 0.0, 0.0
    for k in range(d - 1, -1, -1):
        sumlog += 0.5 * math.log(rd[k])
        n = d - k
        tot += math.exp(math.log(0.5) + 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1.0) + 0.5 * n * math.log(r2) - sumlog)
    return tot


def test_auto_route_takes_both_routes_in_one_call(ctx, monkeypatch):
    """The mixed batch of the solver tests (easy and hard lattices interleaved, one beyond 63 bits, one with two equal
    rows), lattices [1, 10), K = 3: the estimate at radius N0 separates easy from hard, the limit is set between them;
    the easy lattices carry the kernel's deterministic answers, every good lattice the exact norms, the bad ones
    zeros, and nothing is written behind the range."""
    from fplll_amd.gso import MatGSOBatch
    bs, roles = F.mixed_batch()
    first, count = F.MIXED_FIRST, F.MIXED_COUNT
    est = {}
    for k, role in enumerate(roles):
        if role in ("easy", "hard"):
            _, r = H.gso_exact(bs[k])
            de = X.d_eff_exact(bs[k])
            est[k] = _gh_nodes([float(v) for v in r[:de]], float(min(sum(v * v for v in row) for row in bs[k][:de])))
    lo, hi = max(est[k] for k in est if roles[k] == "easy"), min(est[k] for k in est if roles[k] == "hard")
    assert lo * 1.5 < hi
    monkeypatch.setenv("FPHIP_SVP_WAVE_MAX_NODES", repr(math.sqrt(lo * hi)))
    g = MatGSOBatch(ctx, len(bs), 16, 17)
    try:
        g.set_basis(_np(bs))
        waved = {}
        for k in range(first, first + count):
            if roles[k] in ("easy", "hard"):
                g.shortest_vectors(3, first=k, count=1, route="auto")
                waved[k] = g.last_kernel_ms > 0.0
        assert all(waved[k] == (roles[k] == "easy") for k in waved), waved
        wave = g.shortest_vectors(3, first=first, count=count, route="wave")
        rc, a, SENT = _raw_call(g, first, count, 3, "auto")
        ms = g.last_kernel_ms
    finally:
        g.close()
    assert rc == 0 and ms > 0.0
    for w in range(count):
        k = first + w
        if roles[k] in ("big", "equal"):
            assert int(a["st"][w]) == (-2 if roles[k] == "big" else 0) and int(a["found"][w]) == 0
            assert not a["sol"][w].any() and not a["vec"][w].any() and not a["norm"][w].any() and int(a["nodes"][w]) == 0
            continue
        de = X.d_eff_exact(bs[k])
        N0 = min(sum(v * v for v in row) for row in bs[k][:de])
        want = [nv for nv, _ in X.short_exact(bs[k], N0, rows=de)[0]][:3]
        assert int(a["st"][w]) == 1 and _ints(a["norm"][w])[:int(a["found"][w])] == want
        _valid(bs[k], dict(found=int(a["found"][w]), sol_coord=_rows(a["sol"][w]), vec=_rows(a["vec"][w]), norm=_ints(a["norm"][w])))
        if roles[k] == "easy":  # the kernel's answer, node count included
            assert np.array_equal(a["sol"][w], wave[1][w]) and int(a["nodes"][w]) == int(wave[4][w])
    assert _untouched(a, SENT, count)


# ---- 7. the reference's own N-best -----------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["wave", "enum"])
@pytest.mark.parametrize("path", REF_FIXTURES, ids=lambda f: os.path.basename(f)[:-5])
def test_reference_n_best_norms(ctx, path, route):
    """Both routes return the norms fplll's Enumeration under FastEvaluator(BEST_N) kept."""
    fx = json.load(open(path))
    out = _call(ctx, fx["basis"], fx["max_sols"], fx["bound_sq"], route=route)
    assert out["status"] == 1 and out["found"] == fx["found"] and out["norm"][:out["found"]] == fx["norm"]
    _valid(fx["basis"], out)


def test_reference_fixtures_are_there():
    assert len(REF_FIXTURES) == 6


# ---- 8. the wrappers and the declined calls ---------------------------------------------------------------------------
def test_reduce_on_the_reference_example(ctx):
    """example_svp_in (20 x 21, not reduced) with reduce=True: the first norm is that of example_svp_out, the norms
    are those of short_vectors up to the last of them, and sol_coord is expressed in the CALLER's basis through u."""
    from fplll_amd.svp import short_vectors, shortest_vectors
    txt = open(os.path.join(C.GOLDEN, "example_svp_in.txt")).read().replace("[", " ").replace("]", " ")
    b_in = np.array([int(t) for t in txt.split()], dtype=np.int64).reshape(20, 21)
    txt = open(os.path.join(C.GOLDEN, "example_svp_out.txt")).read().replace("[", " ").replace("]", " ")
    lam1 = sum(int(t) ** 2 for t in txt.split())
    for route in ("wave", "enum", "auto"):
        found, sol, vec, norm = shortest_vectors(ctx, b_in, 8, bound_sq=2 * lam1, route=route)
        assert found >= 1 and int(norm[0]) == lam1
        _valid(b_in, dict(found=found, sol_coord=_rows(sol), vec=_rows(vec), norm=_ints(norm)))
        count, _, _, lnorm = short_vectors(ctx, b_in, 2 * lam1)
        assert _ints(norm[:found]) == _ints(lnorm[:8]) and found == min(8, count)
    found, sol, vec, norm = shortest_vectors(ctx, b_in, 3, route="wave")  # the default bound: the reduced basis' shortest row
    assert found >= 1 and int(norm[0]) == lam1


def test_declined_calls_launch_nothing(ctx):
    """max_sols outside 1 .. 64 and a negative bound: FPHIP_ERROR with a text (the first points to short_vectors);
    SVPM_PROVED, SVP_DUAL, SVP_OVERRIDE_BND, the WAVE route with 65 rows: FPHIP_UNSUPPORTED; a NULL output, a range
    beyond the batch: errors — and not one output is written."""
    from fplll_amd import _lib
    from fplll_amd.enumeration import Unsupported
    from fplll_amd.gso import MatGSOBatch
    bs, _, _ = _batch_case(ctx)
    g = MatGSOBatch(ctx, 2, 16, 65)
    try:
        g.set_basis(bs[:2])
        for K in (0, 65, -3):
            rc, a, SENT = _raw_call(g, 0, 2, max(K, 1), "auto")  # (arrays of a valid size)
            fn = _lib.bind_shortest_vectors(g.lib)
            rc = fn(g.h, None, 0, 2, K, None, 0, 0, None, 0, *(a[k].ctypes.data_as(ctypes.c_void_p) for k in ("found", "sol", "vec", "norm", "nodes", "st")))
            assert rc == _lib.FPHIP_ERROR and "short_vectors" in ctx.last_error()
        rc, a, SENT = _raw_call(g, 0, 2, 4, "wave", bound=[5, -1])
        assert rc == _lib.FPHIP_ERROR and "negative" in ctx.last_error() and _untouched(a, SENT)
        for kw, text in ((dict(method=_lib.SVPM_PROVED), "SVPM_FAST only"), (dict(flags=_lib.SVP_DUAL), "SVP_DUAL"),
                         (dict(flags=_lib.SVP_OVERRIDE_BND), "SVP_OVERRIDE_BND"), (dict(method=1), "SVPM_FAST only")):
            rc, a, SENT = _raw_call(g, 0, 2, 4, "auto", **kw)
            assert rc == _lib.FPHIP_UNSUPPORTED and text in ctx.last_error() and _untouched(a, SENT)
            with pytest.raises(Unsupported, match=text):
                g.shortest_vectors(4, **kw)
        for null in ("found", "sol", "vec", "norm", "nodes", "st"):
            rc, a, SENT = _raw_call(g, 0, 2, 4, "wave", null=null)
            assert rc == _lib.FPHIP_ERROR and "required" in ctx.last_error() and _untouched(a, SENT)
        rc, a, SENT = _raw_call(g, 1, 2, 4, "wave")
        assert rc == _lib.FPHIP_ERROR and "outside the batch" in ctx.last_error()
        with pytest.raises(ValueError, match="short_vectors"):
            g.shortest_vectors(65)
        with pytest.raises(ValueError, match="bound_sq"):
            g.shortest_vectors(4, bound_sq=[1, 2, 3])
    finally:
        g.close()
    g = MatGSOBatch(ctx, 1, 65, 65)
    try:
        g.set_basis(np.eye(65, dtype=np.int64) * 3)
        rc, a, SENT = _raw_call(g, 0, 1, 4, "wave")
        assert rc == _lib.FPHIP_UNSUPPORTED and "at most 64 rows" in ctx.last_error() and _untouched(a, SENT)
    finally:
        g.close()
