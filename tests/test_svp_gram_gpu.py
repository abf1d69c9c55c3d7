"""The N-shortest-vectors solver for quadratic forms on the GPU (fplll_amd.gram.shortest_vectors_gram,
MatGSOGramBatch.shortest_vectors, fphip_gram_shortest_vectors): the WAVE route against the kernel's model
(tests/svp_gram_model.py fed with the device's own mu / r: status, found, norm, sol_coord and nodes bit for bit) and
against the exact rational enumeration of the form (tests/exact_form.py), the batch mechanics of the kernel, the ENUM
route's norms against the exact answers, the AUTO route, the recorded runs of the reference
(tests/golden/svpgram_*.json), the basis solver on B where the form is B B^T, the wrappers and the declined calls."""
import ctypes
import glob
import json
import math
import os

import numpy as np
import pytest

import conftest as C
import exact_form as XF
import exact_lattice as X
import list_helpers as H
import solver_families as F
import svp_gram_cases as BIG
import svp_gram_model as GM

pytestmark = pytest.mark.gpu

REF_FIXTURES = sorted(glob.glob(os.path.join(C.GOLDEN, "svpgram_*.json")))
_cache = {}


def _np(g):
    return np.ascontiguousarray(np.array(g, dtype=object).astype(np.int64))


def _ints(a):
    return [int(v) for v in a]


def _rows(a):
    return [[int(v) for v in r] for r in a]


def gram_of(b):
    return [[sum(int(x) * int(y) for x, y in zip(r, s)) for s in b] for r in b]


def _q24():
    return json.load(open(os.path.join(C.GOLDEN, "svpsolve_q24_s1.json")))["basis"]


def _golden(name):
    return json.load(open(os.path.join(C.GOLDEN, name)))


def _call(ctx, G, K, bound=None, pruning=None, route="wave", want_gso=False, lll=False):
    """One form through MatGSOGramBatch.shortest_vectors: dict(found, sol_coord [K][d], norm [K], nodes, status) and,
    for the model, the form as it stands on the device with the device's own mu / r_ii."""
    from fplll_amd.gram import MatGSOGramBatch
    m = MatGSOGramBatch(ctx, _np(G))
    try:
        if lll:
            assert m.lll()[0][0] == 1
        gso = None
        if want_gso:
            st = int(m.update()[0])
            gso = (_rows(m.gram()[0]), m.mu[0].tolist(), np.diag(m.r[0]).tolist(), st)
        found, sol, norm, nodes, st = m.shortest_vectors(K, bound_sq=bound, pruning=pruning, route=route)
    finally:
        m.close()
    out = dict(found=int(found[0]), sol_coord=_rows(sol[0]), norm=_ints(norm[0]), nodes=int(nodes[0]), status=int(st[0]))
    return (out, gso) if want_gso else out


def _wave_is_the_model(ctx, G, K, bound=None, pruning=None, lll=False):
    out, (Gd, mu, r, ust) = _call(ctx, G, K, bound, pruning, want_gso=True, lll=lll)
    m = GM.solve(Gd, mu, r, K, bound_sq=bound, pruning=pruning, update_status=ust)
    for key in ("status", "found", "norm", "sol_coord", "nodes"):
        assert out[key] == m[key], key
    m["G"] = Gd
    return out, m


def _valid(G, o):
    """Every returned record is distinct modulo +-, non-zero, with x G x^T = norm in Python integers; sorted by norm;
    entries beyond found are zero."""
    seen = set()
    for j in range(len(o["norm"])):
        x, nv = o["sol_coord"][j], o["norm"][j]
        if j >= o["found"]:
            assert not any(x) and nv == 0
            continue
        assert XF.sqnorm(G, x) == nv > 0
        assert j == 0 or o["norm"][j - 1] <= nv
        assert tuple(x) not in seen and tuple(-t for t in x) not in seen
        seen.add(tuple(x))


def _exact_q24(bound):
    if ("q24", bound) not in _cache:
        _cache[("q24", bound)] = [nv for nv, _ in XF.short_exact_form(gram_of(_q24()), bound)[0]]
    return _cache[("q24", bound)]


# ---- 1. the WAVE route is the model, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3])
def test_degenerate_dimensions(ctx, d):
    """d = 1: the multiples of the one variable; d = 2, 3: loops of one and two levels."""
    b = [[7, 2, 1, 0]] if d == 1 else H.lll_exact(np.random.default_rng(d).integers(-30, 31, size=(d, 4)).tolist())
    G = gram_of(b)
    N0 = min(G[i][i] for i in range(d))
    for K, bound in ((4, None), (5, 9 * N0), (2, 100 * N0)):
        out, m = _wave_is_the_model(ctx, G, K, bound)
        _valid(G, out)
        want = [nv for nv, _ in XF.short_exact_form(G, bound or N0, rows=None if bound else m["d_eff"])[0]]
        assert out["status"] == 1 and out["norm"][:out["found"]] == want[:K]
    if d == 1:
        assert _call(ctx, G, 5, 54 * 9)["norm"] == [54, 216, 486, 0, 0]


@pytest.mark.parametrize("d", [63, 64])
def test_lane_edge(ctx, d):
    """Variables up to lane 63 at the third distinct norm, K = 64: records that use the last lane, the LDS triangle at
    d = 64."""
    name = "steep_%d" % d
    G = gram_of(F.basis(name))
    norms3, lst = F.norms_exact(name, 3)
    out, m = _wave_is_the_model(ctx, G, 64, norms3[2])
    assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in lst][:64] and m["d_eff"] == d
    assert any(x[d - 1] != 0 for x in out["sol_coord"][:out["found"]])
    _valid(G, out)


@pytest.mark.parametrize("d", [12, 17, 20])
def test_row_stride_is_not_the_dimension(ctx, d):
    """ldd = 16, 32, 32 with d = 12, 17, 20: a row stride taken for d (or d for the stride) reads other entries."""
    if d == 17:
        b = H.lll_exact(np.random.default_rng(17).integers(-40, 41, size=(17, 19)).tolist())
    else:
        b = F.basis("knap_d%d_b30" % d)
    G = gram_of(b)
    N0 = min(G[i][i] for i in range(d))
    for K, bound in ((8, None), (64, N0 + N0 // 3)):
        out, m = _wave_is_the_model(ctx, G, K, bound)
        want = [nv for nv, _ in XF.short_exact_form(G, bound or m["B0"], rows=None if bound else m["d_eff"], max_nodes=F.NODE_CAP)[0]]
        assert out["status"] == 1 and out["norm"][:out["found"]] == want[:K]
        _valid(G, out)


@pytest.mark.parametrize("bound", [3181, 3817])
@pytest.mark.parametrize("K", [1, 2, 63, 64])
def test_table_sizes_above_and_below_the_number_of_vectors(ctx, K, bound):
    """The form of svpsolve_q24_s1: 26 vectors within 3181 (K = 63, 64 never fill; K = 1, 2 do) and 233 within 3817
    (every K fills and shrinks)."""
    G = gram_of(_q24())
    out, m = _wave_is_the_model(ctx, G, K, bound)
    want = _exact_q24(bound)
    assert len(want) == (26 if bound == 3181 else 233)
    assert out["found"] == min(K, len(want)) and out["norm"][:out["found"]] == want[:K]
    _valid(G, out)


@pytest.mark.parametrize("which", ["dim7", "dim4"])
def test_the_references_two_forms_after_the_gram_lll(ctx, which):
    f = _golden("svpgram_%s_k64.json" % which)
    for K, bound in ((1, None), (8, None), (64, None), (64, 4)):
        out, m = _wave_is_the_model(ctx, f["G_in"], K, bound, lll=True)
        _valid(m["G"], out)
        assert out["status"] == 1 and out["norm"][0] == XF.sqnorm(f["G_in"], f["ref_out"])
    shells = {}
    for nv in out["norm"][:out["found"]]:
        shells[nv] = shells.get(nv, 0) + 1
    assert shells == ({3: 28, 4: 36} if which == "dim7" else {2: 12, 4: 12})


def test_known_shells(ctx):
    """Gram of Z^8 (reduced): K = 8 keeps the eight of norm 1 and stops, K = 16 finds 8, bound 2 with K = 64 fills on
    the last vector; D4: twelve of norm 2, five, and 12 + 12 within 4; 2 E8: 64 of the 120 of norm 8."""
    z8 = gram_of(H.lll_exact(H.z8_basis()))
    assert _wave_is_the_model(ctx, z8, 8)[0]["norm"] == [1] * 8
    assert _wave_is_the_model(ctx, z8, 16)[0]["found"] == 8
    out, m = _wave_is_the_model(ctx, z8, 64, 2)
    assert out["norm"] == [1] * 8 + [2] * 56 and m["insertions"] == 64
    d4 = gram_of(H.d4_basis())
    assert _wave_is_the_model(ctx, d4, 12)[0]["norm"] == [2] * 12
    assert _wave_is_the_model(ctx, d4, 5)[0]["norm"] == [2] * 5
    for K in (24, 64):
        out, _ = _wave_is_the_model(ctx, d4, K, 4)
        assert out["found"] == 24 and out["norm"][:24] == [2] * 12 + [4] * 12
    e8 = gram_of(H.lll_exact(H.e8_basis()[0]))
    out, _ = _wave_is_the_model(ctx, e8, 64)
    assert out["norm"] == [8] * 64
    _valid(e8, out)


def test_the_form_that_is_no_gram_matrix_of_an_integer_basis(ctx):
    f = _golden("lllgram_form_nobasis.json")
    G = f["G_out"]
    rn = sorted(G[i][i] for i in range(7))
    for K in (1, 5, 64):
        for bound in (None, rn[2], rn[-1]):
            out, m = _wave_is_the_model(ctx, G, K, bound)
            want = [nv for nv, _ in XF.short_exact_form(G, bound or m["B0"], rows=None if bound else m["d_eff"])[0]]
            assert out["status"] == 1 and out["found"] == min(K, len(want)) and out["norm"][:out["found"]] == want[:K]
            _valid(G, out)
    # from the unreduced form, through the Gram LLL: the same norms
    out, m = _wave_is_the_model(ctx, f["G_in"], 5, rn[-1], lll=True)
    assert m["G"] == f["G_out"] and out["norm"][:out["found"]] == want[:5]


@pytest.mark.parametrize("name", F.PRUNED)
def test_pruned_walk(ctx, name):
    """The level bound is pruning[k] * radius, also after the radius shrinks; found may stay below K."""
    G = gram_of(F.basis(name))
    norms3, _ = F.norms_exact(name, 3)
    out, _ = _wave_is_the_model(ctx, G, 5, norms3[2], pruning=F.pruning_of(name))
    _valid(G, out)
    _wave_is_the_model(ctx, G, 3, None, pruning=F.pruning_of(name))


def test_pruning_can_leave_nothing(ctx):
    out, _ = _wave_is_the_model(ctx, gram_of(H.d4_basis()), 4, pruning=[0.01] * 4)
    assert out["status"] == 1 and out["found"] == 0 and out["norm"] == [0] * 4


@pytest.mark.parametrize("name", F.names("cut_rows"))
def test_rows_cut_with_and_without_a_callers_bound(ctx, name):
    b = F.basis(name)
    G = gram_of(b)
    ex = F.exact(name)
    out, m = _wave_is_the_model(ctx, G, 8, None)
    assert m["d_eff"] == ex["d_eff"] and m["B0"] == ex["N0"]
    assert out["norm"][:out["found"]] == [nv for nv, _ in XF.short_exact_form(G, ex["N0"], rows=ex["d_eff"])[0]][:8]
    norms3, lst = F.norms_exact(name, 3)
    out, m = _wave_is_the_model(ctx, G, 64, norms3[2])
    assert out["norm"][:out["found"]] == [nv for nv, _ in lst][:64]
    _valid(G, out)


# ---- 2. the WAVE route against the exact answers ----------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names("scaled_root"))
def test_scaled_roots_against_the_exact_list(ctx, name):
    """Entries up to 2^61 with near-tied minima, K = 5 at the third distinct norm: status 1 and the five smallest exact
    norms.  (The sums of these forms stay within 63 bits; test_partial_sums_beyond_63_bits has the wide ones.)"""
    G = gram_of(F.basis(name))
    norms3, lst = F.norms_exact(name, 3)
    out, _ = _wave_is_the_model(ctx, G, 5, norms3[2])
    assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in lst][:5]
    _valid(G, out)


@pytest.mark.parametrize("route", ["wave", "enum"])
@pytest.mark.parametrize("name", sorted(BIG.CASES))
def test_partial_sums_beyond_63_bits(ctx, name, route):
    """tests/svp_gram_cases.py: prefixes of y_j = sum_i x_i g_ij of 2^63 and more, products x_j y_j likewise, the value
    within 63 bits.  WAVE: the model bit for bit, status 1; ENUM (the host callback's 128 bits): the exact norms."""
    G, bound, K = BIG.case(name)
    want = [nv for nv, _ in XF.short_exact_form(G, bound, max_nodes=F.NODE_CAP)[0]]
    out = _wave_is_the_model(ctx, G, K, bound)[0] if route == "wave" else _call(ctx, G, K, bound, route="enum")
    assert out["status"] == 1 and out["found"] == min(K, len(want)) > 0 and out["norm"][:out["found"]] == want[:K]
    _valid(G, out)
    prefix, term = BIG.partial_bits(G, out["sol_coord"][:out["found"]])
    assert prefix >= 64 and (term >= 64 or K == 4), (prefix, term)


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_a_value_beyond_63_bits_behind_wide_sums(ctx, route):
    """2^56 [[64, 24], [24, 10]]: thirteen vectors within 64 2^56, the last with prefixes of 3 2^62; under the bound
    2^63 - 1 a candidate's value itself is beyond 63 bits: status -2."""
    s2 = 2**56
    G = [[64 * s2, 24 * s2], [24 * s2, 10 * s2]]
    out = _call(ctx, G, 64, 64 * s2, route=route)
    assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in XF.short_exact_form(G, 64 * s2)[0]]
    assert out["found"] == 13 and BIG.partial_bits(G, out["sol_coord"][:13])[0] >= 64
    out = _call(ctx, G, 64, 2**63 - 1, route=route)
    assert out["status"] == -2 and out["found"] == 0 and out["nodes"] == 0 and not any(out["norm"])


# ---- 3. batch mechanics -----------------------------------------------------------------------------------------------
def _batch_case(ctx):
    """19 forms of 16 variables (A A^T of 16 x 20 integers, reduced by the batched Gram LLL), their per-form bounds (the
    default, B0 + B0 / 8 and B0 + B0 / 3 in turn: mixed `found` under a table of K = 6) and their one-form results."""
    from fplll_amd.gram import MatGSOGramBatch
    if "batch" not in _cache:
        gs = []
        for s in range(19):
            a = np.random.default_rng(1600 + s).integers(-60, 61, size=(16, 20))
            gs.append(a @ a.T)
        m = MatGSOGramBatch(ctx, np.stack(gs))
        try:
            st, _ = m.lll()
            assert (st == 1).all()
            gs = m.gram()
        finally:
            m.close()
        bounds = []
        for k in range(19):
            B0 = int(min(np.diag(gs[k])))
            bounds.append((0, B0 + B0 // 8, B0 + B0 // 3)[k % 3])
        single = [_call(ctx, gs[k], 6, bounds[k] or None) for k in range(19)]
        _cache["batch"] = (gs, bounds, single)
    return _cache["batch"]


def _same_as_single(arrs, w, s1):
    found, sol, norm, nodes, st = arrs
    assert int(st[w]) == s1["status"] and int(found[w]) == s1["found"] and _ints(norm[w]) == s1["norm"]
    assert _rows(sol[w]) == s1["sol_coord"] and int(nodes[w]) == s1["nodes"]


@pytest.mark.parametrize("count", [1, 5, 19])
def test_batches_equal_single_runs(ctx, count, monkeypatch):
    """1, 5 and 2 * 8 + 3 forms on a grid of two workgroups of four waves (FPHIP_SVP_WAVE_GRID=2), per-form bounds,
    mixed found; two calls give identical arrays.  Catches: LDS or table state shared between waves or kept across the
    grid-stride loop, the bound indexed by the form, records written into a neighbour's slots."""
    from fplll_amd.gram import MatGSOGramBatch
    gs, bounds, single = _batch_case(ctx)
    assert len({s["found"] for s in single}) > 1
    for k in (1, 7, 17):  # (forms with a caller's bound: every row is within it or cut soundly)
        _valid(_rows(gs[k]), single[k])
        want = [nv for nv, _ in XF.short_exact_form(_rows(gs[k]), bounds[k], max_nodes=F.NODE_CAP)[0]]
        assert bounds[k] and single[k]["norm"][:single[k]["found"]] == want[:6]
    monkeypatch.setenv("FPHIP_SVP_WAVE_GRID", "2")
    m = MatGSOGramBatch(ctx, gs[:count])
    try:
        arrs = m.shortest_vectors(6, bound_sq=bounds[:count], route="wave")
        ms = m.last_kernel_ms
        again = m.shortest_vectors(6, bound_sq=bounds[:count], route="wave")
    finally:
        m.close()
    assert ms > 0.0
    for k in range(count):
        _same_as_single(arrs, k, single[k])
    for a, b in zip(arrs, again):
        assert np.array_equal(a, b)


def _raw_call(m, first, count, K, route, guard=2, bound=None, method=0, flags=0, null=None, pruning=None):
    """fphip_gram_shortest_vectors with `guard` forms of sentinel behind the count forms of every output array."""
    from fplll_amd import _lib
    fn = _lib.bind_gram_shortest_vectors(m.lib)
    SENT = -77
    n = count + guard
    arrs = dict(found=np.full(n, SENT, dtype=np.int32), sol=np.full((n, K, m.d), SENT, dtype=np.int64),
                norm=np.full((n, K), SENT, dtype=np.int64), nodes=np.full(n, 77, dtype=np.uint64),
                st=np.full(n, SENT, dtype=np.int32))
    ptr = {k: (None if k == null else v.ctypes.data_as(ctypes.c_void_p)) for k, v in arrs.items()}
    bd = None if bound is None else np.ascontiguousarray(bound, dtype=np.int64)
    pr = None if pruning is None else np.ascontiguousarray(pruning, dtype=np.float64)
    rc = fn(m.h, None, first, count, K, None if bd is None else bd.ctypes.data_as(ctypes.c_void_p), method, flags,
            None if pr is None else pr.ctypes.data_as(ctypes.c_void_p), _lib.SVP_ROUTES[route], ptr["found"], ptr["sol"],
            ptr["norm"], ptr["nodes"], ptr["st"])
    return rc, arrs, SENT


def _untouched(a, SENT, start=0):
    return all((v[start:] == (77 if k == "nodes" else SENT)).all() for k, v in a.items())


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_sub_range_leaves_the_rest_untouched(ctx, route):
    """first_form = 2, count = 3 of a batch of 7: the outputs are those of forms 2, 3, 4 in places 0, 1, 2 with THEIR
    bounds (bound_sq is indexed by the place in the range), and nothing is written behind them."""
    from fplll_amd.gram import MatGSOGramBatch
    gs, bounds, single = _batch_case(ctx)
    m = MatGSOGramBatch(ctx, gs[:7])
    try:
        rc, a, SENT = _raw_call(m, 2, 3, 6, route, bound=bounds[2:5])
    finally:
        m.close()
    assert rc == 0
    for w in range(3):
        s1 = single[2 + w]
        assert int(a["st"][w]) == 1 and int(a["found"][w]) == s1["found"] and _ints(a["norm"][w]) == s1["norm"]
        if route == "wave":
            assert _rows(a["sol"][w]) == s1["sol_coord"] and int(a["nodes"][w]) == s1["nodes"]
        _valid(_rows(gs[2 + w]), dict(found=int(a["found"][w]), sol_coord=_rows(a["sol"][w]), norm=_ints(a["norm"][w])))
    assert _untouched(a, SENT, 3)


@pytest.mark.parametrize("route", ["wave", "enum"])
def test_a_form_beyond_63_bits_spares_its_neighbours(ctx, route):
    """[[2^62, 0], [0, 2^62]] with the bound 2^63 - 1 between two small forms: its candidate (1, 1) has the value 2^63 —
    status -2 and zero outputs for it, the neighbours as alone."""
    from fplll_amd import _lib
    from fplll_amd.gram import MatGSOGramBatch, shortest_vectors_gram
    gs = [[[2, 1], [1, 3]], [[2**62, 0], [0, 2**62]], [[5, 2], [2, 7]]]
    bounds = [0, 2**63 - 1, 30]
    alone = [_call(ctx, gs[k], 4, bounds[k] or None, route=route) for k in (0, 2)]
    m = MatGSOGramBatch(ctx, _np(gs))
    try:
        found, sol, norm, nodes, st = m.shortest_vectors(4, bound_sq=bounds, route=route)
    finally:
        m.close()
    assert _ints(st) == [1, -2, 1]
    assert int(found[1]) == 0 and not sol[1].any() and not norm[1].any() and int(nodes[1]) == 0
    for k, s1 in zip((0, 2), alone):
        assert int(found[k]) == s1["found"] and _ints(norm[k]) == s1["norm"] and _rows(sol[k]) == s1["sol_coord"]
        want = [nv for nv, _ in XF.short_exact_form(gs[k], bounds[k] or min(gs[k][0][0], gs[k][1][1]))[0]]
        assert s1["norm"][:s1["found"]] == want[:4]
    with pytest.raises(_lib.HipError, match="form 1 .*-2"):
        shortest_vectors_gram(ctx, _np(gs), 4, bound_sq=bounds, reduce=False, route=route)
    # the same form below its limit answers
    assert _call(ctx, gs[1], 4, route=route)["norm"] == [2**62, 2**62, 0, 0]


@pytest.mark.parametrize("route", ["wave", "enum", "auto"])
def test_a_semidefinite_form_spares_its_neighbours(ctx, route):
    """The Gram matrix of lllgram_rankdef's input (two equal rows: rank 7 of 8) between the forms of Z^8 and 2 E8: status
    0 and zero outputs for it, the neighbours as alone."""
    from fplll_amd.gram import MatGSOGramBatch
    bad = _golden("lllgram_rankdef.json")["G_in"]
    gs = [gram_of(H.lll_exact(H.z8_basis())), bad, gram_of(H.lll_exact(H.e8_basis()[0]))]
    m = MatGSOGramBatch(ctx, _np(gs))
    try:
        found, sol, norm, nodes, st = m.shortest_vectors(8, route=route)
    finally:
        m.close()
    assert _ints(st) == [1, 0, 1]
    assert int(found[1]) == 0 and not sol[1].any() and not norm[1].any() and int(nodes[1]) == 0
    assert _ints(norm[0]) == [1] * 8 and _ints(norm[2]) == [8] * 8
    if route == "wave":
        for k in (0, 2):
            _same_as_single((found, sol, norm, nodes, st), k, _call(ctx, gs[k], 8))


# ---- 4. the ENUM route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names("knapsack", "wide"))
def test_enum_route_against_the_exact_list(ctx, name):
    """The K norms are the exact ones (which of several vectors tied at the cut are kept is the parallel walk's)."""
    G = gram_of(F.basis(name))
    norms3, lst = F.norms_exact(name, 3)
    for K in (5, 64):
        out = _call(ctx, G, K, norms3[2], route="enum")
        assert out["status"] == 1 and out["norm"][:out["found"]] == [nv for nv, _ in lst][:K]
        _valid(G, out)
    ex = F.exact(name)
    out = _call(ctx, G, 4, None, route="enum")
    assert out["norm"][:out["found"]] == [nv for nv, _ in XF.short_exact_form(G, ex["N0"], rows=ex["d_eff"])[0]][:4]


@pytest.mark.parametrize("bound", [3181, 3817])
def test_enum_route_partial_fill_and_shrink(ctx, bound):
    G = gram_of(_q24())
    want = _exact_q24(bound)
    for K in (8, 64):
        out = _call(ctx, G, K, bound, route="enum")
        assert out["found"] == min(K, len(want)) and out["norm"][:out["found"]] == want[:K]
        _valid(G, out)


def test_enum_route_above_64_rows(ctx):
    """The form of the 72-row steep basis with K = 4 and a bound a sixth above the smallest diagonal entry: the first
    vector needs the coefficients of the levels >= 64; ENUM and AUTO return the exact four norms, WAVE declines."""
    from fplll_amd.enumeration import Unsupported
    b = F.steep(72)
    G = gram_of(b)
    N0 = min(G[i][i] for i in range(72))
    bound = N0 + N0 // 6
    want = [nv for nv, _ in X.short_exact(b, bound, max_nodes=F.NODE_CAP)[0]]
    assert len(want) >= 4
    out = _call(ctx, G, 4, bound, route="enum")
    assert out["status"] == 1 and out["norm"] == want[:4]
    _valid(G, out)
    assert any(x[71] != 0 for x in out["sol_coord"])
    assert _call(ctx, G, 4, bound, route="auto")["norm"] == want[:4]  # (AUTO above 64 rows is ENUM)
    with pytest.raises(Unsupported, match="at most 64 rows"):
        _call(ctx, G, 4, bound, route="wave")


# ---- 5. the AUTO route -------------------------------------------------------------------------------------------------
def _gh_nodes(rd, r2):
    """The enumerator's Gaussian-heuristic node estimate (estimate_levels, enum_host.hip) at the squared radius r2."""
    d, tot, sumlog = len(rd), 0.0, 0.0
    for k in range(d - 1, -1, -1):
        sumlog += 0.5 * math.log(rd[k])
        n = d - k
        tot += math.exp(math.log(0.5) + 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1.0) + 0.5 * n * math.log(r2) - sumlog)
    return tot


def test_auto_route_takes_both_routes_in_one_call(ctx, monkeypatch):
    """The forms of the mixed batch of the solver tests (easy and hard interleaved), forms [1, 10), K = 3: the estimate
    at radius B0 separates easy from hard, the limit is set between them; the easy forms carry the kernel's
    deterministic answers, every good form the exact norms, the bad ones zeros, and nothing is written behind the
    range.  The bad ones: in place of the basis with entries of 2^62 (its Gram matrix is beyond int64) the form 2^62 I
    under the bound 2^63 - 1 (status -2); the basis with two equal rows gives a semidefinite form (status 0)."""
    from fplll_amd.gram import MatGSOGramBatch
    bs, roles = F.mixed_batch()
    first, count = F.MIXED_FIRST, F.MIXED_COUNT
    gs = [[[(2**62) * int(i == j) for j in range(16)] for i in range(16)] if role == "big" else gram_of(b)
          for b, role in zip(bs, roles)]
    bounds = [2**63 - 1 if role == "big" else 0 for role in roles]
    est = {}
    for k, role in enumerate(roles):
        if role in ("easy", "hard"):
            _, r = H.gso_exact(bs[k])
            de = X.d_eff_exact(bs[k])
            est[k] = _gh_nodes([float(v) for v in r[:de]], float(min(gs[k][i][i] for i in range(de))))
    lo, hi = max(est[k] for k in est if roles[k] == "easy"), min(est[k] for k in est if roles[k] == "hard")
    assert lo * 1.5 < hi
    monkeypatch.setenv("FPHIP_SVP_WAVE_MAX_NODES", repr(math.sqrt(lo * hi)))
    m = MatGSOGramBatch(ctx, _np(gs))
    try:
        waved = {}
        for k in range(first, first + count):
            if roles[k] in ("easy", "hard"):
                m.shortest_vectors(3, first=k, count=1, route="auto")
                waved[k] = m.last_kernel_ms > 0.0
        assert all(waved[k] == (roles[k] == "easy") for k in waved), waved
        wave = m.shortest_vectors(3, first=first, count=count, bound_sq=bounds[first:first + count], route="wave")
        rc, a, SENT = _raw_call(m, first, count, 3, "auto", bound=bounds[first:first + count])
        ms = m.last_kernel_ms
    finally:
        m.close()
    assert rc == 0 and ms > 0.0
    for w in range(count):
        k = first + w
        if roles[k] in ("big", "equal"):
            assert int(a["st"][w]) == (-2 if roles[k] == "big" else 0) and int(a["found"][w]) == 0
            assert not a["sol"][w].any() and not a["norm"][w].any() and int(a["nodes"][w]) == 0
            continue
        de = X.d_eff_exact(bs[k])
        N0 = min(gs[k][i][i] for i in range(de))
        want = [nv for nv, _ in XF.short_exact_form(gs[k], N0, rows=de)[0]][:3]
        assert int(a["st"][w]) == 1 and _ints(a["norm"][w])[:int(a["found"][w])] == want
        _valid(gs[k], dict(found=int(a["found"][w]), sol_coord=_rows(a["sol"][w]), norm=_ints(a["norm"][w])))
        if roles[k] == "easy":  # the kernel's answer, node count included
            assert np.array_equal(a["sol"][w], wave[1][w]) and int(a["nodes"][w]) == int(wave[3][w])
    assert _untouched(a, SENT, count)


# ---- 6. the reference's own answers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["wave", "enum"])
@pytest.mark.parametrize("path", REF_FIXTURES, ids=lambda f: os.path.basename(f)[:-5])
def test_reference_norms(ctx, path, route):
    """Both routes return the norms fplll's shortest_vectors(MatGSOGram, ..., max_sols) kept, on its reduced form."""
    fx = json.load(open(path))
    out = _call(ctx, fx["G"], fx["max_sols"], route=route)
    assert out["status"] == 1 and out["found"] == fx["found"] and out["norm"][:out["found"]] == fx["norm"]
    assert out["norm"][0] == fx["sv_norm"]
    _valid(fx["G"], out)


def test_reference_fixtures_are_there():
    assert len(REF_FIXTURES) == 8


# ---- 7. the basis solver on B where the form is B B^T ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["knap_d16_b40", "root_e8_s29_x2_0", "cut_scaled", "wide_n65", "steep_63"])
def test_norms_are_those_of_the_basis_solver(ctx, name):
    from fplll_amd.gso import MatGSOBatch
    b = F.basis(name)
    norms3, _ = F.norms_exact(name, 3)
    for K, bound in ((5, None), (64, norms3[2])):
        g = MatGSOBatch(ctx, 1, len(b), len(b[0]), row_expo=False)
        try:
            g.set_basis(_np(b))
            found, _, _, norm, _, st = g.shortest_vectors(K, bound_sq=bound, route="wave")
        finally:
            g.close()
        out = _call(ctx, gram_of(b), K, bound)
        assert int(st[0]) == out["status"] == 1 and int(found[0]) == out["found"] and _ints(norm[0]) == out["norm"]


# ---- 8. the wrappers and the declined calls ---------------------------------------------------------------------------
def test_wrappers_on_the_references_unreduced_form(ctx):
    from fplll_amd.gram import shortest_vector_gram, shortest_vectors_gram, sqnorm_coordinates
    G_in = _golden("svpgram_dim7_k8.json")["G_in"]
    for route in ("wave", "enum", "auto"):
        sol, norm = shortest_vector_gram(ctx, G_in, reduce=True, route=route)
        assert norm == 3 and sqnorm_coordinates(G_in, sol) == 3
        found, sols, norms = shortest_vectors_gram(ctx, G_in, 64, bound_sq=4, route=route)
        assert found == 64 and _ints(norms) == [3] * 28 + [4] * 36
        for x, nv in zip(sols, norms):
            assert sqnorm_coordinates(G_in, x) == int(nv)
        assert len({tuple(_ints(x)) for x in sols} | {tuple(-v for v in _ints(x)) for x in sols}) == 128
    # a batch of two: the dimension-7 form twice, the second permuted
    p = [6, 5, 4, 3, 2, 1, 0]
    G2 = [[G_in[p[i]][p[j]] for j in range(7)] for i in range(7)]
    sol, norm = shortest_vector_gram(ctx, [G_in, G2])
    assert _ints(norm) == [3, 3] and sqnorm_coordinates(G2, sol[1]) == 3 and sqnorm_coordinates(G_in, sol[0]) == 3


def test_reduction_failures_are_named(ctx):
    from fplll_amd import _lib
    from fplll_amd.gram import shortest_vectors_gram
    bad = _golden("lllgram_rankdef.json")["G_in"]
    good = gram_of(H.lll_exact(H.z8_basis()))
    with pytest.raises(_lib.HipError, match="form 1 "):
        shortest_vectors_gram(ctx, [good, bad], 4, reduce=False)


def test_declined_calls_launch_nothing(ctx):
    """max_sols outside 1 .. 64, a negative bound, a NULL output, a range beyond the batch, a bad pruning coefficient:
    FPHIP_ERROR with a text; SVPM_PROVED, SVP_DUAL, SVP_OVERRIDE_BND, the WAVE route with 65 variables:
    FPHIP_UNSUPPORTED — and not one output is written."""
    from fplll_amd import _lib
    from fplll_amd.enumeration import Unsupported
    from fplll_amd.gram import MatGSOGramBatch
    gs, _, _ = _batch_case(ctx)
    m = MatGSOGramBatch(ctx, gs[:2])
    try:
        for K in (0, 65, -3):
            rc, a, SENT = _raw_call(m, 0, 2, max(K, 1), "auto")  # (arrays of a valid size, written by a valid call ...)
            for k, v in a.items():  # (... and set back to the sentinels)
                v[...] = 77 if k == "nodes" else SENT
            fn = _lib.bind_gram_shortest_vectors(m.lib)
            rc = fn(m.h, None, 0, 2, K, None, 0, 0, None, 0, *(a[k].ctypes.data_as(ctypes.c_void_p) for k in ("found", "sol", "norm", "nodes", "st")))
            assert rc == _lib.FPHIP_ERROR and "outside 1 .. 64" in ctx.last_error() and _untouched(a, SENT)
        rc, a, SENT = _raw_call(m, 0, 2, 4, "wave", bound=[5, -1])
        assert rc == _lib.FPHIP_ERROR and "negative" in ctx.last_error() and _untouched(a, SENT)
        for kw, text in ((dict(method=_lib.SVPM_PROVED), "SVPM_FAST only"), (dict(flags=_lib.SVP_DUAL), "SVP_DUAL"),
                         (dict(flags=_lib.SVP_OVERRIDE_BND), "SVP_OVERRIDE_BND"), (dict(method=1), "SVPM_FAST only")):
            rc, a, SENT = _raw_call(m, 0, 2, 4, "auto", **kw)
            assert rc == _lib.FPHIP_UNSUPPORTED and text in ctx.last_error() and _untouched(a, SENT)
            with pytest.raises(Unsupported, match=text):
                m.shortest_vectors(4, **kw)
        for null in ("found", "sol", "norm", "nodes", "st"):
            rc, a, SENT = _raw_call(m, 0, 2, 4, "wave", null=null)
            assert rc == _lib.FPHIP_ERROR and "required" in ctx.last_error() and _untouched(a, SENT)
        rc, a, SENT = _raw_call(m, 1, 2, 4, "wave")
        assert rc == _lib.FPHIP_ERROR and "outside the batch" in ctx.last_error() and _untouched(a, SENT)
        for badp in (0.0, -1.0, float("inf"), float("nan")):
            rc, a, SENT = _raw_call(m, 0, 2, 4, "wave", pruning=[1.0] * 15 + [badp])
            assert rc == _lib.FPHIP_ERROR and "pruning coefficient" in ctx.last_error() and _untouched(a, SENT)
        with pytest.raises(ValueError, match="max_sols"):
            m.shortest_vectors(65)
        with pytest.raises(ValueError, match="bound_sq"):
            m.shortest_vectors(4, bound_sq=[1, 2, 3])
    finally:
        m.close()
    m = MatGSOGramBatch(ctx, np.eye(65, dtype=np.int64) * 3)
    try:
        rc, a, SENT = _raw_call(m, 0, 1, 4, "wave")
        assert rc == _lib.FPHIP_UNSUPPORTED and "at most 64 rows" in ctx.last_error() and _untouched(a, SENT)
    finally:
        m.close()
