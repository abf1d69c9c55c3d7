"""Exact ties on the GPU: the enumeration kernels on blocks where centres ARE integers and half-integers, siblings tie
and distances equal their bounds (tests/exact_enum.py; sizes and tie counts of the named blocks: the table in
tests/test_enum_exact_ties_cpu.py), against the exact rational reference exact_enum.exact_enumerate — or, where the
tree is above 3 10^4 nodes, the block has more than 64 rows or the call is dual, against the C oracle, which equals the
exact reference on every named block (test_enum_exact_ties_cpu.py).

What rests on ties in the kernels: the 64 candidates of a node of enum_walk.hip have non-decreasing distances and the
survivors are counted from the ballot of `dist_j <= bound`; the first step's direction is `c >= x_0` again; roundto of
a half-integer centre; reprune when the bound drops onto the distance of pending siblings; the coefficients a chain
link did not store are roundto(centre) again; the first child's distance without the crossbar; the zig-zag rank of
enum_order.h.  The inputs are dyadic, all arithmetic on them is exact in double: every comparison here is `==`."""
from fractions import Fraction

import pytest

import conftest as C
import exact_enum as E

pytestmark = pytest.mark.gpu

ALL_BLOCKS = dict(E.TIE_BLOCKS, **E.ORACLE_ONLY_BLOCKS)
EVALUATORS = [(1, 0), (5, 0), (3, 1), (1, 2)]  # (1, BEST), (5, BEST), (3, OPPORTUNISTIC), (1, FIRST)
MU_LDS = dict(FPHIP_MU_GLOBAL_MIN_TASKS="1000000000", FPHIP_MU_GLOBAL_MIN_LEVEL="1000")  # (test_enum_walk3_gpu.py's)
MU_GLOBAL = dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0")
SWITCHES = {
    "walk3=0": dict(FPHIP_WALK3="0"), "walk3=1": dict(FPHIP_WALK3="1"), "walk2=0": dict(FPHIP_WALK2="0"),
    "bfs=0": dict(FPHIP_BFS="0"), "mu_lds": MU_LDS, "mu_global": MU_GLOBAL,
    "walk3=0,mu_global": dict(FPHIP_WALK3="0", **MU_GLOBAL), "budget=64": dict(FPHIP_BUDGET="64"),
    "walk3=0,budget=64": dict(FPHIP_WALK3="0", FPHIP_BUDGET="64"),
}

_fixed_cache = {}


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _sorted_bits(log):
    return _bits(sorted((a, tuple(b)) for a, b in log))


def _reference(name):
    """(mut, rdiag, pruning, R, nodes, sorted candidates) of a named block at a radius that never shrinks: the exact
    reference up to 3 10^4 nodes, the C oracle above.  Computed once per process, read-only."""
    if name not in _fixed_cache:
        mut, rdiag, pruning, R = ALL_BLOCKS[name]()
        if name in E.TIE_BLOCKS:
            nodes, cands, _ = E.exact_of(name)
        else:
            nodes, cands = _oracle(mut, rdiag, pruning, R)
            assert sum(nodes) > 30000
        _fixed_cache[name] = (mut, rdiag, pruning, R, nodes, cands)
    return _fixed_cache[name]


def _oracle(mut, rdiag, pruning, R, **kw):
    from fplll_amd.enumeration import FastEvaluator
    log = []
    nodes, _ = C.oracle_enumerate(mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log, **kw)
    return [int(v) for v in nodes], sorted((a, tuple(b)) for a, b in log)


def _device(ctx, mut, rdiag, pruning, R, **kw):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    log = []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log=log, **kw)
    return [int(v) for v in res.nodes], log


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", list(ALL_BLOCKS))
def test_fixed_radius_counts_and_candidates_are_exact(ctx, monkeypatch, name, switch):
    """Radius that never shrinks, default mode: per-level counts and the multiset of candidates (distance and all
    coefficients, bit for bit) under both generations of the walk, the first-generation kernel, split launches instead
    of the breadth-first stage, mu in LDS and through the buffer loads, and a donation budget so small that the
    prefixes of donated tasks replay roundto(centre) on tie centres."""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _reference(name)
    nodes, log = _device(ctx, mut, rdiag, pruning, R)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk3", ["0", "1"])
@pytest.mark.parametrize("d,fat,seed,R", [(9, 2, 5, 1.5), (10, 5, 6, 1.5), (8, 1, 5, 1.5)])
def test_more_than_63_children_with_exact_ties(ctx, monkeypatch, walk3, d, fat, seed, R):
    """exact_enum.fat_level_block: every node of level `fat` has centre 0, r = 2^-12: up to 91 children, +-z of equal
    distance across the boundary between the 63 candidates of one ballot and the rest.  Fat level 1, 2: inside the walk;
    5: inside the breadth-first stage.  Counts and candidates are the oracle's AND the exact reference's."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag = E.fat_level_block(d, fat, seed)
    nodes_o, cands_o = _oracle(mut, rdiag, None, R)
    nodes_e, cands_e, stats = E.exact_enumerate(mut, rdiag, None, R, max_nodes=30000)
    assert nodes_e == nodes_o and _bits(cands_e) == _bits(cands_o)
    assert stats["max_children"] > 63  # (91: the zig-zag passes the 63rd candidate between +z and -z, z = 32)
    nodes, log = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk3", ["0", "1"])
def test_above_64_rows(ctx, monkeypatch, walk3):
    """exact_enum.wide_dyadic_block, 72 rows: the rows >= 40 have centre 0 (children +-1 tie), candidates sit under a
    level-64 ancestor with non-zero coefficients; the top walk and the subtree kernel against the C oracle."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag, R = E.wide_dyadic_block(72, 40, 9, 1.25)
    nodes_o, cands_o = _oracle(mut, rdiag, None, R)
    assert sum(nodes_o[64:]) > 0 and len(cands_o) >= 10
    assert any(any(v != 0.0 for v in x[64:]) for _, x in cands_o)
    assert len(set(a for a, _ in cands_o)) < len(cands_o)
    nodes, log = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk3", ["0", "1"])
@pytest.mark.parametrize("name", ["dy12", "dy20", "pr28", "q2"])
def test_dual_on_the_dyadic_inputs(ctx, monkeypatch, name, walk3):
    """The same inputs through the dual recursion (centres driven by alpha = x - c: multiples of 1/q^depth, the
    arithmetic is no longer exact and the walk is another one) against the oracle's dualenum walk."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    nodes_o, cands_o = _oracle(mut, rdiag, pruning, R, dual=True)
    assert len(cands_o) >= 3
    nodes, log = _device(ctx, mut, rdiag, pruning, R, dual=True)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk3", ["0", "1"])
@pytest.mark.parametrize("nsol", [1, 5])
@pytest.mark.parametrize("name", list(E.TIE_BLOCKS))
def test_shrinking_radius_default_mode(ctx, monkeypatch, name, nsol, walk3):
    """BEST_N in the default mode (the order is a race: logs are not compared).  The bound drops ONTO the distances of
    pending siblings and of whole groups of candidates.  By exact_enum.best_n_guarantee every walk order must end with
    the exact reference's nsol-th smallest candidate distance as the bound and the head of that multiset kept (checked
    as a precondition: also on the pruned block the candidates concerned pass every pruning bound under the final
    radius); every logged candidate is a member of the exact candidate set."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag, pruning, R, _, cands = _reference(name)
    m, final_fixed, head_fixed = E.best_n_guarantee(mut, rdiag, pruning, cands, nsol)
    assert final_fixed and head_fixed, "the block no longer fixes the result of a BEST-%d run" % nsol
    ev, log = FastEvaluator(nsol, 0), []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, ev, log=log)
    assert res.final_maxdist == m
    assert [s[0] for s in ev.solutions] == sorted(a for a, _ in cands)[:nsol]
    members = set(_bits(cands))
    assert log and all(c in members for c in _bits(log))
    assert len(set(_bits(log))) == len(log)  # (no candidate twice)


@pytest.mark.parametrize("windows", [None, "1,1.5", "0"])
@pytest.mark.parametrize("name", list(ALL_BLOCKS))
def test_reference_order_mode_log_is_the_oracles(ctx, monkeypatch, name, windows):
    """ordered=True: for BEST-1, BEST-5, opportunistic-3 and FIRST-1 the log is the oracle's as an ordered list, bit
    for bit, although most distances repeat — only the rank of enum_order.h orders them, at centres equal to x_0 and at
    half-integer centres; the final bound agrees; the device's counts are per level >= the oracle's.  With the default
    windows, many tiny ones and a single one.  Some of these runs report a candidate AT the current bound (the `<=` after
    an evaluator returned max_dist = dist)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    if windows is not None:
        monkeypatch.setenv("FPHIP_ORDER_WINDOWS", windows)
    mut, rdiag, pruning, R = ALL_BLOCKS[name]()
    at_bound = 0
    for nsol, strategy in EVALUATORS:
        ev_o, log_o = FastEvaluator(nsol, strategy), []
        nodes_o, final_o = C.oracle_enumerate(mut, rdiag, pruning, R, ev_o, log_o)
        at_bound += E.reports_at_current_bound(log_o, FastEvaluator(nsol, strategy), R)
        ev, log = FastEvaluator(nsol, strategy), []
        res = enumerate_block(ctx, mut, rdiag, pruning, R, ev, log=log, ordered=True)
        assert _bits(log) == _bits(log_o) and len(log_o) >= 1, (nsol, strategy)
        assert float(res.final_maxdist).hex() == float(final_o).hex(), (nsol, strategy)
        assert ev.solutions == ev_o.solutions
        low = [(k, int(res.nodes[k]), int(nodes_o[k])) for k in range(len(rdiag)) if int(res.nodes[k]) < int(nodes_o[k])]
        assert not low, "levels with fewer nodes than the oracle (level, device, oracle): %s" % low
        assert res.stats.windows >= 1 and (windows != "0" or res.stats.windows == 1)
    assert at_bound >= 1, "no run of this block reports a candidate at the current bound"


@pytest.mark.parametrize("name", ["dy20", "pr28"])
def test_subsolutions_are_the_exact_minima(ctx, name):
    """findsubsols on a tie block: an offset has a sub-solution iff the smallest non-zero partial distance of the exact
    reference at that level is below r_kk (enumerate.cpp:143, enumerate_base.cpp:36-40), its distance IS that minimum,
    and the reported vector attains it in rational arithmetic.  Which of several tied vectors comes is not asserted.
    The main results are unchanged by the option."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _reference(name)
    d = len(rdiag)
    level_min = E.exact_of(name)[2]["level_min"]
    want = {k: level_min[k] for k in range(d) if level_min[k] is not None and level_min[k] < rdiag[k]}
    assert len(want) >= 5
    ev, log = FastEvaluator(10**9, 0), []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, ev, log=log, findsubsols=True)
    assert [int(v) for v in res.nodes] == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)
    assert sorted(ev.sub_solutions) == sorted(want)
    for o, (dist, x) in ev.sub_solutions.items():
        assert dist == want[o]
        assert all(v == 0.0 for v in x[:o]) and all(float(v).is_integer() for v in x)
        tot = Fraction(0)
        for i in range(o, d):
            c = sum((Fraction(float(mut[i, j])) * Fraction(float(x[j])) for j in range(i + 1, d)), Fraction(0))
            tot += Fraction(float(rdiag[i])) * (Fraction(float(x[i])) + c) ** 2
        assert tot == Fraction(dist), "sub-solution of offset %d: the vector does not have the reported length" % o
