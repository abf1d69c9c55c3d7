"""Exact ties, the host half — no GPU.

Every other enumeration test draws inputs in general position (conftest.synthetic_block, recorded reduced bases): no
centre is an integer or a half-integer, no two siblings tie, no distance equals its bound.  The blocks of
tests/exact_enum.py are made of dyadic rationals so that all of that happens hundreds of times per block AND every
operation is exact in double; exact_enum.exact_enumerate is then a reference in rational arithmetic that shares nothing
with oracle/enum_oracle.c or the kernels.  Here:
  * exact_enumerate against the closed form on Z^d (ball_count);
  * exact_enumerate against the C oracle on the tie blocks — counts per level, candidates bit for bit;
  * non-vacuity: the blocks do contain the ties they are named for (a block that loses them FAILS);
  * the host half of the reference-order mode (enum_order.h's rank, the replay of enum_host.hip) on the same blocks,
    where a centre sits exactly on x_0 or exactly between two integers and distances repeat;
  * the identity of test_walk_child_distance_cpu.py on operands taken from a tie block.
Every comparison is exact: there is no tolerance in this file.

Figures of the named blocks (committed generator; exact reference == C oracle on each of them):

  block    definition                                          nodes  candidates  int.c  half.c  at bound  group  distinct
  z8       Z^8, R = 4                                           1753         856   1736       0       568    568         4
  z12      Z^12, R = 2                                           651         144    638       0       132    132         2
  eq10     dyadic(10, 3, q=4, rexp=(0,)), R = 3                  991         316    237     254        35     41        31
  dy12     dyadic(12, 7, q=4, rexp=(0,1,2)), R = 1              1693         118    518     398        20     20        16
  dy20     dyadic(20, 7, q=4, rexp=(0,1,2)), R = 1.5           28029         404   7945    5948        58     58        32
  pr28     dyadic(28, 11, q=4, rexp=(0,1,2)), R = 1.5, pruned  20960         415   5671    5194        42     44        31
  q2       dyadic(16, 5, q=2, rexp=(0,1)), R = 2                7259         599   3788    3446       237    237        10
  dy20big  dy20's block at R = 2 (C oracle only)              181179        7029

(int.c / half.c: counted nodes below a non-zero prefix whose centre is an integer / a half-integer; at bound: candidates
with dist == R; group: the largest set of candidates of one distance.)  The exact reference takes 0.05-2.7 s per block
(40-100 us per node) and is computed once per process."""
import random
from fractions import Fraction

import numpy as np
import pytest

import conftest as C
import exact_enum as E
import test_enum_order_cpu as O
import test_walk_child_distance_cpu as W

EVALUATORS = [(1, 0), (5, 0), (3, 1), (1, 2)]  # (1, BEST), (5, BEST), (3, OPPORTUNISTIC), (1, FIRST)


def _oracle_fixed(name):
    from fplll_amd.enumeration import FastEvaluator
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    log = []
    nodes, _ = C.oracle_enumerate(mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log)
    return mut, rdiag, pruning, R, [int(v) for v in nodes], log


@pytest.mark.parametrize("d,R", [(1, 16), (2, 25), (3, 9), (4, 4), (5, 2), (3, 0)])
def test_ball_count_against_the_definition(d, R):
    import itertools
    m = int(R ** 0.5)
    assert E.ball_count(d, R) == sum(1 for x in itertools.product(range(-m, m + 1), repeat=d)
                                     if sum(v * v for v in x) <= R)


@pytest.mark.parametrize("name,d,R", [("z8", 8, 4), ("z12", 12, 2)])
def test_zd_closed_form(name, d, R):
    """Z^d: the candidates are half of the non-zero points of the ball, level k holds half of the non-zero points of
    the (d-k)-dimensional ball (the all-zero prefix is not counted at the levels >= 1) plus the zero leaf at level 0."""
    nodes, cands, stats = E.exact_of(name)
    assert len(cands) == (E.ball_count(d, R) - 1) // 2
    assert nodes == E.zd_nodes(d, R)
    assert (len(cands), sum(nodes)) == ((856, 1753) if name == "z8" else (144, 651))
    assert stats["half_centres"] == 0 and stats["int_centres"] > 0 and stats["at_bound"] >= 2
    for dist, x in cands:
        assert dist == sum(v * v for v in x)
        assert [v for v in reversed(x) if v != 0.0][0] > 0.0


@pytest.mark.parametrize("name", list(E.TIE_BLOCKS))
def test_exact_reference_equals_the_oracle(name):
    nodes, cands, _ = E.exact_of(name)
    mut, rdiag, pruning, R, nodes_o, log_o = _oracle_fixed(name)
    assert nodes == nodes_o
    assert O._bits(cands) == O._bits(sorted((a, tuple(b)) for a, b in log_o))
    assert sum(nodes) <= 30000


@pytest.mark.parametrize("name", E.DYADIC)
def test_the_blocks_contain_the_ties_they_are_named_for(name):
    _, cands, stats = E.exact_of(name)
    assert stats["int_centres"] > 0, "no node with an integer centre"
    assert stats["half_centres"] > 0, "no node with a half-integer centre"
    assert stats["at_bound"] >= 2, "fewer than 2 candidates with dist == bound"
    assert stats["max_group"] >= 3, "no 3 candidates of one distance"
    assert stats["distinct"] < len(cands)
    mut, rdiag, pruning, _ = E.TIE_BLOCKS[name]()
    if name == "q2":  # every centre is an integer or a half-integer
        assert set(np.unique(np.abs(mut))) == {0.0, 0.5}
    assert set(np.unique(np.abs(mut * 4.0))) <= {0.0, 1.0, 2.0} and np.all(np.diff(rdiag) <= 0.0)
    assert (pruning is not None) == (name == "pr28")


@pytest.mark.parametrize("name", list(E.TIE_BLOCKS))
def test_keys_are_distinct_and_restore_the_oracles_order(name):
    """Distances repeat (up to 568 candidates of one distance): only the rank can order them, and it has to come out
    right where the centre equals x_0 (`c >= x_0`) or lies exactly between two integers (round away from zero)."""
    lib, _ = O._lib()
    mut, rdiag, pruning, R, _, log = _oracle_fixed(name)
    mut = np.ascontiguousarray(mut)
    shuffled = list(log)
    random.Random(17).shuffle(shuffled)
    assert O._bits(shuffled) != O._bits(log)
    keyed = []
    for dist, x in shuffled:
        key, nd = O._key(lib, mut, rdiag, x)
        assert float(nd[0]).hex() == float(dist).hex()
        keyed.append((key, dist, x))
    assert len(set(k for k, _, _ in keyed)) == len(keyed)
    assert len(set(a for _, a, _ in keyed)) < len(keyed)
    keyed.sort(key=lambda t: t[0])
    assert O._bits([(a, x) for _, a, x in keyed]) == O._bits(log)


@pytest.mark.parametrize("nsol,strategy", EVALUATORS)
@pytest.mark.parametrize("name", list(E.TIE_BLOCKS))
def test_replay_equals_the_oracles_shrinking_run(name, nsol, strategy):
    from fplll_amd.enumeration import FastEvaluator
    lib, L = O._lib()
    mut, rdiag, pruning, R, _, superset = _oracle_fixed(name)
    mut = np.ascontiguousarray(mut)
    ev_o, log_o = FastEvaluator(nsol, strategy), []
    _, final_o = C.oracle_enumerate(mut, rdiag, pruning, R, ev_o, log_o)
    shuffled = list(superset)
    random.Random(23).shuffle(shuffled)
    ev = FastEvaluator(nsol, strategy)
    log, final = O._replay(lib, L, mut, rdiag, pruning, R, shuffled, ev)
    assert O._bits(log) == O._bits(log_o) and len(log_o) >= 1
    assert float(final).hex() == float(final_o).hex()
    assert ev.solutions == ev_o.solutions
    if strategy == 0:  # BEST_N: the final bound is the N-th smallest distance of the exact candidate set ...
        dists = sorted(a for a, _ in E.exact_of(name)[1])
        if pruning is None:  # (... wherever no pruning bound shrinks with the radius)
            assert final_o == dists[nsol - 1]
            assert [s[0] for s in ev.solutions] == dists[:nsol]


def test_some_run_reports_a_candidate_at_the_current_bound():
    """After a BEST_N evaluator returned max_dist = dist every vector of that very norm still passes `<=`: the oracle's
    shrinking logs of the tie blocks do contain such reports (none of the seeded blocks of the suite has one)."""
    from fplll_amd.enumeration import FastEvaluator
    hits = {}
    for name in E.TIE_BLOCKS:
        mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
        for nsol, strategy in EVALUATORS[:3]:
            log = []
            C.oracle_enumerate(mut, rdiag, pruning, R, FastEvaluator(nsol, strategy), log)
            hits[name, nsol, strategy] = E.reports_at_current_bound(log, FastEvaluator(nsol, strategy), R)
    print(hits)
    assert any(v >= 1 for v in hits.values()), hits


def _tie_operands(name):
    """(centre, parent distance, r_kk) of every level of every candidate of a block whose centre is an integer or a
    half-integer, recomputed in double (exact on these inputs)."""
    mut, rdiag, _, _ = E.TIE_BLOCKS[name]()
    d = len(rdiag)
    ci, ch = [], []
    for _, x in E.exact_of(name)[1]:
        pd = 0.0
        for k in range(d - 1, -1, -1):
            c = 0.0
            for j in range(d - 1, k, -1):
                c = c - x[j] * mut[k, j]
            if pd > 0.0:
                (ci if c == np.rint(c) else ch if c + c == np.rint(c + c) else []).append((c, pd, rdiag[k]))
            a = x[k] - c
            pd = pd + a * a * rdiag[k]
    return ci, ch


@pytest.mark.parametrize("name", ["dy12", "q2"])
def test_first_childs_distance_on_tie_operands(name):
    """test_walk_child_distance_cpu.py's identity (lane 0 of the 64-lane test == the wave-uniform expression) on
    operands of a tie block, integer and half-integer centres apart; on these operands both are also the EXACT value
    nd + (round-away(c) - c)^2 r."""
    for kind, ops in zip(("integer", "half-integer"), _tie_operands(name)):
        assert len(ops) >= 100, "%s: too few %s centres (%d)" % (name, kind, len(ops))
        c, nd, r = (np.array(v, dtype=np.float64) for v in zip(*ops))
        assert {bool(s) for s in np.signbit(c)} == {False, True} or kind == "integer"
        x1, lane0, uniform = W._both(c, nd, r)
        assert W._same_bits(lane0, uniform)
        away = np.where(c >= 0.0, np.floor(c + 0.5), np.ceil(c - 0.5))
        assert np.array_equal(x1, away)
        for i in range(0, len(ops), max(1, len(ops) // 500)):
            a = Fraction(float(away[i])) - Fraction(float(c[i]))
            assert Fraction(float(uniform[i])) == Fraction(float(nd[i])) + a * a * Fraction(float(r[i]))
            assert abs(a) == (0 if kind == "integer" else Fraction(1, 2))
