"""The walk kernels (enum_walk.hip, both generations) with the candidate layout of the row broadcast: z = 0 in lane 0 of
every 16-lane row, 61 distinct candidates per vector test, the first child's distance taken from lane 0 of each row by
one DPP move.  Per-level counts and candidates against the C oracle at a radius that never shrinks.  A broadcast that
took another lane, or a count that were not popcount - 3, changes distances and with them the counts: these tests pin
the DPP semantics on the hardware as well.

  * nodes with exactly 59, 61, 63 and 65 children whose outermost pair +-z has a distance EQUAL to the bound: one side
    and the other of the boundary between the vector test and the one-by-one path, as it is now (61 children and more
    go one by one) and as it was (63);
  * a dual call (the column is driven by a1 = x_0 - c, which the candidates now share);
  * a launch whose column stack is split between LDS and global memory."""
from fractions import Fraction

import numpy as np
import pytest

import conftest as C
import exact_enum as E

pytestmark = pytest.mark.gpu

WALKS = ["0", "1"]
_cache = {}


def _oracle(key, mut, rdiag, pruning, R, **kw):
    """The oracle's (nodes, sorted candidates) of a case, computed once per process and shared (read-only)."""
    from fplll_amd.enumeration import FastEvaluator
    if key not in _cache:
        log = []
        nodes, _ = C.oracle_enumerate(mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log, **kw)
        _cache[key] = ([int(v) for v in nodes], sorted((a, tuple(b)) for a, b in log))
    return _cache[key]


def _device(ctx, mut, rdiag, pruning, R, **kw):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    log = []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log=log, **kw)
    return res, [int(v) for v in res.nodes], log


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _fattest(mut, rdiag, fat, R):
    """(children, at the bound) of the fattest node of level `fat` below a NON-zero prefix, in rational arithmetic: the
    nodes of level fat + 1 below a non-zero prefix are the candidates of the block of the rows above `fat`; each has
    centre 0 at level `fat` (exact_enum.fat_level_block), its children are the z with pd + z^2 r <= R."""
    _, parents, _ = E.exact_enumerate(mut[fat + 1:, fat + 1:], rdiag[fat + 1:], None, R, max_nodes=30000)
    assert parents
    pd = min(Fraction(a) for a, _ in parents)
    r, Rf = Fraction(float(rdiag[fat])), Fraction(float(R))
    z = 0
    while pd + (z + 1) * (z + 1) * r <= Rf:
        z += 1
    return 2 * z + 1, pd + z * z * r == Rf


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("children", [59, 61, 63, 65])
@pytest.mark.parametrize("d,fat,seed", [(9, 2, 5), (8, 1, 5), (12, 2, 7)])
def test_children_counts_around_the_vector_tests_limit(ctx, monkeypatch, walk3, children, d, fat, seed):
    """exact_enum.fat_level_block at radius^2 1 + z^2 2^-12, z = 29 .. 32: the node of level `fat` below the prefix
    (0, .., 0, 1) has distance 1 and centre 0, so exactly 2 z + 1 children, the outermost two AT the bound; no node of
    the level below a non-zero prefix has more.  60 children are the most the vector test resolves: 59 stays on the hot
    path, 61, 63 and 65 take the one-by-one path (63 was the limit of the former layout).  Below the level the
    coefficients up to +-32 enter the centres."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    z = (children - 1) // 2
    R = 1.0 + z * z / 4096.0
    mut, rdiag = E.fat_level_block(d, fat, seed)
    assert _fattest(mut, rdiag, fat, R) == (children, True)
    nodes_o, cands_o = _oracle(("fat", d, fat, seed, children), mut, rdiag, None, R)
    assert sum(nodes_o) < 10**5 and nodes_o[fat] >= children
    _, nodes, log = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_o
    assert _bits(sorted((a, tuple(b)) for a, b in log)) == _bits(cands_o)


@pytest.mark.parametrize("walk3", WALKS)
def test_dual_call(ctx, monkeypatch, walk3):
    """A seeded 24-row block through the dual recursion: DUAL keeps a1 for the column update."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag, maxdist = C.synthetic_block(24, 3, 0.04, 1.2)
    nodes_o, cands_o = _oracle("dual24", mut, rdiag, None, maxdist, dual=True)
    assert 10**3 < sum(nodes_o) < 10**5 and len(cands_o) >= 3
    _, nodes, log = _device(ctx, mut, rdiag, None, maxdist, dual=True)
    assert nodes == nodes_o
    assert _bits(sorted((a, tuple(b)) for a, b in log)) == _bits(cands_o)


@pytest.mark.parametrize("walk3", WALKS)
def test_split_stack(ctx, monkeypatch, walk3):
    """A seeded 40-row block cut into more than 1024 tasks (a subtree is a task from 8 estimated nodes down) with mu
    through the buffer loads and the column stack split at slot 8: the tasks start at levels whose columns live in
    global memory, the descents with siblings push there and, lower down, into LDS."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    for k, v in dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0", FPHIP_STACK_SPLIT="8",
                     FPHIP_BFS_HEAVY="8", FPHIP_BFS_TASKS="1000000000").items():
        monkeypatch.setenv(k, v)
    d = 40
    mut, rdiag, maxdist = C.synthetic_block(d, 5, 0.05, 1.04)
    pruning = np.maximum(0.05, 1.0 - 0.9 * np.arange(d) / d)
    nodes_o, cands_o = _oracle("split40", mut, rdiag, pruning, maxdist)
    assert 3 * 10**4 < sum(nodes_o) < 10**5
    res, nodes, log = _device(ctx, mut, rdiag, pruning, maxdist)
    assert res.stats.final_tasks >= 1024 and res.stats.final_root_level >= 8  # (what the split of the stack asks for)
    assert nodes == nodes_o
    assert _bits(sorted((a, tuple(b)) for a, b in log)) == _bits(cands_o)
