"""The chain link of the walk kernels (enum_walk.hip) on the GPU since roundto()'s tie test left it:
the vector test of every expansion runs around rint(centre), and the tie is corrected on the descent with siblings
only — a tie has no child or at least two, the ballot's popcount and the first child's distance do not depend on which
of the two nearest integers is x_0 (tests/test_walk_tie_model.py).  Both generations (FPHIP_WALK3=0/1: the second
shares the vector test), at the smallest shapes where this — and the bookkeeping around the link: the special levels,
the sibling masks, the pushes — can go wrong:

  half-integer centres   the tie blocks of tests/exact_enum.py at a fixed radius against the exact rational reference
                         (counts per level, every candidate with its coefficients), mu in LDS and through the buffer
                         loads; the dual recursion (its column update multiplies by x_0 - c, whose sign the correction
                         flips) against the C oracle's (the exact reference has no dual walk);
  emission levels        the same blocks under the smallest donation budget: emission levels appear inside chains, the
                         prefix of every donated task is replayed with roundto(centre) on tie centres;
  zero chain, 61+        a root of distance 0 and a level with more than 63 children on blocks of 8-12 rows: most chains
                         run down to level 1; these exits redo the expansion by hand with their own roundto;
  global pushes          a seeded block of 44 rows with the stack split low: the descents with siblings above the split
                         push to the global slots — the block the tie correction now sits in front of;
  reprune                BEST-1 and BEST-5 on the tie blocks: the bound drops onto pending siblings of levels whose
                         stored x_0 is the corrected one — the guarantees of test_enum_exact_ties_gpu.py."""
import numpy as np
import pytest

import conftest as C
import exact_enum as E

pytestmark = pytest.mark.gpu

WALKS = ["0", "1"]
HALF_BLOCKS = ["q2", "dy12", "dy20", "pr28"]
MU = {  # (test_enum_walk3_gpu.py's switches)
    "mu_lds": dict(FPHIP_MU_GLOBAL_MIN_TASKS="1000000000", FPHIP_MU_GLOBAL_MIN_LEVEL="1000"),
    "mu_global": dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0"),
}
_cache = {}


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _sorted_bits(log):
    return _bits(sorted((a, tuple(b)) for a, b in log))


def _env(monkeypatch, walk3, **kw):
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


def _device(ctx, mut, rdiag, pruning, R, **kw):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    log = []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log=log, **kw)
    return [int(v) for v in res.nodes], log, res


def _oracle(mut, rdiag, pruning, R, **kw):
    from fplll_amd.enumeration import FastEvaluator
    log = []
    nodes, _ = C.oracle_enumerate(mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log, **kw)
    return [int(v) for v in nodes], sorted((a, tuple(b)) for a, b in log)


def _half_block(name):
    """A tie block with its exact reference — after the check that makes the case prove something: counted nodes below
    a non-zero prefix DO have half-integer centres."""
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    nodes, cands, stats = E.exact_of(name)
    assert stats["half_centres"] > 0, "%s has no half-integer centre below a non-zero prefix" % name
    return mut, rdiag, pruning, R, nodes, cands


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("mu", list(MU))
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_half_integer_centres_fixed_radius(ctx, monkeypatch, name, mu, walk3):
    _env(monkeypatch, walk3, **MU[mu])
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_half_integer_centres_dual(ctx, monkeypatch, name, walk3):
    """DUAL multiplies the column update by a1 = x_0 - c: the tie correction flips its sign.  (The dual walk's centres
    are driven by a1, so only its first levels meet exact halves — the precondition is the primal one.)"""
    _env(monkeypatch, walk3)
    mut, rdiag, pruning, R, _, _ = _half_block(name)
    nodes_o, cands_o = _cached(("dual", name), lambda: _oracle(mut, rdiag, pruning, R, dual=True))
    assert len(cands_o) >= 3
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, dual=True)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_emission_levels_inside_chains(ctx, monkeypatch, name, walk3):
    """FPHIP_BUDGET=64, the smallest budget that acts (a task may shed work from its first refresh on), on a handful of
    tasks as large as the tree allows (the breadth-first stage stops one level below the root): emission levels sit
    inside chains, donated subtrees come back as tasks of later launches with a replayed prefix.  That tasks WERE
    donated shows in the number of launches, against a run that may not donate (FPHIP_MAX_ROUNDS=0).  Counts add up to
    the reference's and the candidates are the reference's, in both runs."""
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    _env(monkeypatch, walk3, FPHIP_BFS_HEAVY="1000000000", FPHIP_MAX_ROUNDS="0")
    nodes0, log0, plain = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    monkeypatch.delenv("FPHIP_MAX_ROUNDS")
    monkeypatch.setenv("FPHIP_BUDGET", "64")
    nodes, log, res = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    print("launches: %d with the budget, %d without donation" % (res.stats.phases, plain.stats.phases))
    assert res.stats.phases > plain.stats.phases, "no donation round: the case proves nothing"
    assert nodes0 == nodes_ref and nodes == nodes_ref
    assert _sorted_bits(log0) == _bits(cands_ref)
    assert _sorted_bits(log) == _bits(cands_ref)


FAT = [(8, 1, 5, 1.5), (10, 2, 6, 1.5), (12, 1, 9, 1.25), (12, 3, 4, 1.25)]


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("d,fat,seed,R", FAT)
def test_zero_chain_and_more_than_63_children(ctx, monkeypatch, walk3, d, fat, seed, R):
    """exact_enum.fat_level_block: the root has distance 0 (every level is special until the first step away from the
    zero chain) and every node of level `fat` has up to 91 children (popcount 64: the general path)."""
    _env(monkeypatch, walk3)
    mut, rdiag = E.fat_level_block(d, fat, seed)
    nodes_e, cands_e, stats = _cached(("fat", d, fat, seed, R),
                                      lambda: E.exact_enumerate(mut, rdiag, None, R, max_nodes=30000))
    assert stats["max_children"] > 63
    nodes, log, _ = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_e
    assert _sorted_bits(log) == _bits(cands_e)


@pytest.mark.parametrize("walk3", WALKS)
def test_global_pushes_above_the_stack_split(ctx, monkeypatch, walk3):
    """A seeded block of 44 rows against the C oracle at a radius that never shrinks, mu through the buffer loads and
    the stack split at slot 12: the tasks' roots lie above the split, so the descents with siblings between the root and
    the split push their columns to the global slots."""
    split = 12
    _env(monkeypatch, walk3, FPHIP_STACK_SPLIT=str(split), **MU["mu_global"])
    d = 44
    mut, rdiag, maxdist = C.synthetic_block(d, 3, 0.05, 1.2)
    pruning = np.maximum(0.05, 1.0 - 0.8 * np.arange(d) / d)
    nodes_o, cands_o = _cached("global", lambda: _oracle(mut, rdiag, pruning, maxdist))
    nodes, log, res = _device(ctx, mut, rdiag, pruning, maxdist)
    print("final tasks %d, root level %d" % (res.stats.final_tasks, res.stats.final_root_level))
    # (the split is taken by launches of 1024 tasks and more: enum_host.hip)
    assert res.stats.final_tasks >= 1024 and res.stats.final_root_level > split + 1, "no push above the split"
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("nsol", [1, 5])
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_reprune_on_the_tie_blocks(ctx, monkeypatch, name, nsol, walk3):
    """BEST-1 / BEST-5 under a shrinking radius (the order is a race: logs are not compared).  By
    exact_enum.best_n_guarantee every walk order ends with the exact reference's nsol-th smallest candidate distance as
    the bound and the head of that multiset kept; every logged candidate is a member of the exact candidate set, none
    comes twice.  mu through the buffer loads (test_enum_exact_ties_gpu.py runs the default)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3, **MU["mu_global"])
    mut, rdiag, pruning, R, _, cands = _half_block(name)
    m, final_fixed, head_fixed = E.best_n_guarantee(mut, rdiag, pruning, cands, nsol)
    assert final_fixed and head_fixed, "the block no longer fixes the result of a BEST-%d run" % nsol
    ev, log = FastEvaluator(nsol, 0), []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, ev, log=log)
    assert res.final_maxdist == m
    assert [s[0] for s in ev.solutions] == sorted(a for a, _ in cands)[:nsol]
    members = set(_bits(cands))
    assert log and all(c in members for c in _bits(log))
    assert len(set(_bits(log))) == len(log)
