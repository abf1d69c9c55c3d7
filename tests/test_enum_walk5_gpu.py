"""The fifth-generation walk (enum_walk5_kernel, enum_walk5.hip) on the GPU next to the fourth
(FPHIP_WALK5=0), each run checked on its own against the exact rational reference or the C oracle — the cases, the
references and the helpers of tests/test_enum_walk4_gpu.py.  What the generation changes can go wrong here:

  tie blocks             fixed radius, counts per level and every candidate with its coefficients, mu in LDS and through
                         the buffer loads.  The blocks hold nodes with exactly two children on tie centres (the fourth
                         generation's computation, in its own block) and on other centres (the sibling read off the
                         test's lane, its coefficient x_0 +- 1.0), at levels in every 16-lane row of the level registers,
                         and nodes with three or more (their count is the ballot's popcount without the copies);
  dual recursion         the pair's column update multiplies by x_2 - c, formed from the new x_2;
  emission levels        FPHIP_BUDGET=64 on a handful of tasks: pending pair siblings are donated (popped column, x_2,
                         nd_2) and the prefix of every donated task is replayed with the stored x_2;
  reprune                BEST-1 / BEST-5: the bound drops onto the pair siblings' distances in lane k of pds;
  global pushes          the stack split low: the pair's column goes through the global slots;
  zero chain, 55+        the exits that expand by hand (fewer candidates than the fourth generation's 61: a node with
                         55 to 60 children takes the general path here);
  task root at level 64  the masks at their top bit, level 63 as a pair level: the last lane of the last row."""
import numpy as np
import pytest

import conftest as C
import exact_enum as E
from test_enum_walk4_gpu import (FAT, HALF_BLOCKS, MU, ROOT64, _bits, _cached, _device, _half_block, _oracle,
                                 _sorted_bits)

pytestmark = pytest.mark.gpu

WALK5 = ["0", "1"]


def _env(monkeypatch, walk5, **kw):
    monkeypatch.setenv("FPHIP_WALK5", walk5)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("mu", list(MU))
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_tie_blocks_fixed_radius(ctx, monkeypatch, name, mu, walk5):
    _env(monkeypatch, walk5, **MU[mu])
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_tie_blocks_dual(ctx, monkeypatch, name, walk5):
    _env(monkeypatch, walk5)
    mut, rdiag, pruning, R, _, _ = _half_block(name)
    nodes_o, cands_o = _cached(("dual", name), lambda: _oracle(mut, rdiag, pruning, R, dual=True))
    assert len(cands_o) >= 3
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, dual=True)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_pending_pairs_are_donated(ctx, monkeypatch, name, walk5):
    """FPHIP_BUDGET=64 on a handful of tasks (target_tasks=1): more launches than a run that may not donate; counts and
    candidates the reference's in both."""
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    _env(monkeypatch, walk5, FPHIP_BFS_HEAVY="1000000000", FPHIP_MAX_ROUNDS="0")
    nodes0, log0, plain = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    monkeypatch.delenv("FPHIP_MAX_ROUNDS")
    monkeypatch.setenv("FPHIP_BUDGET", "64")
    nodes, log, res = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    print("launches: %d with the budget, %d without donation" % (res.stats.phases, plain.stats.phases))
    assert res.stats.phases > plain.stats.phases, "no donation round: the case proves nothing"
    assert nodes0 == nodes_ref and nodes == nodes_ref
    assert _sorted_bits(log0) == _bits(cands_ref)
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("nsol", [1, 5])
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_reprune_on_the_tie_blocks(ctx, monkeypatch, name, nsol, walk5):
    """BEST-1 / BEST-5 under a shrinking radius, by exact_enum.best_n_guarantee (test_enum_walk_link_gpu.py)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk5, **MU["mu_global"])
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


@pytest.mark.parametrize("walk5", WALK5)
def test_pair_columns_through_the_global_slots(ctx, monkeypatch, walk5):
    """The 44-row seeded block with the stack split at slot 12, mu through the buffer loads."""
    split = 12
    _env(monkeypatch, walk5, FPHIP_STACK_SPLIT=str(split), **MU["mu_global"])
    d = 44
    mut, rdiag, maxdist = C.synthetic_block(d, 3, 0.05, 1.2)
    pruning = np.maximum(0.05, 1.0 - 0.8 * np.arange(d) / d)
    nodes_o, cands_o = _cached("global", lambda: _oracle(mut, rdiag, pruning, maxdist))
    nodes, log, res = _device(ctx, mut, rdiag, pruning, maxdist)
    assert res.stats.final_tasks >= 1024 and res.stats.final_root_level > split + 1, "no push above the split"
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("d,fat,seed,R", FAT)
def test_zero_chain_and_more_than_63_children(ctx, monkeypatch, walk5, d, fat, seed, R):
    _env(monkeypatch, walk5)
    mut, rdiag = E.fat_level_block(d, fat, seed)
    nodes_e, cands_e, stats = _cached(("fat", d, fat, seed, R),
                                      lambda: E.exact_enumerate(mut, rdiag, None, R, max_nodes=30000))
    assert stats["max_children"] > 63
    nodes, log, _ = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_e
    assert _sorted_bits(log) == _bits(cands_e)


@pytest.mark.parametrize("walk5", WALK5)
@pytest.mark.parametrize("case", list(ROOT64))
def test_task_root_at_level_64(ctx, monkeypatch, walk5, case):
    d, seed, slope, rf, c, env = ROOT64[case]
    _env(monkeypatch, walk5, **env)
    mut, rdiag, maxdist = C.synthetic_block(d, seed, slope, rf)
    if c is None:
        pruning = np.clip(np.linspace(1.0, 0.25, d)[::-1].copy(), 0.0, 1.0)[::-1].copy()
    else:
        pruning = np.maximum(0.05, 1.0 - c * np.arange(d) / d)
    nodes_o, cands_o = _cached(("root64", d), lambda: _oracle(mut, rdiag, pruning, maxdist))
    nodes, log, res = _device(ctx, mut, rdiag, pruning, maxdist)
    if case == "d64_whole":
        assert res.stats.final_root_level == 64 and res.stats.final_tasks == 1
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)
