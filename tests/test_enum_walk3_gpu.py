"""The third-generation walk (enum_walk_kernel<.., CHAIN = true>, enum_walk.hip) next to the second (<.., false>, FPHIP_WALK3=0):
each run is checked on its own against the reference's golden vectors or the C oracle.  The chain walk stores nothing
for a node with one child and replays the path from the task's root column where coefficients are needed — the
level-1 leaf reports (the candidate lists below), the prefixes of donated tasks (a small FPHIP_BUDGET), reprune
after a candidate lowers the bound (BEST-1 runs) — so those paths are covered explicitly, for both instantiations
of MU_LDS (FPHIP_MU_GLOBAL_MIN_TASKS / _LEVEL move the switch) and of DUAL."""
import os

import numpy as np
import pytest

import conftest as C

pytestmark = pytest.mark.gpu

WALKS = ["0", "1"]
FIXED = [p for p in C.enum_fixtures() if p.endswith("_fixed.json")]


def _lin_pruning(d, c):
    return None if c is None else np.maximum(0.05, 1.0 - c * np.arange(d) / d)


def _sols(ev):
    return sorted((s[0], tuple(s[1])) for s in ev.solutions)


def _env(monkeypatch, walk3, **kw):
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("path", FIXED, ids=lambda p: os.path.basename(p)[:-5])
def test_fixture_counts_and_candidates(ctx, monkeypatch, walk3, path):
    """Radius that never shrinks: per-level counts and the candidates with their coefficients are fplll's."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    f = C.load_fixture(path)
    ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log)
    assert [int(v) for v in res.nodes] == f["nodes"]
    assert sorted((a, tuple(b)) for a, b in log) == sorted((a, tuple(b)) for a, b in f["sol_log"])


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("budget", ["64", "256"])
@pytest.mark.parametrize("name", ["enum_d40_lin20_fixed", "enum_d48_lin30_fixed", "enum_d80_lin70_fixed"])
def test_forced_donation(ctx, monkeypatch, walk3, budget, name):
    """A tiny donation budget: tasks shed their upper subtrees early and often, every emitted task's coefficient
    prefix comes out of the path replay — the counts and candidates stay the reference's."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3, FPHIP_BUDGET=budget)
    f = C.load_fixture(os.path.join(C.GOLDEN, name + ".json"))
    ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log)
    assert [int(v) for v in res.nodes] == f["nodes"]
    assert sorted((a, tuple(b)) for a, b in log) == sorted((a, tuple(b)) for a, b in f["sol_log"])


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("mu_global", [False, True])
@pytest.mark.parametrize("d,seed,slope,rf,c", [(20, 4, 0.03, 1.6, None), (40, 3, 0.05, 1.2, 0.8),
                                               (56, 8, 0.05, 1.05, 1.2), (64, 7, 0.055, 1.02, 1.25)])
def test_oracle_shapes_both_mu_paths(ctx, monkeypatch, walk3, mu_global, d, seed, slope, rf, c):
    """Seeded blocks at a fixed radius with mu in LDS (small launches) and through the buffer loads (big launches)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    kw = dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0") if mu_global else \
        dict(FPHIP_MU_GLOBAL_MIN_TASKS="1000000000", FPHIP_MU_GLOBAL_MIN_LEVEL="1000")
    _env(monkeypatch, walk3, **kw)
    mut, rdiag, maxdist = C.synthetic_block(d, seed, slope, rf)
    pruning = _lin_pruning(d, c)
    ev_o, ev = FastEvaluator(10**9, 0), FastEvaluator(10**9, 0)
    nodes_o, _ = C.oracle_enumerate(mut, rdiag, pruning, maxdist, ev_o)
    res = enumerate_block(ctx, mut, rdiag, pruning, maxdist, ev)
    assert [int(v) for v in res.nodes] == [int(v) for v in nodes_o]
    assert _sols(ev) == _sols(ev_o)
    # shrinking radius: every candidate lowers the bound and re-prunes the pending siblings
    ev1, ev1o = FastEvaluator(1, 0), FastEvaluator(1, 0)
    res1 = enumerate_block(ctx, mut, rdiag, pruning, maxdist, ev1)
    _, m_o = C.oracle_enumerate(mut, rdiag, pruning, maxdist, ev1o)
    if pruning is None:  # (a pruned tree under a shrinking radius is order dependent: DESIGN.md, parity)
        assert res1.final_maxdist == m_o
        assert [s[0] for s in ev1.solutions] == [s[0] for s in ev1o.solutions]


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("path", [p for p in C.dual_enum_fixtures() if p.endswith("_fixed.json")],
                         ids=lambda p: os.path.basename(p)[:-5])
def test_dual_fixtures(ctx, monkeypatch, walk3, path):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    f = C.load_fixture(path)
    ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log, dual=True)
    assert [int(v) for v in res.nodes] == f["nodes"]
    assert sorted((a, tuple(b)) for a, b in log) == sorted((a, tuple(b)) for a, b in f["sol_log"])


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("fat,d,seed,maxdist,rfat", [(2, 10, 5, 3.0, 5e-4), (3, 11, 7, 2.5, 6e-4)])
def test_zero_root_and_more_than_63_children(ctx, monkeypatch, walk3, fat, d, seed, maxdist, rfat):
    """The root of distance 0 (its chain of first children is the slow path) and a level with 60-140 children."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    mut, rdiag, _ = C.synthetic_block(d, seed, 0.0, 1.0)
    rdiag = rdiag.copy()
    rdiag[fat] = rfat
    ev, ev_o = FastEvaluator(10**9, 0), FastEvaluator(10**9, 0)
    res = enumerate_block(ctx, mut, rdiag, None, maxdist, ev)
    nodes_o, _ = C.oracle_enumerate(mut, rdiag, None, maxdist, ev_o)
    assert [int(v) for v in res.nodes] == [int(v) for v in nodes_o]
    assert _sols(ev) == _sols(ev_o)


@pytest.mark.parametrize("walk3", WALKS)
@pytest.mark.parametrize("d,seed,rf", [(70, 22, 0.46), (100, 23, 0.22)])
def test_blocks_above_64_rows(ctx, monkeypatch, walk3, d, seed, rf):
    """Tasks under level-64 ancestors: the replay starts from the subtree task's root column."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    mut, rdiag, maxdist = C.synthetic_block(d, seed, 0.03, rf)
    pruning = np.clip(np.linspace(1.0, 0.25, d)[::-1].copy(), 0.0, 1.0)[::-1].copy()
    ev, ev_o = FastEvaluator(10**9, 0), FastEvaluator(10**9, 0)
    res = enumerate_block(ctx, mut, rdiag, pruning, maxdist, ev)
    nodes_o, _ = C.oracle_enumerate(mut, rdiag, pruning, maxdist, ev_o)
    assert [int(v) for v in res.nodes] == [int(v) for v in nodes_o]
    assert _sols(ev) == _sols(ev_o)


@pytest.mark.parametrize("walk3", WALKS)
def test_wide_block_candidates_under_level64_ancestors(ctx, monkeypatch, walk3):
    """Candidates below several level-64 ancestors: the leaf reports' replayed coefficients plus the ancestors'."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    mut, rdiag, maxdist = C.wide_block_with_candidates(130, 43)
    ev, ev_o = FastEvaluator(10**9, 0), FastEvaluator(10**9, 0)
    res = enumerate_block(ctx, mut, rdiag, None, maxdist, ev)
    nodes_o, _ = C.oracle_enumerate(mut, rdiag, None, maxdist, ev_o)
    assert [int(v) for v in res.nodes] == [int(v) for v in nodes_o]
    assert len(ev_o.solutions) >= 30 and _sols(ev) == _sols(ev_o)


@pytest.mark.parametrize("walk3", WALKS)
def test_two_ranks_on_one_device_add_up(ctx, monkeypatch, walk3):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk3)
    f = C.load_fixture(os.path.join(C.GOLDEN, "enum_d48_lin30_fixed.json"))
    tot = np.zeros(f["d"] + 1, dtype=np.uint64)
    for s in range(2):
        ev = FastEvaluator(f["max_sols"], f["strategy"])
        res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev,
                              shard_index=s, shard_count=2, exchange_chunks=3)
        tot += res.nodes
    assert [int(v) for v in tot] == f["nodes"]
