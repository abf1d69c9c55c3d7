"""The fourth-generation walk (enum_walk4_kernel, enum_walk4.hip) on the GPU next to the third
(FPHIP_WALK4=0), each run checked on its own against the exact rational reference or the C oracle, on the shapes of
tests/test_enum_walk_link_gpu.py.  What the generation changes — the second child of a two-child node is formed at the
descent and only popped at the STEP — can go wrong here:

  tie blocks             fixed radius, counts per level and every candidate with its coefficients, mu in LDS and through
                         the buffer loads.  A CPU walk of the test's own first proves that the block holds nodes with
                         exactly two children above level 1 (the pair format; a tie has no child or at least two, so
                         pairs on tie centres — the corrected-x_1 direction — are among them) and nodes with three or
                         more (the third generation's format): both formats run, on the same path;
  dual recursion         the pair's column update multiplies by x_2 - c;
  emission levels        FPHIP_BUDGET=64 on a handful of tasks: pending pair siblings are donated as tasks, the prefix
                         of every donated task is replayed (a pair level below its second child: the stored x_2);
  reprune                BEST-1 / BEST-5: the bound drops onto ready pair siblings (lane registers of distances);
  global pushes          the stack split low: the pair's column is pushed to and popped from the global slots;
  zero chain, 61+        the exits that expand by hand;
  task root at level 64  the masks P, B and Q at their top bit: walks that begin at level 64, whose first descent is
                         level 63's."""
from fractions import Fraction

import numpy as np
import pytest

import conftest as C
import exact_enum as E

pytestmark = pytest.mark.gpu

WALK4 = ["0", "1"]
HALF_BLOCKS = ["q2", "dy12", "dy20", "pr28"]
# visited nodes whose children sit above level 1, by their number of children: (exactly two, three or more)
CHILDREN = {"q2": (1414, 245), "dy12": (296, 71), "dy20": (5116, 814), "pr28": (3829, 156)}
MU = {
    "mu_lds": dict(FPHIP_MU_GLOBAL_MIN_TASKS="1000000000", FPHIP_MU_GLOBAL_MIN_LEVEL="1000"),
    "mu_global": dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0"),
}
_cache = {}


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _sorted_bits(log):
    return _bits(sorted((a, tuple(b)) for a, b in log))


def _env(monkeypatch, walk4, **kw):
    monkeypatch.setenv("FPHIP_WALK4", walk4)
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


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _children_histogram(mut, rdiag, pruning, R):
    """(nodes with exactly two children, with three or more) among the visited nodes whose children sit at a level
    >= 2 — a small exact walk in rational arithmetic: the half of the tree the reference walks (below the all-zero
    prefix only x >= 0)."""
    d = len(rdiag)
    F = lambda v: Fraction(float(v))  # noqa: E731
    mu = [[F(mut[k][j]) for j in range(d)] for k in range(d)]
    r = [F(v) for v in rdiag]
    bound = [(F(pruning[k]) if pruning is not None else Fraction(1)) * F(R) for k in range(d)]
    x = [0] * d
    two_more = [0, 0]

    def visit(k, pd, zero_prefix):
        c = -sum((x[j] * mu[k][j] for j in range(k + 1, d) if x[j]), Fraction(0))
        lo = c.numerator // c.denominator
        ch = []
        v = lo
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            ch.append(v)
            v -= 1
        v = lo + 1
        while pd + (v - c) * (v - c) * r[k] <= bound[k]:
            ch.append(v)
            v += 1
        if zero_prefix:
            ch = [v for v in ch if v >= 0]
        if k >= 2:
            two_more[0] += len(ch) == 2
            two_more[1] += len(ch) >= 3
        for v in ch:
            x[k] = v
            if k > 0:
                visit(k - 1, pd + (v - c) * (v - c) * r[k], zero_prefix and v == 0)
        x[k] = 0

    visit(d - 1, Fraction(0), True)
    return tuple(two_more)


def _half_block(name):
    """A tie block with its exact reference — after the checks that make the case prove something: half-integer centres
    below a non-zero prefix, nodes with exactly two children and nodes with three or more."""
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    nodes, cands, stats = E.exact_of(name)
    assert stats["half_centres"] > 0
    hist = _cached(("hist", name), lambda: _children_histogram(mut, rdiag, pruning, R))
    assert hist == CHILDREN[name], hist
    assert hist[0] > 0 and hist[1] > 0
    return mut, rdiag, pruning, R, nodes, cands


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("mu", list(MU))
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_tie_blocks_fixed_radius(ctx, monkeypatch, name, mu, walk4):
    _env(monkeypatch, walk4, **MU[mu])
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_tie_blocks_dual(ctx, monkeypatch, name, walk4):
    _env(monkeypatch, walk4)
    mut, rdiag, pruning, R, _, _ = _half_block(name)
    nodes_o, cands_o = _cached(("dual", name), lambda: _oracle(mut, rdiag, pruning, R, dual=True))
    assert len(cands_o) >= 3
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, dual=True)
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_pending_pairs_are_donated(ctx, monkeypatch, name, walk4):
    """FPHIP_BUDGET=64 on a handful of tasks (target_tasks=1): levels with a pending sibling become emission levels,
    the sibling is stepped to and leaves as a task — a pair sibling with (popped column, x_2, nd_2) — and comes back in a
    later launch.  More launches than a run that may not donate; counts and candidates the reference's in both."""
    mut, rdiag, pruning, R, nodes_ref, cands_ref = _half_block(name)
    _env(monkeypatch, walk4, FPHIP_BFS_HEAVY="1000000000", FPHIP_MAX_ROUNDS="0")
    nodes0, log0, plain = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    monkeypatch.delenv("FPHIP_MAX_ROUNDS")
    monkeypatch.setenv("FPHIP_BUDGET", "64")
    nodes, log, res = _device(ctx, mut, rdiag, pruning, R, target_tasks=1)
    print("launches: %d with the budget, %d without donation" % (res.stats.phases, plain.stats.phases))
    assert res.stats.phases > plain.stats.phases, "no donation round: the case proves nothing"
    assert nodes0 == nodes_ref and nodes == nodes_ref
    assert _sorted_bits(log0) == _bits(cands_ref)
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("nsol", [1, 5])
@pytest.mark.parametrize("name", HALF_BLOCKS)
def test_reprune_on_the_tie_blocks(ctx, monkeypatch, name, nsol, walk4):
    """BEST-1 / BEST-5 under a shrinking radius, by exact_enum.best_n_guarantee (test_enum_walk_link_gpu.py)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    _env(monkeypatch, walk4, **MU["mu_global"])
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


@pytest.mark.parametrize("walk4", WALK4)
def test_pair_columns_through_the_global_slots(ctx, monkeypatch, walk4):
    """The 44-row seeded block with the stack split at slot 12, mu through the buffer loads: descents between the tasks'
    roots and the split push to the global slots, pair descents their sibling's column, which the pair STEP pops."""
    split = 12
    _env(monkeypatch, walk4, FPHIP_STACK_SPLIT=str(split), **MU["mu_global"])
    d = 44
    mut, rdiag, maxdist = C.synthetic_block(d, 3, 0.05, 1.2)
    pruning = np.maximum(0.05, 1.0 - 0.8 * np.arange(d) / d)
    nodes_o, cands_o = _cached("global", lambda: _oracle(mut, rdiag, pruning, maxdist))
    nodes, log, res = _device(ctx, mut, rdiag, pruning, maxdist)
    assert res.stats.final_tasks >= 1024 and res.stats.final_root_level > split + 1, "no push above the split"
    assert nodes == nodes_o
    assert _sorted_bits(log) == _bits(cands_o)


FAT = [(8, 1, 5, 1.5), (10, 2, 6, 1.5), (12, 1, 9, 1.25), (12, 3, 4, 1.25)]


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("d,fat,seed,R", FAT)
def test_zero_chain_and_more_than_63_children(ctx, monkeypatch, walk4, d, fat, seed, R):
    _env(monkeypatch, walk4)
    mut, rdiag = E.fat_level_block(d, fat, seed)
    nodes_e, cands_e, stats = _cached(("fat", d, fat, seed, R),
                                      lambda: E.exact_enumerate(mut, rdiag, None, R, max_nodes=30000))
    assert stats["max_children"] > 63
    nodes, log, _ = _device(ctx, mut, rdiag, None, R)
    assert nodes == nodes_e
    assert _sorted_bits(log) == _bits(cands_e)


# whole: the root task of the 64-row block goes to the walk launch as it is (no breadth-first stage, no splitting
# launch): the walk begins at level 64.  d = 70: the tasks are the level-64 nodes of the top walk, of non-zero
# distance — the hot chain itself starts at level 64, and level 63 (bit 63 of the masks) can be a pair level.
ROOT64 = {
    "d64": (64, 7, 0.055, 1.02, 1.25, {}),
    "d64_whole": (64, 7, 0.055, 1.02, 1.25, dict(FPHIP_BFS="0", FPHIP_MAX_SPLIT_PHASES="0")),
    "d70": (70, 22, 0.03, 0.46, None, {}),
}


@pytest.mark.parametrize("walk4", WALK4)
@pytest.mark.parametrize("case", list(ROOT64))
def test_task_root_at_level_64(ctx, monkeypatch, walk4, case):
    d, seed, slope, rf, c, env = ROOT64[case]
    _env(monkeypatch, walk4, **env)
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
