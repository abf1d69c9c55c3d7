"""Closest-vector enumeration of blocks of 65 .. 256 rows on the GPU (enum_top_cvp_kernel<NQT, false, false> above
level 64, the closest-vector walk below), against two references that share nothing with the kernels:

  * tests/exact_cvp.py on the narrow dyadic blocks of tests/wide_cvp_cases.py — w72 (NQT = 2, the column stack in LDS)
    and w136 (NQT = 4, the stack in global memory): a few thousand exact nodes, the top branches, four closest vectors
    tie;
  * tests/golden/cvpw_*.json.gz — the real reference through tests/native/cvp_ref_driver.cpp at d = 72, 96 and 136
    (tests/golden/make_cvp_wide_fixtures.sh says what each is for; their conditions: tests/test_enum_cvp_wide_cpu.py).

Every comparison is `==`: per-level counts (mod 2^64), candidates (distance and coefficients, bit for bit), final
distances.  Above 64 rows the mode is opt-in (FPHIP_CVP_WIDE=1; by default such a call is declined as it always was):
every test of this file runs with the switch on, except where it says otherwise."""
import os

import numpy as np
import pytest

import conftest as C
import wide_cvp_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _wide_targets_on(monkeypatch):
    monkeypatch.setenv("FPHIP_CVP_WIDE", "1")


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _sorted_bits(log):
    return _bits(sorted((a, tuple(b)) for a, b in log))


def _device(ctx, mut, rdiag, pruning, R, target, **kw):
    """A run whose radius never shrinks: (per-level counts, log of candidates, result)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    log = []
    res = enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(10**9, 0), log=log, target=target, **kw)
    return [int(v) for v in res.nodes], log, res


@pytest.mark.parametrize("name", list(W.WIDE_BLOCKS))
def test_exact_wide_blocks_counts_and_candidates(ctx, name):
    """Per-level counts and the sorted candidate list equal the rational reference's; the four tied closest vectors
    are all reported."""
    mut, rdiag, pruning, R, target = W.wide_cvp_block(name)
    nodes_ref, cands_ref, stats = W.exact_of(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, target)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)
    best = min(a for a, _ in log)
    assert sum(1 for a, _ in log if a == best) == stats["min_group"] == 4


@pytest.mark.parametrize("name", W.FIXTURES)
def test_wide_golden_fixed_radius_counts_and_candidates(ctx, name):
    """The reference's per-level counts (mod 2^64 where its unchecked decrement wrapped; the compensation covers the
    levels >= 64: cvpw_d96_k0's descent leaves the radius above level 64) and its multiset of candidates."""
    f = W.fixture(name)
    nodes, log, _ = _device(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], f["target"])
    assert nodes == f["nodes"]
    assert _sorted_bits(log) == _bits(f["cands"])


@pytest.mark.parametrize("name", W.FIXTURES)
def test_wide_golden_best1_final_distance(ctx, name):
    """BEST_N(1): the final distance is the reference's bit for bit (precondition, asserted on the CPU: the shortest
    candidate passes every pruned bound under its own distance, and it is the only one at that distance)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = W.fixture(name)
    m, xm = f["cands"][0]
    ev = FastEvaluator(1, 0)
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, target=f["target"])
    assert float(ev.solutions[0][0]).hex() == float(m).hex()
    assert tuple(ev.solutions[0][1]) == xm
    assert float(res.final_maxdist).hex() == float(m).hex()


def test_wide_lattice_point_target_is_at_distance_zero(ctx):
    from fplll_amd.enumeration import closest_vector_block
    name = [n for n in W.FIXTURES if n.endswith("_lattice")][0]
    f = W.fixture(name)
    dist, x = closest_vector_block(ctx, f["mut"], f["rdiag"], f["target"], f["maxdist"], pruning=f["pruning"])
    assert dist == 0.0 and float(dist).hex() == "0x0.0p+0"
    assert x == tuple([0.0] * (f["d"] - 1) + [3.0]) and (dist, x) == f["best"]


PATHS = {"walk3=0": dict(FPHIP_WALK3="0"), "walk2=0": dict(FPHIP_WALK2="0"), "budget=64": dict(FPHIP_BUDGET="64"),
         "bfs=0": dict(FPHIP_BFS="0")}


@pytest.mark.parametrize("switch", list(PATHS))
@pytest.mark.parametrize("name", ["w72", "w136"])
def test_wide_paths_give_the_identical_result(ctx, monkeypatch, name, switch):
    """Each generation of the walk, split launches, and a donation budget so small that donated prefixes are replayed
    from the task's column (which carries the target and the levels >= 64): counts and candidates unchanged."""
    for k, v in PATHS[switch].items():
        monkeypatch.setenv(k, v)
    mut, rdiag, pruning, R, target = W.wide_cvp_block(name)
    nodes_ref, cands_ref, _ = W.exact_of(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, target)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


def test_wide_small_task_buffer_restarts_with_split_launches(monkeypatch):
    """cvpw_d72_real (1078 level-64 nodes, 10^6 nodes below them) with a task buffer of 2048: the level-64 nodes fit,
    the breadth-first stage below them overflows, and the call starts over with split launches — the root top task is
    set up again, target and all.  Counts and candidates unchanged; the statistics say it happened."""
    import fplll_amd
    monkeypatch.setenv("FPHIP_TASK_CAP", "2048")
    c2 = fplll_amd.Context(0)
    try:
        f = W.fixture("cvpw_d72_real")
        nodes, log, res = _device(c2, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], f["target"], target_tasks=100000)
        assert nodes == f["nodes"]
        assert _sorted_bits(log) == _bits(f["cands"])
        assert res.stats.bfs_restarts >= 1
    finally:
        c2.close()


def test_wide_declines(ctx, monkeypatch):
    """Above 256 rows the mode is declined like a shortest-vector call; the other limits keep their texts at 72 rows;
    without the switch a block above 64 rows is declined with the text it always had, and nothing is launched."""
    from fplll_amd.enumeration import FastEvaluator, Unsupported, enumerate_block
    d = 257
    with pytest.raises(Unsupported, match="256 rows"):
        enumerate_block(ctx, np.zeros((d, d)), np.ones(d), None, 0.5, FastEvaluator(1, 0), target=np.full(d, 0.25))
    mut, rdiag, pruning, R, target = W.wide_cvp_block("w72")
    cases = [(dict(dual=True), "dual"), (dict(findsubsols=True), "findsubsols"), (dict(ordered=True), "ordered"),
             (dict(shard_index=0, shard_count=2), "ranks")]
    for kw, word in cases:
        with pytest.raises(Unsupported, match="closest-vector.*" + word):
            enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(1, 0), target=target, **kw)
    monkeypatch.delenv("FPHIP_CVP_WIDE")
    with pytest.raises(Unsupported, match="closest-vector.*64 rows.*FPHIP_CVP_WIDE"):
        enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(1, 0), target=target)
    monkeypatch.setenv("FPHIP_CVP_WIDE", "0")
    with pytest.raises(Unsupported, match="closest-vector.*64 rows"):
        enumerate_block(ctx, mut, rdiag, pruning, R, FastEvaluator(1, 0), target=target)


@pytest.mark.parametrize("name", ["enum_d72_lin60_fixed", "enum_d96_lin90_fixed"])
def test_wide_without_a_target_nothing_changed(ctx, name):
    """target=None above 64 rows: the shortest-vector call, today's counts."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = C.load_fixture(os.path.join(C.GOLDEN, name + ".json"))
    ev = FastEvaluator(f["max_sols"], f["strategy"])
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, target=None)
    assert [int(v) for v in res.nodes] == f["nodes"]
    assert sorted(s[0] for s in ev.solutions) == sorted(a for a, _ in f["sol_log"])
