"""Closest-vector mode of the enumeration on the GPU (enumerate_block(..., target=t), fphip_enum_opts::target; DESIGN.md
section 3c), against two references that share nothing with the kernels:

  * tests/exact_cvp.py — exact rational arithmetic over the order-free definition of the visited set, on dyadic blocks
    where every centre is a multiple of 1/q (sizes and tie counts: the table in tests/test_enum_cvp_cpu.py).  q2t and
    z8t are where half-integer centres make siblings tie; z8t has 2^8 closest vectors at one distance.
  * tests/golden/cvp_*.json — runs of the real reference's Enumeration::enumerate with a target, recorded by
    tests/native/cvp_ref_driver.cpp on general-position blocks (tests/golden/make_cvp_fixtures.sh says what each is for).

Every comparison is `==`: per-level counts, candidates (distance and coefficients, bit for bit), final distances."""
import glob
import json
import os

import numpy as np
import pytest

import conftest as C
import exact_cvp as X

pytestmark = pytest.mark.gpu

# each of the three kernels of the final walk answers alone (third / second generation of enum_walk_cvp_kernel,
# enum_phase_cvp_kernel), split launches instead of the breadth-first stage, and a donation budget so small that the
# prefixes of donated tasks are replayed from the task's column — which carries the target
SWITCHES = {
    "default": {}, "walk3=0": dict(FPHIP_WALK3="0"), "walk2=0": dict(FPHIP_WALK2="0"), "bfs=0": dict(FPHIP_BFS="0"),
    "budget=64": dict(FPHIP_BUDGET="64"), "walk3=0,budget=64": dict(FPHIP_WALK3="0", FPHIP_BUDGET="64"),
    "mu_global": dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0"),
}
FIXTURES = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(C.GOLDEN, "cvp_*.json")))
_fixture_cache = {}


def _fixture(name):
    """A recorded run of the reference, decoded once per process (read-only)."""
    if name not in _fixture_cache:
        with open(os.path.join(C.GOLDEN, name + ".json")) as fh:
            j = json.load(fh)
        d = j["d"]
        f = dict(name=name, d=d, mut=C.hexvec(j["mut"]).reshape(d, d), rdiag=C.hexvec(j["rdiag"]),
                 pruning=C.hexvec(j["pruning"]), target=C.hexvec(j["target"]), maxdist=float.fromhex(j["maxdist"]),
                 nodes=[int(v) for v in j["nodes"]],
                 cands=sorted((float.fromhex(s["dist"]), tuple(float(v) for v in s["x"])) for s in j["sol_log"]),
                 best=None if j["best"] is None else (float.fromhex(j["best"]["dist"]),
                                                      tuple(float(v) for v in j["best"]["x"])))
        _fixture_cache[name] = f
    return _fixture_cache[name]


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


def test_the_fixtures_are_the_ones_the_issue_lists():
    assert FIXTURES == ["cvp_d20_real", "cvp_d32_lattice", "cvp_d32_near", "cvp_d32_real_k0", "cvp_d32_stair",
                        "cvp_d40_real", "cvp_d40_stair", "cvp_d40_stair_bump"]


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", list(X.CVP_BLOCKS))
def test_exact_blocks_counts_and_candidates(ctx, monkeypatch, name, switch):
    """Per-level counts (the compensation with the exact k0 included) and the sorted candidate list equal the
    rational reference's; on z8t all 2^8 closest vectors are there."""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    mut, rdiag, pruning, R, target = X.CVP_BLOCKS[name]()
    nodes_ref, cands_ref, stats = X.exact_of(name)
    nodes, log, _ = _device(ctx, mut, rdiag, pruning, R, target)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)
    if name == "z8t":
        assert sum(1 for a, _ in log if a == 2.0) == 256


@pytest.mark.parametrize("walk3", ["0", "1"])
@pytest.mark.parametrize("d,fat,seed", [(9, 2, 5), (10, 5, 6), (8, 1, 5)])
def test_more_than_63_children_around_a_target(ctx, monkeypatch, walk3, d, fat, seed):
    """exact_enum.fat_level_block with a dyadic target: the nodes of level `fat` (r = 2^-12) have up to 139 children,
    more than one ballot holds — the slow levels, whose one-by-one steps must zig-zag where the shortest-vector walk
    would only count upwards.  Fat level 1, 2: inside the walk; 5: inside the breadth-first stage."""
    import exact_enum as E
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag = E.fat_level_block(d, fat, seed)
    target = X.dyadic_target(d, seed, 4)
    nodes_ref, cands_ref, stats = X.exact_cvp_enumerate(mut, rdiag, None, 1.5, target, max_nodes=30000)
    assert stats["max_children"] > 63
    nodes, log, _ = _device(ctx, mut, rdiag, None, 1.5, target)
    assert nodes == nodes_ref
    assert _sorted_bits(log) == _bits(cands_ref)


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixed_radius_counts_and_candidates(ctx, name):
    """The reference's per-level counts (mod 2^64 where its unchecked decrement wrapped) and its multiset of
    candidates."""
    f = _fixture(name)
    nodes, log, _ = _device(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], f["target"])
    assert nodes == f["nodes"]
    assert _sorted_bits(log) == _bits(f["cands"])
    if name == "cvp_d40_stair_bump":  # the rounding descent is cut by a pruned bound: the levels it never reached wrap
        assert nodes[1:21] == [2**64 - 1] * 20 and not log


def _safe_under_own_distance(f, dist, x):
    """Every partial distance of candidate x passes pruning_k * dist: a run whose radius has shrunk to `dist` (it
    never shrinks below the smallest candidate) still visits x, whatever the order of the walk."""
    d, pd = f["d"], 0.0
    for k in range(d - 1, -1, -1):
        c = f["target"][k]
        for j in range(d - 1, k, -1):
            c = c - x[j] * f["mut"][k, j]
        a = x[k] - c
        pd = pd + a * a * f["rdiag"][k]
        if not pd <= f["pruning"][k] * dist:
            return False
    return pd == dist


@pytest.mark.parametrize("name", [n for n in FIXTURES if n != "cvp_d40_stair_bump"])
def test_golden_best1_final_distance(ctx, name):
    """BEST_N(1), the radius shrinks with every candidate: the final distance is the reference's bit for bit, and —
    the minimum being unique in the fixed-radius list — so is the vector.  (Precondition, checked: the shortest
    candidate passes every pruned bound under its own distance, so no order of the walk can miss it.)"""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = _fixture(name)
    m, xm = f["cands"][0]
    assert f["best"] == (m, xm) and (len(f["cands"]) == 1 or f["cands"][1][0] > m)
    assert _safe_under_own_distance(f, m, xm)
    ev = FastEvaluator(1, 0)
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, target=f["target"])
    assert float(ev.solutions[0][0]).hex() == float(m).hex()
    assert tuple(ev.solutions[0][1]) == xm
    assert float(res.final_maxdist).hex() == float(m).hex()


def test_lattice_point_target_is_at_distance_zero(ctx):
    """The target of cvp_d32_lattice IS the lattice point 3 b_31: distance exactly 0.0, the zero leaf reported."""
    from fplll_amd.enumeration import closest_vector_block
    f = _fixture("cvp_d32_lattice")
    dist, x = closest_vector_block(ctx, f["mut"], f["rdiag"], f["target"], f["maxdist"])
    assert dist == 0.0 and float(dist).hex() == "0x0.0p+0"
    assert x == tuple([0.0] * 31 + [3.0]) and (dist, x) == f["best"]


@pytest.mark.parametrize("walk", ["default", "walk2=0"])
@pytest.mark.parametrize("name", ["cvp_d40_real", "cvp_d40_stair"])
def test_split_launches_and_donation(ctx, monkeypatch, name, walk):
    """Split launches (enum_phase_cvp_kernel with a stop level) towards a handful of tasks, which then shed work
    through donation: counts and candidates unchanged."""
    monkeypatch.setenv("FPHIP_BFS", "0")
    for k, v in SWITCHES[walk].items():
        monkeypatch.setenv(k, v)
    f = _fixture(name)
    nodes, log, res = _device(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], f["target"], target_tasks=64)
    assert nodes == f["nodes"]
    assert _sorted_bits(log) == _bits(f["cands"])
    assert res.stats.phases >= 2


@pytest.mark.parametrize("name", ["cvp_d40_real", "cvp_d40_stair"])
def test_task_buffer_overflow_is_walked_inline(monkeypatch, name):
    """A tiny task buffer: the breadth-first stage overflows, the call starts over with split launches, and those walk
    what does not fit inline, in closest-vector form.  Counts and candidates unchanged; the statistics say it
    happened."""
    import fplll_amd
    monkeypatch.setenv("FPHIP_TASK_CAP", "512")
    c2 = fplll_amd.Context(0)
    try:
        f = _fixture(name)
        nodes, log, res = _device(c2, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], f["target"], target_tasks=100000)
        assert nodes == f["nodes"]
        assert _sorted_bits(log) == _bits(f["cands"])
        assert res.stats.overflowed == 1
    finally:
        c2.close()


def test_declined_combinations(ctx):
    """v1 limits: each is declined before anything is launched, with the reason in the text."""
    from fplll_amd.enumeration import FastEvaluator, Unsupported, enumerate_block
    f = _fixture("cvp_d20_real")
    args = (ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"])
    cases = [
        (dict(dual=True), "dual"), (dict(findsubsols=True), "findsubsols"), (dict(ordered=True), "ordered"),
        (dict(shard_index=0, shard_count=2), "ranks"), (dict(exchange=lambda b, a: (b, a)), "ranks"),
        (dict(gather=lambda blk: [blk]), "ranks"),
    ]
    for kw, word in cases:
        with pytest.raises(Unsupported, match="closest-vector.*" + word):
            enumerate_block(*args, FastEvaluator(1, 0), target=f["target"], **kw)
    d = 65
    with pytest.raises(Unsupported, match="closest-vector.*64 rows"):
        enumerate_block(ctx, np.zeros((d, d)), np.ones(d), None, 0.5, FastEvaluator(1, 0), target=np.full(d, 0.25))
    # min_nodes_decline is ignored with a target: a small call is not declined
    ev = FastEvaluator(1, 0)
    enumerate_block(*args, ev, target=f["target"], min_nodes_decline=10**9)
    assert ev.solutions[0] == f["best"]
    with pytest.raises(Unsupported):
        enumerate_block(*args, FastEvaluator(1, 0), min_nodes_decline=10**9)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_target_is_an_error(ctx, bad):
    import fplll_amd
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = _fixture("cvp_d20_real")
    t = f["target"].copy()
    t[7] = bad
    with pytest.raises(fplll_amd.HipError, match="target coordinate 7 is not finite"):
        enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], FastEvaluator(1, 0), target=t)


@pytest.mark.parametrize("name", ["enum_d32_fixed", "enum_d40_lin20_fixed"])
def test_without_a_target_nothing_changed(ctx, name):
    """target=None: the shortest-vector call, today's counts (the glue's new branch is not taken)."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = C.load_fixture(os.path.join(C.GOLDEN, name + ".json"))
    ev = FastEvaluator(f["max_sols"], f["strategy"])
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, target=None)
    assert [int(v) for v in res.nodes] == f["nodes"]
    assert sorted(s[0] for s in ev.solutions) == sorted(a for a, _ in f["sol_log"])


def test_closest_vector_block(ctx):
    """closest_vector_block on the d = 32 fixtures returns the reference's vector; None when the radius holds none."""
    from fplll_amd.enumeration import closest_vector_block
    for name in ("cvp_d32_real_k0", "cvp_d32_stair", "cvp_d32_near"):
        f = _fixture(name)
        got = closest_vector_block(ctx, f["mut"], f["rdiag"], f["target"], f["maxdist"], pruning=f["pruning"])
        assert got == f["best"], name
    f = _fixture("cvp_d40_stair_bump")
    assert closest_vector_block(ctx, f["mut"], f["rdiag"], f["target"], f["maxdist"], pruning=f["pruning"]) is None
