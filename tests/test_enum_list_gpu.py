"""List mode of the enumeration on the GPU (fphip_enum_list / enumeration.list_block): every
candidate within a fixed radius, kept on the device during the walk.

References that share nothing with the kernels: the C restatement oracle under a callback that returns the bound
unchanged, the exact rational references tests/exact_enum.py and tests/exact_cvp.py, and known numbers of short vectors
(Z^8, D4, E8, the Leech lattice of the reference's test_list_cvp).  Every comparison of records is `==` on the doubles.
Radii were picked on the CPU (the oracle) so that each list holds a few hundred to a few thousand records."""
import os

import numpy as np
import pytest

import conftest as C
import exact_cvp as X
import exact_enum as E
import list_helpers as H

pytestmark = pytest.mark.gpu


class _Keep:
    """An evaluator that returns the bound unchanged: the reference's BEST_N evaluator that never fills."""

    def eval_sol(self, x, dist, maxdist):
        return maxdist


# fixture -> factor on its radius: 926, 1556 and 636 records (the last one under pruning coefficients)
ORACLE_CASES = {"enum_d24_best1": 1.8, "enum_d32_fixed": 1.5, "enum_d40_lin20_fixed": 1.5}
_oracle_cache = {}


def _oracle_case(name):
    """(fixture, radius, per-level counts, canonical list) of the oracle, computed once per process (read-only)."""
    if name not in _oracle_cache:
        f = C.load_fixture(os.path.join(C.GOLDEN, name + ".json"))
        R = f["maxdist"] * ORACLE_CASES[name]
        log = []
        nodes, _ = C.oracle_enumerate(f["mut"], f["rdiag"], f["pruning"], R, _Keep(), log=log)
        _oracle_cache[name] = (f, R, [int(v) for v in nodes], H.canonical(log))
    return _oracle_cache[name]


def _list(ctx, mut, rdiag, pruning, R, target=None, cap=1 << 16):
    from fplll_amd.enumeration import list_block
    res = list_block(ctx, mut, rdiag, pruning, R, target=target, cap=cap)
    assert res.count <= cap and res.stats.solutions == res.count
    return [int(v) for v in res.nodes], H.records(res), res


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_oracle_without_a_target(ctx, name):
    """Shortest-vector trees of 24, 32 and 40 rows: records (in canonical order) and per-level counts are the oracle's."""
    f, R, nodes_ref, recs_ref = _oracle_case(name)
    assert 300 <= len(recs_ref) <= 3000
    if name == "enum_d40_lin20_fixed":
        assert (f["pruning"] != 1.0).any()
    nodes, recs, _ = _list(ctx, f["mut"], f["rdiag"], f["pruning"], R)
    print(name, "records", len(recs), "nodes", sum(nodes))
    assert recs == recs_ref
    assert nodes == nodes_ref


@pytest.mark.parametrize("name", list(X.CVP_BLOCKS))
def test_exact_blocks_with_a_target(ctx, name):
    """The dyadic blocks of tests/exact_cvp.py: list and per-level counts equal the exact rational reference's; z8t
    holds its 2^8 tied closest vectors and 2048 more."""
    mut, rdiag, pruning, R, target = X.CVP_BLOCKS[name]()
    nodes_ref, cands_ref, _ = X.exact_of(name)
    nodes, recs, _ = _list(ctx, mut, rdiag, pruning, R, target)
    assert recs == H.canonical(cands_ref)
    assert nodes == nodes_ref
    if name == "z8t":
        assert sum(1 for a, _ in recs if a == (2.0).hex()) == 256 and len(recs) == 2304


def test_lattice_point_target_has_the_record_at_distance_zero(ctx):
    mut, rdiag = E.dyadic_block(10, 3, q=4, rexp=(0,))
    x = np.array([1.0, -2.0, 0.0, 3.0, 0.0, 0.0, -1.0, 0.0, 2.0, -1.0])
    target = np.array([x[i] + sum(x[j] * mut[i, j] for j in range(i + 1, 10)) for i in range(10)])
    nodes_ref, cands_ref, _ = X.exact_cvp_enumerate(mut, rdiag, None, 1.0, target, max_nodes=30000)
    nodes, recs, _ = _list(ctx, mut, rdiag, None, 1.0, target)
    assert recs == H.canonical(cands_ref) and nodes == nodes_ref
    assert recs[0] == ((0.0).hex(), tuple(x))


@pytest.mark.parametrize("name", ["dy12", "z8", "eq10"])
def test_exact_blocks_without_a_target_are_the_half_tree(ctx, name):
    """No zero vector, the topmost non-zero coefficient of every record is positive; list and counts are exact."""
    mut, rdiag, pruning, R = E.TIE_BLOCKS[name]()
    nodes_ref, cands_ref, _ = E.exact_enumerate(mut, rdiag, pruning, R, max_nodes=30000)
    nodes, recs, _ = _list(ctx, mut, rdiag, pruning, R)
    assert recs == H.canonical(cands_ref) and nodes == [int(v) for v in nodes_ref]
    assert len(recs) > 0
    for a, x in recs:
        nz = [v for v in x if v != 0.0]
        assert nz and nz[-1] > 0.0 and float.fromhex(a) > 0.0


def test_known_answers_small(ctx):
    """Z^8 in a unimodular basis with mu != 0 (r_8 = 16, 112, 448, 1136), D4 (kissing number 24), E8 (240)."""
    mut, rdiag = H.block_of(H.z8_basis())
    assert np.abs(mut).max() > 0.0
    assert _list(ctx, mut, rdiag, None, 4.5)[2].count == (16 + 112 + 448 + 1136) // 2 == 856
    assert _list(ctx, mut, rdiag, None, 4.5, np.zeros(8))[2].count == 1713
    mut, rdiag = H.block_of(H.d4_basis())
    assert _list(ctx, mut, rdiag, None, 2.5)[2].count == 12
    B, scale = H.e8_basis()
    mut, rdiag = H.block_of(B)
    assert _list(ctx, mut, rdiag, None, 2.5 * scale)[2].count == 120


def test_known_answers_leech(ctx):
    """The reference's test_list_cvp: 196 560 minimal vectors of norm 32 (one of each pair without a target), with the
    origin as a target all of them and the zero vector, the same around (0.0001, ..); around a half-lattice point of
    its loop (rep = 0 with every other coin at zero: b_0 / 2) 2 or 48 vectors within 16.5."""
    B = H.leech_basis()
    mut, rdiag = H.block_of(B)
    cap = 200000
    _, recs, res = _list(ctx, mut, rdiag, None, 32.5, cap=cap)
    print("leech: %d records, %d nodes, wall %.1f ms, kernels %.1f ms" % (res.count, res.total_nodes, res.stats.wall_ms,
                                                                        res.stats.kernel_ms))
    assert res.count == 98280 and all(a == (32.0).hex() for a, _ in recs)
    assert len(set(recs)) == 98280
    assert _list(ctx, mut, rdiag, None, 32.5, np.zeros(24), cap=cap)[2].count == 196561
    assert _list(ctx, mut, rdiag, None, 32.5, np.full(24, 0.0001), cap=cap)[2].count == 196561
    half = H.target_of(B, [0.5] + [0] * 23)
    assert _list(ctx, mut, rdiag, None, 16.5, half, cap=cap)[2].count in (2, 48)


# ---- each launch kind alone ------------------------------------------------------------------------------------------
SWITCHES = {
    "walk3=0": dict(FPHIP_WALK3="0"), "walk2=0": dict(FPHIP_WALK2="0"),
    "split": dict(FPHIP_BFS="0", FPHIP_TARGET_TASKS="64"), "split,walk2=0": dict(FPHIP_BFS="0", FPHIP_TARGET_TASKS="64",
                                                                                 FPHIP_WALK2="0"),
    "budget=64": dict(FPHIP_BUDGET="64"), "walk3=0,budget=64": dict(FPHIP_WALK3="0", FPHIP_BUDGET="64"),
    "mu_global": dict(FPHIP_MU_GLOBAL_MIN_TASKS="0", FPHIP_MU_GLOBAL_MIN_LEVEL="0"),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_each_launch_kind_without_a_target(ctx, monkeypatch, switch):
    """Walk generation 2, the phase kernel alone, split launches, donation: the list and the counts of the default."""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    f, R, nodes_ref, recs_ref = _oracle_case("enum_d32_fixed")
    nodes, recs, res = _list(ctx, f["mut"], f["rdiag"], f["pruning"], R)
    assert recs == recs_ref and nodes == nodes_ref
    if switch.startswith("split"):
        assert res.stats.phases >= 2


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", ["q2t", "pr28t"])
def test_each_launch_kind_with_a_target(ctx, monkeypatch, name, switch):
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    mut, rdiag, pruning, R, target = X.CVP_BLOCKS[name]()
    nodes_ref, cands_ref, _ = X.exact_of(name)
    nodes, recs, _ = _list(ctx, mut, rdiag, pruning, R, target)
    assert recs == H.canonical(cands_ref) and nodes == nodes_ref


@pytest.mark.parametrize("walk2", ["1", "0"])
def test_task_buffer_overflow_restarts_without_duplicates(monkeypatch, walk2):
    """A tiny task buffer: the breadth-first stage overflows and the call starts over with split launches, which walk
    what does not fit inline.  The list is the oracle's: nothing appended before the restart is seen twice."""
    import fplll_amd
    monkeypatch.setenv("FPHIP_TASK_CAP", "512")
    monkeypatch.setenv("FPHIP_TARGET_TASKS", "100000")
    monkeypatch.setenv("FPHIP_BFS_TASKS", "100000")
    monkeypatch.setenv("FPHIP_WALK2", walk2)
    c2 = fplll_amd.Context(0)
    try:
        f, R, nodes_ref, recs_ref = _oracle_case("enum_d40_lin20_fixed")
        nodes, recs, res = _list(c2, f["mut"], f["rdiag"], f["pruning"], R)
        assert recs == recs_ref and nodes == nodes_ref and len(set(recs)) == len(recs)
        assert res.stats.bfs_restarts >= 1 and res.stats.overflowed == 1
    finally:
        c2.close()


# ---- the leaf pass -----------------------------------------------------------------------------------------------------
def _fat_leaf_block():
    """Two rows, r = [2^-14, 1] (level 0 is the fat one), mu(1,0) = 1/4: everything dyadic, every sum exact."""
    mut = np.zeros((2, 2))
    mut[0, 1] = 0.25
    return mut, np.array([2.0 ** -14, 1.0])


# radius^2 (k / 128)^2: the level-1 node x_1 = 0 has k + 1 leaves (0 .. k) in the half tree: 63, 64, 65 — one pass less
# one lane, exactly one pass, one pass and one lane — and 200 (four passes); beyond 1 the node x_1 = 1 joins with a
# zig-zag around -1/4 of some 300 leaves
LEAF_RADII = [(62 / 128.0) ** 2, (63 / 128.0) ** 2, (64 / 128.0) ** 2, (199 / 128.0) ** 2]


@pytest.mark.parametrize("walk3", ["1", "0"])
@pytest.mark.parametrize("R", LEAF_RADII)
def test_leaf_passes_half_tree(ctx, monkeypatch, R, walk3):
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag = _fat_leaf_block()
    nodes_ref, cands_ref, stats = E.exact_enumerate(mut, rdiag, None, R, max_nodes=30000)
    nodes, recs, _ = _list(ctx, mut, rdiag, None, R)
    assert recs == H.canonical(cands_ref) and nodes == [int(v) for v in nodes_ref]
    if R < 1.0:
        assert nodes[0] == int(round(R ** 0.5 * 128)) + 1 and len(recs) == nodes[0] - 1


@pytest.mark.parametrize("walk3", ["1", "0"])
@pytest.mark.parametrize("R", LEAF_RADII)
def test_leaf_passes_around_a_target(ctx, monkeypatch, R, walk3):
    """The same shape with a target: the zig-zag goes both ways from a centre that is not an integer (3/8 and, under
    x_1 = 1, 1/8), first step up and first step down."""
    monkeypatch.setenv("FPHIP_WALK3", walk3)
    mut, rdiag = _fat_leaf_block()
    for target in (np.array([0.375, 0.25]), np.array([-0.375, 0.0])):
        nodes_ref, cands_ref, stats = X.exact_cvp_enumerate(mut, rdiag, None, R, target, max_nodes=30000)
        assert stats["max_children"] >= 63
        nodes, recs, _ = _list(ctx, mut, rdiag, None, R, target)
        assert recs == H.canonical(cands_ref) and nodes == nodes_ref


def test_dimensions_1_2_and_64(ctx):
    # one row: x = 1 .. 8 around the origin (the zero leaf is a node and not a record), 16 of them around 1/4
    mut, rdiag = np.zeros((1, 1)), np.array([2.0 ** -6])
    nodes_ref, cands_ref, _ = E.exact_enumerate(mut, rdiag, None, 1.0)
    nodes, recs, _ = _list(ctx, mut, rdiag, None, 1.0)
    assert recs == H.canonical(cands_ref) and len(recs) == 8 and nodes == [int(v) for v in nodes_ref]
    nodes_ref, cands_ref, _ = X.exact_cvp_enumerate(mut, rdiag, None, 1.0, np.array([0.25]))
    nodes, recs, _ = _list(ctx, mut, rdiag, None, 1.0, np.array([0.25]))
    assert recs == H.canonical(cands_ref) and len(recs) == 16 and nodes == nodes_ref
    # two rows
    mut, rdiag = E.dyadic_block(2, 1, q=4, rexp=(0, 2))
    nodes_ref, cands_ref, _ = E.exact_enumerate(mut, rdiag, None, 9.0)
    nodes, recs, _ = _list(ctx, mut, rdiag, None, 9.0)
    assert recs == H.canonical(cands_ref) and len(recs) > 10 and nodes == [int(v) for v in nodes_ref]
    # 64 rows: the oracle (r = 1, mu dyadic; 1358 records under radius^2 3)
    mut, rdiag = E.dyadic_block(64, 3, q=4, rexp=(0,))
    log = []
    nodes_ref, _ = C.oracle_enumerate(mut, rdiag, None, 3.0, _Keep(), log=log)
    assert 100 <= len(log) <= 60000
    nodes, recs, _ = _list(ctx, mut, rdiag, None, 3.0)
    assert recs == H.canonical(log) and nodes == [int(v) for v in nodes_ref]


# ---- capacity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [False, True])
def test_capacity_edges(ctx, target):
    """cap = count - 1, count, count + 1 and 0: the count stays exact, min(count, cap) records are written, each one a
    member of the full list, sorted; nothing lands behind them (sentinels)."""
    if target:
        mut, rdiag, pruning, R, t = X.CVP_BLOCKS["q2t"]()
        full = H.canonical(X.exact_of("q2t")[1])
    else:
        f, R, _, full = _oracle_case("enum_d24_best1")
        mut, rdiag, pruning, t = f["mut"], f["rdiag"], f["pruning"], None
    n, d = len(full), len(rdiag)
    members = set(full)
    for cap in (n - 1, n, n + 1, 0):
        count, dist, x, nodes, sent = H.raw_list(ctx, mut, rdiag, pruning, R, t, cap)
        m = min(n, cap)
        assert count == n
        got = H.bits(zip(dist[:m], x[:m]))
        assert all(r in members for r in got) and len(set(got)) == m
        assert got == H.canonical([(float.fromhex(a), v) for a, v in got])
        if cap >= n:
            assert got == full
        assert (dist[m:] == sent).all() and (x[m:] == sent).all()


def test_counts_do_not_leak_between_calls(ctx):
    """Two list calls, then an ordinary call on the same context: every call's own count, the fixture's result."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f, R, nodes_ref, recs_ref = _oracle_case("enum_d24_best1")
    for _ in range(2):
        nodes, recs, res = _list(ctx, f["mut"], f["rdiag"], f["pruning"], R)
        assert res.count == len(recs_ref) and recs == recs_ref
    g = C.load_fixture(os.path.join(C.GOLDEN, "enum_d32_fixed.json"))
    ev = FastEvaluator(g["max_sols"], g["strategy"])
    r2 = enumerate_block(ctx, g["mut"], g["rdiag"], g["pruning"], g["maxdist"], ev)
    assert [int(v) for v in r2.nodes] == g["nodes"]
    assert sorted(s[0] for s in ev.solutions) == sorted(a for a, _ in g["sol_log"])
    assert r2.stats.solutions == len(g["sol_log"])


def test_run_to_run_identical_arrays(ctx):
    f, R, _, recs_ref = _oracle_case("enum_d32_fixed")
    outs = [H.raw_list(ctx, f["mut"], f["rdiag"], f["pruning"], R, None, len(recs_ref) + 3) for _ in range(3)]
    for o in outs[1:]:
        assert o[0] == outs[0][0] and o[1].tobytes() == outs[0][1].tobytes() and o[2].tobytes() == outs[0][2].tobytes()


def test_declined_calls(ctx):
    from fplll_amd.enumeration import Unsupported, list_block
    with pytest.raises(Unsupported, match="list enumeration.*64 rows"):
        list_block(ctx, np.zeros((65, 65)), np.ones(65), None, 0.5)
    with pytest.raises(Unsupported, match="list enumeration.*several ranks"):
        list_block(ctx, np.zeros((8, 8)), np.ones(8), None, 0.5, shard_index=0, shard_count=2)


def test_foreign_bounds_are_ignored_during_a_list_call(ctx):
    """Another host thread keeps calling fphip_enum_lower_bound(ctx, 0) — what would end an ordinary call at once — while
    list calls run: list and counts are the oracle's.  Afterwards an ordinary call finds its fixture's result (the
    bound word is the call's own again)."""
    import ctypes
    import threading
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f, R, nodes_ref, recs_ref = _oracle_case("enum_d40_lin20_fixed")
    lib = ctx.lib
    lib.fphip_enum_lower_bound.argtypes = [ctypes.c_void_p, ctypes.c_double]
    lib.fphip_enum_lower_bound.restype = ctypes.c_int
    stop = threading.Event()

    def lower():
        while not stop.is_set():
            lib.fphip_enum_lower_bound(ctx.handle, 0.0)

    th = threading.Thread(target=lower)
    th.start()
    try:
        for _ in range(3):
            nodes, recs, _ = _list(ctx, f["mut"], f["rdiag"], f["pruning"], R)
            assert recs == recs_ref and nodes == nodes_ref
    finally:
        stop.set()
        th.join()
    g = C.load_fixture(os.path.join(C.GOLDEN, "enum_d32_fixed.json"))
    ev = FastEvaluator(g["max_sols"], g["strategy"])
    r2 = enumerate_block(ctx, g["mut"], g["rdiag"], g["pruning"], g["maxdist"], ev)
    assert [int(v) for v in r2.nodes] == g["nodes"]
