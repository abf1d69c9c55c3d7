"""Reference-order mode of the enumeration (enumerate_block(..., ordered=True), fphip_enum_opts::ordered) on the GPU.

Contract (DESIGN.md "reference-order mode"; the contract of the default mode is in tests/test_enum_gpu.py):
  * whatever the evaluator does to the radius — BEST_N, opportunistic, FIRST_N — the evaluator receives EXACTLY the
    candidates the reference's enumerator hands its evaluator, in the reference's order: the log of the call equals
    the fixture's sol_log as an ordered list, bit for bit, and so does the final radius;
  * the same from run to run, and under every scheduling switch (walk generation, breadth-first stage or split
    launches, a task buffer so small that subtrees are walked inline);
  * the per-level node counts are the DEVICE's work, a superset of the reference's walk: per level >= its counts;
  * dual, sub-solutions, blocks above 64 rows and several ranks are declined (Unsupported), never answered inexactly.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conftest as C

pytestmark = pytest.mark.gpu


def _shrinking(path):
    with open(path) as fh:
        j = json.load(fh)
    fixed = j["max_sols"] >= 1000000 and j["strategy"] == 0
    return j["d"] <= 64 and not fixed and not path.endswith("_subsols.json")


ENUM_CASES = [p for p in C.enum_fixtures() if _shrinking(p)]
C3_CASES = [os.path.join(C.GOLDEN, "c3_b60_k%d_%s.json" % (k, kind)) for k in (0, 1, 2) for kind in ("pruner", "linear30")]


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


def _check(ctx, f, **kw):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
    res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log, ordered=True, **kw)
    C.note(lambda: ("%s ordered: %d nodes (reference %d), %d windows, %d candidates -> %d solutions, %.2f ms kernels, "
                    "%.2f ms wall" % (f["name"], res.total_nodes, sum(f["nodes"]), res.stats.windows, res.stats.candidates,
                                      res.stats.solutions, res.stats.kernel_ms, res.stats.wall_ms),))
    assert _bits(log) == _bits(f["sol_log"])
    assert float(res.final_maxdist).hex() == float(f["final_maxdist"]).hex()
    low = [(k, int(res.nodes[k]), f["nodes"][k]) for k in range(f["d"]) if int(res.nodes[k]) < f["nodes"][k]]
    assert not low, "levels with fewer nodes than the reference (level, device, reference): %s" % low
    assert res.stats.solutions == len(f["sol_log"]) and res.stats.candidates >= res.stats.solutions
    return res


def test_the_case_lists_are_what_the_contract_names():
    names = [os.path.basename(p)[:-5] for p in ENUM_CASES]
    for want in ("enum_d12_best1", "enum_d32_best1", "enum_d32_best5", "enum_d32_first1", "enum_d32_opp3",
                 "enum_d36_lin18_best1", "enum_d48_lin30_best1"):
        assert want in names
    assert all(os.path.exists(p) for p in C3_CASES)


@pytest.mark.parametrize("path", ENUM_CASES, ids=lambda p: os.path.basename(p)[:-5])
def test_reference_fixture_log_is_exact(ctx, path):
    _check(ctx, C.load_fixture(path))


@pytest.mark.parametrize("path", C3_CASES, ids=lambda p: os.path.basename(p)[:-5])
def test_config3_block_log_is_exact(ctx, path):
    """The beta = 60 blocks of config 3, under the pruner's coefficients (k2_pruner: the block on which the default
    mode ends on another vector than the reference in most runs) and under LinearPruningParams(60, 30)."""
    res = _check(ctx, C.load_fixture(path))
    assert res.stats.windows >= 1


def test_two_runs_are_identical(ctx):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    f = C.load_fixture(os.path.join(C.GOLDEN, "c3_b60_k2_pruner.json"))
    logs = []
    for _ in range(2):
        ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
        enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log, ordered=True)
        logs.append(_bits(log))
    assert logs[0] == logs[1] == _bits(f["sol_log"])


@pytest.mark.parametrize("name,value", [("FPHIP_WALK3", "0"), ("FPHIP_WALK2", "0"), ("FPHIP_BFS", "0"),
                                        ("FPHIP_ORDER_WINDOWS", "1,1.5"), ("FPHIP_ORDER_WINDOWS", "0")])
def test_scheduling_switches_do_not_change_the_log(ctx, monkeypatch, name, value):
    """The second-generation walk, the first-generation kernel, split launches instead of the breadth-first stage,
    many tiny windows and one single window: the same log."""
    monkeypatch.setenv(name, value)
    for fx in ("enum_d36_lin18_best1", "enum_d32_best5"):
        res = _check(ctx, C.load_fixture(os.path.join(C.GOLDEN, fx + ".json")))
        if name == "FPHIP_ORDER_WINDOWS":
            assert (res.stats.windows == 1) == (value == "0")


def test_inline_overflow_candidates_are_replayed_in_order(monkeypatch):
    """A tiny task buffer: subtrees that do not fit are walked inline by the split launches and report their leaves
    long before the windows reach them — they wait in the store until the frontier has passed them."""
    import fplll_amd
    monkeypatch.setenv("FPHIP_TASK_CAP", "256")
    c2 = fplll_amd.Context(0)
    try:
        for fx in ("enum_d32_best5", "enum_d36_lin18_best1"):
            res = _check(c2, C.load_fixture(os.path.join(C.GOLDEN, fx + ".json")), target_tasks=100000)
            assert res.stats.overflowed == 1
    finally:
        c2.close()


def test_a_rank_beyond_a_key_byte_is_ordered_on_the_host(ctx):
    """One level with a tiny r_kk inside the breadth-first stage: nodes with ~300 children there, so the tasks' ranks do
    not fit the byte the device key gives a level and the call orders its list with the host comparator.  The oracle
    is the reference here (seeded block), with an evaluator that shrinks the radius."""
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    d, fat = 12, 6
    mut, rdiag, _ = C.synthetic_block(d, 8, 0.0, 1.0)
    rdiag = rdiag.copy()
    rdiag[fat] = 5e-5
    maxdist = 1.6
    nodes_f, _ = C.oracle_enumerate(mut, rdiag, None, maxdist, FastEvaluator(10**9, 0))
    assert int(nodes_f[fat]) > 127 * int(nodes_f[fat + 1])  # (more than 127 children per node: ranks beyond 254)
    for nsol, strat in ((1, 0), (5, 0), (3, 1)):
        ev_o, log_o = FastEvaluator(nsol, strat), []
        nodes_o, final_o = C.oracle_enumerate(mut, rdiag, None, maxdist, ev_o, log_o)
        ev, log = FastEvaluator(nsol, strat), []
        res = enumerate_block(ctx, mut, rdiag, None, maxdist, ev, log=log, ordered=True)
        assert _bits(log) == _bits(log_o) and len(log_o) >= 1
        assert res.final_maxdist == final_o
        assert all(int(res.nodes[k]) >= int(nodes_o[k]) for k in range(d))


def test_unsupported_combinations_are_declined(ctx):
    from fplll_amd.enumeration import FastEvaluator, Unsupported, enumerate_block
    mut, rdiag, maxdist = C.synthetic_block(24, 3, 0.04, 1.2)
    for kw in (dict(dual=True), dict(findsubsols=True), dict(shard_index=0, shard_count=2),
               dict(exchange=lambda bound, active: (bound, active))):  # (a bound exchange: a foreign bound)
        with pytest.raises(Unsupported):
            enumerate_block(ctx, mut, rdiag, None, maxdist, FastEvaluator(1, 0), ordered=True, **kw)
    mut, rdiag, maxdist = C.synthetic_block(80, 3, 0.03, 0.4)
    with pytest.raises(Unsupported):
        enumerate_block(ctx, mut, rdiag, None, maxdist, FastEvaluator(1, 0), ordered=True)
    # ... and the same calls without the flag are answered
    mut, rdiag, maxdist = C.synthetic_block(24, 3, 0.04, 1.2)
    enumerate_block(ctx, mut, rdiag, None, maxdist, FastEvaluator(1, 0), dual=True)


def _tour(beta, plug, env_extra, dump=None):
    drv = os.path.join(C.ROOT, "oracle", "_ref", "ref_driver")
    so = os.path.join(C.ROOT, "fplll_amd", "lib", "libfplll_hip_extenum.so")
    assert os.path.exists(drv) and os.path.exists(so), "oracle/_ref/ref_driver or the plugin shim is missing"
    basis = os.path.join(C.GOLDEN, "basis_q180_seed0_lll_bkz20.txt")
    strat = os.path.join(C.GOLDEN, "strategies_q180_b60.json")
    env = dict(os.environ, **env_extra)
    if dump:
        env["REFDRV_DUMP_BASIS"] = dump
    out = subprocess.run([drv, "bkztour", basis, strat, str(beta), so if plug else "none"], capture_output=True,
                         text=True, timeout=3000, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1]), out.stderr


TOUR_BETA = 50  # (the reference's own tour at this block size: 11 s on one host core, 0.6 s at 40)


def test_bkz_tour_through_the_plugin_is_the_references():
    """One BKZ-50 tour of the 180-row q-ary basis with the committed strategies, by the reference with its own
    enumerator and with every enumeration (FPLLL_HIP_MIN_NODES=0) on the device in reference-order mode: the same
    basis, by fingerprint — thousands of pruned enumerations with a shrinking radius, preprocessing and
    rerandomisation included, each of which has to end on the reference's very vector."""
    ref, _ = _tour(TOUR_BETA, False, {})
    ours, err = _tour(TOUR_BETA, True, dict(FPLLL_HIP_ORDERED="1", FPLLL_HIP_MIN_NODES="0", FPLLL_HIP_STATS="1"))
    C.note(lambda: ("BKZ-%d tour: reference %.2f s, plugin in reference-order mode %.2f s; %s" %
                    (TOUR_BETA, ref["tour_seconds"], ours["tour_seconds"], err.strip().splitlines()[-1:]),))
    # the switch did something: the plugin's own count of calls answered in reference-order mode (without the mode
    # the shim reports 0 here, and at this block size the default mode happens to reach the same basis)
    m = re.search(r"(\d+) enumerations on the device .* (\d+) in reference-order mode \((\d+) windows", err)
    assert m, err[-2000:]
    assert int(m.group(1)) > 0 and int(m.group(2)) == int(m.group(1)) and int(m.group(3)) >= int(m.group(2))
    assert ours["basis_fnv"] == ref["basis_fnv"]
    assert ours["r00"] == ref["r00"] and ours["status"] == ref["status"]


@pytest.mark.gpu_long
def test_config3_bkz60_tour_through_the_plugin_is_the_references(tmp_path):
    """Config 3's BKZ-60 tour (15 160 enumerations in the reference, 1.2e9 nodes) through the plugin in
    reference-order mode returns the basis of the reference's own tour, row for row.
    (The golden b_out of c3_bkz60_tour_strategies.json.gz was recorded with the rerandomisation generator seeded 1
    (ref_driver bkzfix); `bkztour`, the only command that takes a plugin, leaves the generator at its default state, so
    its tour — with either enumerator — is another one than the golden's: the reference run of the SAME command is the
    yardstick here, 100 s on one host core.)"""
    def basis(path):
        with open(path) as fh:
            txt = fh.read().replace("[", " ").replace("]", " ")
        return np.array([int(v) for v in txt.split()], dtype=np.int64)

    ref, _ = _tour(60, False, {}, dump=str(tmp_path / "ref.txt"))
    ours, err = _tour(60, True, dict(FPLLL_HIP_ORDERED="1", FPLLL_HIP_MIN_NODES="0", FPLLL_HIP_STATS="1"),
                      dump=str(tmp_path / "ours.txt"))
    C.note(lambda: ("BKZ-60 tour: reference %.1f s, plugin in reference-order mode %.1f s; %s" %
                    (ref["tour_seconds"], ours["tour_seconds"], err.strip().splitlines()[-1:]),))
    assert ours["basis_fnv"] == ref["basis_fnv"]
    b_ours, b_ref = basis(str(tmp_path / "ours.txt")), basis(str(tmp_path / "ref.txt"))
    assert b_ref.size == 180 * 180 and np.array_equal(b_ours, b_ref)
