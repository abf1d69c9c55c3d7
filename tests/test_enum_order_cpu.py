"""Reference-order mode (fphip_enum_opts::ordered), the host half — no GPU.

Contract of the mode (DESIGN.md "reference-order mode"): the caller's evaluator receives EXACTLY the candidates the
reference's enumerator hands its evaluator, in the reference's order, whatever the evaluator does to the radius.  Two
host pieces make that true for any superset of candidates the device reports, and are checked here against the C
oracle (conftest.oracle_enumerate) through the debug entries of include/fplll_hip_debug.h:
  * the depth-first key (fphip_debug_order_key): sorting by it restores the oracle's visiting order;
  * the replay (fphip_debug_order_replay): from the shuffled candidates of a run whose radius never shrinks (a
    superset of every shrinking run) it reproduces the oracle's log of the shrinking run — the ordered list of
    (dist, x), compared bitwise — for every evaluator kind.
"""
import ctypes
import os
import random

import numpy as np
import pytest

import conftest as C


def _lib():
    from fplll_amd import _lib
    return _lib.load(), _lib


def _lin_pruning(d, c):
    if c is None:
        return None
    return np.maximum(0.05, 1.0 - c * np.arange(d) / d)


def _key(lib, mut, rdiag, x):
    d = len(rdiag)
    rank = np.zeros(d, dtype=np.uint32)
    nd = np.zeros(d, dtype=np.float64)
    xs = np.ascontiguousarray(x, dtype=np.float64)
    rc = lib.fphip_debug_order_key(d, mut.ctypes.data, rdiag.ctypes.data, xs.ctypes.data, rank.ctypes.data,
                                   nd.ctypes.data)
    assert rc == 0
    return tuple(int(v) for v in rank[::-1]), nd  # (most significant level first: compares like the walk)


def _replay(lib, L, mut, rdiag, pruning, maxdist, cands, evaluator):
    """fphip_debug_order_replay over `cands` [(dist, x)] with a Python evaluator; returns (log, final bound)."""
    d = len(rdiag)
    dist = np.array([c[0] for c in cands], dtype=np.float64)
    xs = np.ascontiguousarray(np.array([c[1] for c in cands], dtype=np.float64).reshape(len(cands), d))
    state = {"m": float(maxdist)}
    log = []

    def cb(_u, dv, sol):
        x = [sol[i] for i in range(d)]
        log.append((dv, x))
        state["m"] = float(evaluator.eval_sol(x, dv, state["m"]))
        return state["m"]

    fb = ctypes.c_double(0.0)
    pr = None if pruning is None else np.ascontiguousarray(pruning, dtype=np.float64)
    n = lib.fphip_debug_order_replay(d, ctypes.c_double(maxdist), mut.ctypes.data, rdiag.ctypes.data,
                                     None if pr is None else pr.ctypes.data, len(cands), dist.ctypes.data,
                                     xs.ctypes.data, L.SOL_CB(cb), None, ctypes.byref(fb))
    assert n == len(log), "replay failed (%d)" % n
    return log, fb.value


def _bits(log):
    return [(float(a).hex(), tuple(float(v) for v in x)) for a, x in log]


# seeded blocks: (d, seed, slope, radius factor, linear pruning c or None): 3-400 leaves at the initial radius
BLOCKS = [(24, 101, 0.04, 1.25, None), (28, 102, 0.04, 1.45, 0.6), (30, 103, 0.045, 1.6, 0.8), (32, 104, 0.04, 1.5, 1.0),
          (34, 105, 0.035, 1.7, 1.1), (36, 106, 0.04, 1.8, 1.2), (40, 107, 0.045, 1.9, 1.3)]
EVALUATORS = [(1, 0), (5, 0), (3, 1), (1, 2)]  # (nr_solutions, strategy): BEST_N, BEST_N, opportunistic, FIRST_N


def _superset(d, seed, slope, rf, c):
    from fplll_amd.enumeration import FastEvaluator
    mut, rdiag, maxdist = C.synthetic_block(d, seed, slope, rf)
    mut = np.ascontiguousarray(mut)
    pruning = _lin_pruning(d, c)
    log = []
    C.oracle_enumerate(mut, rdiag, pruning, maxdist, FastEvaluator(10**9, 0), log)
    return mut, rdiag, pruning, maxdist, log


@pytest.mark.parametrize("d,seed,slope,rf,c", BLOCKS)
def test_key_restores_the_oracles_order(d, seed, slope, rf, c):
    lib, _ = _lib()
    mut, rdiag, pruning, maxdist, log = _superset(d, seed, slope, rf, c)
    assert len(log) >= 3, "the block has too few leaves to order (%d)" % len(log)
    shuffled = list(log)
    random.Random(seed).shuffle(shuffled)
    assert _bits(shuffled) != _bits(log)
    keyed = []
    for dist, x in shuffled:
        key, nd = _key(lib, mut, rdiag, x)
        assert float(nd[0]).hex() == float(dist).hex()  # the partial distances are the reference's sums
        keyed.append((key, dist, x))
    assert len(set(k for k, _, _ in keyed)) == len(keyed)
    keyed.sort(key=lambda t: t[0])
    assert _bits([(a, x) for _, a, x in keyed]) == _bits(log)


@pytest.mark.parametrize("nsol,strategy", EVALUATORS)
@pytest.mark.parametrize("d,seed,slope,rf,c", BLOCKS)
def test_replay_equals_the_oracles_shrinking_run(d, seed, slope, rf, c, nsol, strategy):
    from fplll_amd.enumeration import FastEvaluator
    lib, L = _lib()
    mut, rdiag, pruning, maxdist, superset = _superset(d, seed, slope, rf, c)
    ev_o, log_o = FastEvaluator(nsol, strategy), []
    _, final_o = C.oracle_enumerate(mut, rdiag, pruning, maxdist, ev_o, log_o)
    shuffled = list(superset)
    random.Random(seed + 7).shuffle(shuffled)
    ev = FastEvaluator(nsol, strategy)
    log, final = _replay(lib, L, mut, rdiag, pruning, maxdist, shuffled, ev)
    assert _bits(log) == _bits(log_o)
    assert float(final).hex() == float(final_o).hex()
    assert ev.solutions == ev_o.solutions


def test_replay_of_the_fixed_radius_fixture_gives_the_best1_fixture():
    """The reference's own logs: enum_d32_fixed.json (radius never shrinks) replayed with FastEvaluator(1) is
    enum_d32_best1.json's log."""
    from fplll_amd.enumeration import FastEvaluator
    lib, L = _lib()
    fx = C.load_fixture(os.path.join(C.GOLDEN, "enum_d32_fixed.json"))
    fb = C.load_fixture(os.path.join(C.GOLDEN, "enum_d32_best1.json"))
    assert np.array_equal(fx["mut"], fb["mut"]) and fx["maxdist"] == fb["maxdist"]
    shuffled = list(fx["sol_log"])
    random.Random(5).shuffle(shuffled)
    ev = FastEvaluator(fb["max_sols"], fb["strategy"])
    log, final = _replay(lib, L, np.ascontiguousarray(fx["mut"]), fx["rdiag"], fx["pruning"], fx["maxdist"], shuffled, ev)
    assert _bits(log) == _bits(fb["sol_log"])
    assert final == fb["final_maxdist"]


def test_replay_rejects_a_distance_that_is_not_the_vectors():
    lib, L = _lib()
    mut, rdiag, pruning, maxdist, log = _superset(*BLOCKS[0])
    bad = [(log[0][0] * (1.0 + 2.0 ** -50), log[0][1])]
    d = len(rdiag)
    dist = np.array([bad[0][0]])
    xs = np.array(bad[0][1], dtype=np.float64)
    n = lib.fphip_debug_order_replay(d, ctypes.c_double(maxdist), mut.ctypes.data, rdiag.ctypes.data, None, 1,
                                     dist.ctypes.data, xs.ctypes.data, L.SOL_CB(lambda u, a, s: a), None, None)
    assert n == L.FPHIP_ERROR


@pytest.mark.parametrize("d,seed", [(31, 237), (31, 321), (31, 381)])
def test_levels_shared_with_the_last_solution_are_not_tested_again(d, seed):
    """Blocks on which the replay rule and the stricter "test every level of every candidate against the current
    radius" differ (found by a seeded search with BEST-5): the reference does not test a level again that it entered
    before the radius dropped (enumerate_base.cpp:74-94), so it reports a candidate whose UPPER levels, shared with the
    last solution, would fail under the new radius.  The replay must report it too; the strict rule loses it."""
    from fplll_amd.enumeration import FastEvaluator
    lib, L = _lib()
    mut, rdiag, pruning, maxdist, superset = _superset(d, seed, 0.04, 1.9, 1.0)
    ev_o, log_o = FastEvaluator(5, 0), []
    C.oracle_enumerate(mut, rdiag, pruning, maxdist, ev_o, log_o)
    # the strict rule, in Python, on the superset in the oracle's order
    ev_s, B, strict = FastEvaluator(5, 0), maxdist, []
    for dist, x in superset:
        _, nd = _key(lib, mut, rdiag, x)
        if all(nd[k] <= pruning[k] * B for k in range(d)):
            strict.append((dist, x))
            B = ev_s.eval_sol(x, dist, B)
    assert _bits(strict) != _bits(log_o), "the block no longer separates the two rules"
    shuffled = list(superset)
    random.Random(seed).shuffle(shuffled)
    log, _ = _replay(lib, L, mut, rdiag, pruning, maxdist, shuffled, FastEvaluator(5, 0))
    assert _bits(log) == _bits(log_o)
