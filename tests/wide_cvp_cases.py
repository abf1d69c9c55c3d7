"""Closest-vector enumeration of blocks above 64 rows: the named inputs of tests/test_enum_cvp_wide_{cpu,gpu}.py.

  * ``wide_cvp_block(d, seed)``: a dyadic block with a dyadic target (the exactness argument of exact_cvp.py holds:
    mu and the target are multiples of 1/4, r_ii powers of two, every partial distance a multiple of 2^-6 below 2^10)
    that is NARROW — the exact rational reference walks it in a few thousand nodes — and still branches above level
    64: the target is a lattice point x* moved by 1/2 along two rows >= 64 that touch no other row (each doubles the
    closest vectors: four tie at the smallest distance), by 1/4 along three more rows, and a handful of "unit-ish" rows
    >= 64 have r = 1/4, so that +-1 (and +-2) off x* there is affordable: those subtrees die a few levels further down,
    where the shifted centres meet rows of r = 4.
  * the recorded runs of the reference, tests/golden/cvpw_*.json.gz (tests/native/cvp_ref_driver.cpp through
    tests/golden/make_cvp_wide_fixtures.sh), decoded once.
"""
import glob
import gzip
import json
import os

import numpy as np

import exact_cvp as X
import exact_enum as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOP_TASK_CAP = 32768  # the top walk's task buffer (FPHIP_TOP_TASK_CAP's default)

# name -> (d, seed, tie rows, quarter rows, cheap rows); R = 2
WIDE_BLOCKS = {
    "w72": (72, 3, (66, 70), (5, 30, 68), (64, 65, 67, 69, 71)),     # NQT = 2
    "w136": (136, 4, (70, 130), (7, 50, 100), (64, 66, 90, 120, 135)),  # NQT = 4, the stack in global memory
}
R_WIDE = 2.0


def wide_cvp_block(name):
    """(mut, rdiag, None, R, target) of a named block."""
    d, seed, ties, quarters, cheap = WIDE_BLOCKS[name]
    mut, _ = E.dyadic_block(d, seed, q=4, rexp=(0,))
    mut = mut.copy()
    rdiag = np.full(d, 4.0)
    for k in cheap + ties:
        rdiag[k] = 0.25
    for k in ties:
        mut[:k, k] = 0.0  # mu(k, j) = 0 for j < k: the row touches no centre below it
    rng = np.random.default_rng(seed + 7000)
    xs = rng.integers(-3, 4, size=d).astype(np.float64)
    target = np.array([xs[i] + sum(xs[j] * mut[i, j] for j in range(i + 1, d)) for i in range(d)])
    for k in ties:
        target[k] += 0.5
    for k in quarters:
        target[k] += 0.25
    return mut, rdiag, None, R_WIDE, target


_exact = {}


def exact_of(name):
    """exact_cvp_enumerate of a named block, once per process (read-only)."""
    if name not in _exact:
        mut, rdiag, pruning, R, target = wide_cvp_block(name)
        _exact[name] = X.exact_cvp_enumerate(mut, rdiag, pruning, R, target, max_nodes=30000)
    return _exact[name]


def hexvec(a):
    return np.array([float.fromhex(v) for v in a], dtype=np.float64)


FIXTURES = sorted(os.path.basename(p)[:-8] for p in glob.glob(os.path.join(GOLDEN, "cvpw_*.json.gz")))
_fixtures = {}


def fixture(name):
    """A recorded run of the reference (cvp_ref_driver's JSON), decoded once per process (read-only)."""
    if name not in _fixtures:
        with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rt") as fh:
            j = json.load(fh)
        d = j["d"]
        _fixtures[name] = dict(
            name=name, d=d, desc=j["desc"], mut=hexvec(j["mut"]).reshape(d, d), rdiag=hexvec(j["rdiag"]),
            pruning=hexvec(j["pruning"]), target=hexvec(j["target"]), maxdist=float.fromhex(j["maxdist"]),
            nodes=[int(v) for v in j["nodes"]],
            cands=sorted((float.fromhex(s["dist"]), tuple(float(v) for v in s["x"])) for s in j["sol_log"]),
            best=None if j["best"] is None else (float.fromhex(j["best"]["dist"]),
                                                 tuple(float(v) for v in j["best"]["x"])))
    return _fixtures[name]


def descent_stop(f):
    """k0 of a fixture: the level at which prepare_enumeration's rounding descent leaves the radius (0: never)."""
    d, x, nd, k = f["d"], np.zeros(f["d"]), 0.0, f["d"] - 1
    while k >= 0 and nd <= f["maxdist"]:
        c = f["target"][k]
        for j in range(k + 1, d):
            c -= x[j] * f["mut"][k, j]
        t = np.trunc(c)
        x[k] = t + (np.copysign(1.0, c) if abs(c - t) >= 0.5 else 0.0)
        nd += (x[k] - c) * (x[k] - c) * f["rdiag"][k]
        k -= 1
    return k + 1


def safe_under_own_distance(f, dist, x):
    """Every partial distance of candidate x passes pruning_k * dist (the walk's operand order): a BEST_N(1) run whose
    radius has shrunk to `dist` still visits x, whatever the order of the walk."""
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
