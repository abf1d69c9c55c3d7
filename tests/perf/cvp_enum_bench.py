"""Throughput of the closest-vector mode (fphip_enum_opts::target): nodes/s and milliseconds per call, for

  * the d = 40 recorded runs of the reference (tests/golden/cvp_d40_real.json, cvp_d40_stair.json) at their fixed
    radius (every candidate kept) — the counts are checked against the fixture on the way — and
  * a beta = 60 block of config 3 (tests/golden/c3_b60_k0_pruner.json: its mu, r and the pruner's coefficients) around
    a seeded real target at radius^2 = 1.05 GH^2, under a BEST_N(1) evaluator (the radius shrinks), next to the
    shortest-vector call on the same block and radius for scale.

Wall time of fphip_enum_run, median of the timed repeats after warm-up calls.  One JSON line on stdout.

    python tests/perf/cvp_enum_bench.py [--repeats 5] [--warmup 2]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest as C  # noqa: E402


def timed(ctx, mut, rdiag, pruning, maxdist, target, max_sols, repeats, warmup, want_nodes=None):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    wall, kern, nodes, ev = [], [], [], None
    for i in range(warmup + repeats):
        ev = FastEvaluator(max_sols, 0)
        res = enumerate_block(ctx, mut, rdiag, pruning, maxdist, ev, target=target)
        if want_nodes is not None:
            assert [int(v) for v in res.nodes] == want_nodes, "per-level counts differ from the fixture's"
        if i >= warmup:
            wall.append(res.stats.wall_ms)
            kern.append(res.stats.kernel_ms)
            nodes.append(sum(int(v) for v in res.nodes if int(v) < 2**63))
    ms, n = statistics.median(wall), int(statistics.median(nodes))
    return dict(ms=ms, ms_min=min(wall), ms_max=max(wall), kernel_ms=statistics.median(kern), nodes=n,
                nodes_per_s=n / (ms * 1e-3), best=ev.solutions[0][0] if ev.solutions else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import fplll_amd
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    rows = []
    for name in ("cvp_d40_real", "cvp_d40_stair"):
        with open(os.path.join(C.GOLDEN, name + ".json")) as fh:
            j = json.load(fh)
        d = j["d"]
        r = timed(ctx, C.hexvec(j["mut"]).reshape(d, d), C.hexvec(j["rdiag"]), C.hexvec(j["pruning"]),
                  float.fromhex(j["maxdist"]), C.hexvec(j["target"]), 10**9, a.repeats, a.warmup,
                  want_nodes=[int(v) for v in j["nodes"]])
        rows.append(dict(block=name, mode="cvp, fixed radius", **r))
        print("# %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    f = C.load_fixture(os.path.join(C.GOLDEN, "c3_b60_k0_pruner.json"))
    d = f["d"]
    gh2 = math.exp((2.0 / d) * math.lgamma(d / 2.0 + 1.0) - math.log(math.pi) + float(np.log(f["rdiag"]).mean()))
    target = np.random.default_rng(60).uniform(-4.0, 4.0, size=d)
    for mode, t in (("cvp, BEST_N(1)", target), ("svp, BEST_N(1)", None)):
        r = timed(ctx, f["mut"], f["rdiag"], f["pruning"], 1.05 * gh2, t, 1, a.repeats, a.warmup)
        rows.append(dict(block=f["name"] + " at 1.05 GH^2", mode=mode, **r))
        print("# %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(dict(bench="cvp_enum", repeats=a.repeats, warmup=a.warmup, rows=rows)))


if __name__ == "__main__":
    main()
