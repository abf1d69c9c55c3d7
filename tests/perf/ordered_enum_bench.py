"""What the reference-order mode costs: config 3's beta = 60 blocks (tests/golden/c3_b60_k{0,1,2}_{pruner,linear30}.json),
default mode against ordered mode (fphip_enum_opts::ordered), per block: milliseconds per call (wall time of
fphip_enum_run, median of the timed repeats after warm-up calls), nodes walked, windows, candidates the device
reported, and the reference's node count from the fixture.  One JSON line on stdout.

    python tests/perf/ordered_enum_bench.py [--repeats 7] [--warmup 2] [--kinds pruner,linear30]
                                            [--schedules "1024,8;64,4;256,4;4096,16;0"]

--schedules runs the ordered mode once per FPHIP_ORDER_WINDOWS value (the A/B the default was chosen from); without it
the library's default schedule is measured.  The ordered runs also assert the contract: the log is the fixture's.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest as C  # noqa: E402


def run(ctx, f, ordered, repeats, warmup):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    wall, kern, nodes, res, log = [], [], [], None, None
    for i in range(warmup + repeats):
        ev, log = FastEvaluator(f["max_sols"], f["strategy"]), []
        res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], ev, log=log, ordered=ordered)
        if i >= warmup:
            wall.append(res.stats.wall_ms)
            kern.append(res.stats.kernel_ms)
            nodes.append(res.total_nodes)
    out = dict(ms=statistics.median(wall), ms_min=min(wall), ms_max=max(wall), kernel_ms=statistics.median(kern),
               nodes=int(statistics.median(nodes)), nodes_min=min(nodes), nodes_max=max(nodes),
               final=ev.solutions[0][0] if ev.solutions else None)
    if ordered:
        exact = [(a.hex(), tuple(x)) for a, x in log] == [(a.hex(), tuple(x)) for a, x in f["sol_log"]]
        assert exact, "ordered log differs from the fixture's on " + f["name"]
        out.update(windows=int(res.stats.windows), candidates=int(res.stats.candidates), exact=exact)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kinds", default="pruner,linear30")
    ap.add_argument("--schedules", default="")
    a = ap.parse_args()
    import fplll_amd
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    scheds = [s for s in a.schedules.split(";") if s] or [None]
    blocks = []
    for kind in a.kinds.split(","):
        for k in (0, 1, 2):
            f = C.load_fixture(os.path.join(C.GOLDEN, "c3_b60_k%d_%s.json" % (k, kind)))
            row = dict(block=f["name"], reference_nodes=int(f["total_nodes"]),
                       reference_final=min(s[0] for s in f["sol_log"]))
            os.environ.pop("FPHIP_ORDER_WINDOWS", None)
            row["default"] = run(ctx, f, False, a.repeats, a.warmup)
            row["ordered"] = {}
            for s in scheds:
                if s is None:
                    os.environ.pop("FPHIP_ORDER_WINDOWS", None)
                else:
                    os.environ["FPHIP_ORDER_WINDOWS"] = s
                r = run(ctx, f, True, a.repeats, a.warmup)
                r["ratio_ms"] = r["ms"] / row["default"]["ms"]
                r["ratio_nodes_vs_reference"] = r["nodes"] / row["reference_nodes"]
                row["ordered"][s or "default"] = r
            blocks.append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(dict(bench="ordered_enum", repeats=a.repeats, warmup=a.warmup, blocks=blocks)))


if __name__ == "__main__":
    main()
