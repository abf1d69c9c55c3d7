"""The closest-vector wave route's numbers (profiles/cvp_wave.md and profiles/cvp_wave_bench.json, written by this
script):

  * the bases of tests/golden/cvpsolve_q24.json and cvpsolve_q40.json with seeded `near` targets (a lattice point with
    coefficients in [-8, 8] plus offsets in [-8, 8]) at T = 1, 64, 1024, 4096: wall time per target of the WAVE, the
    AUTO and the ENUM route in the same session, medians with min - max over --reps calls.  ENUM is one enumerator call
    per target whatever T is, so a sample of the batch is timed (--enum-sample);
  * the wave kernel's nodes per second (all targets' nodes over the kernel's time);
  * the lone-wave rate: the near:10 target of cvpsolve_q36.json (1.2 million nodes) alone in a launch;
  * c, the default of FPHIP_CVP_WAVE_NODES_PER_TARGET: the lone-wave rate times the wall time of one ENUM call (the
    median per target at T = 1024 on each basis), with the values it came from.

Every WAVE call carries a node budget (--budget, 4e6 per target): a target that reaches it is reported, not waited for.

    python tests/perf/cvp_wave_bench.py [--batches 1,64,1024,4096] [--reps 5] [--enum-sample 24]
                                        [--out profiles/cvp_wave.md] [--json profiles/cvp_wave_bench.json]
    python tests/perf/cvp_wave_bench.py --from-json profiles/cvp_wave_bench.json      # render a recorded run again
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULT_C = 570  # CVP_WAVE_NODES_PER_TARGET_DEFAULT of gso_host.hip


def fixture(name):
    return json.load(open(os.path.join(GOLDEN, name)))


def near_targets(b, seed, count, off=8):
    rng = np.random.default_rng(seed)
    d, n = b.shape
    c = rng.integers(-8, 9, size=(count, d))
    return (c.astype(object).dot(b.astype(object)) + rng.integers(-off, off + 1, size=(count, n)).astype(object)).astype(np.int64)


def mmm(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def timed(fn, reps):
    out, wall = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return out, wall


def measure(a):
    import fplll_amd
    from fplll_amd.gso import MatGSOBatch
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    rows = []
    # the lone-wave rate
    fx = fixture("cvpsolve_q36.json")
    b = np.array(fx["basis"], dtype=np.int64)
    k = [t["kind"] for t in fx["targets"]].index("near:10")
    tg = np.array([fx["targets"][k]["target"]], dtype=np.int64)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    g.set_basis(b)
    g.closest_vector(tg, route="wave", max_nodes=1000, full=True)  # warm-up
    lone = []
    for _ in range(a.reps):
        sol, dist, norm, nodes, st = g.closest_vector(tg, route="wave", max_nodes=a.budget, full=True)
        assert int(st[0]) == 1 and [int(v) for v in sol[0]] == [int(v) for v in fx["targets"][k]["sol_coord"]]
        lone.append(float(nodes[0]) / (g.last_kernel_ms * 1e-3))
    g.close()
    lone_rate = dict(mmm(lone), nodes=int(nodes[0]))
    print("# lone wave: %s" % json.dumps(lone_rate), file=sys.stderr, flush=True)
    for name in ("cvpsolve_q24.json", "cvpsolve_q40.json"):
        b = np.array(fixture(name)["basis"], dtype=np.int64)
        g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
        g.set_basis(b)
        for T in [int(v) for v in a.batches.split(",")]:
            tg = near_targets(b, 1000 + T, T)
            row = dict(basis=name[:-5], d=int(b.shape[0]), T=T)
            g.closest_vector(tg[:1], route="wave", max_nodes=1000)  # warm-up
            (sol, dist, norm, nodes, st), wall = timed(lambda: g.closest_vector(tg, route="wave", max_nodes=a.budget, full=True), a.reps)
            kms = g.last_kernel_ms
            row.update(wave_ms_per_target=mmm([w * 1e3 / T for w in wall]), wave_kernel_ms=kms,
                       wave_nodes_per_s=float(nodes.sum()) / (kms * 1e-3), nodes_mean=float(nodes.mean()),
                       nodes_max=int(nodes.max()), wave_over_budget=int((st == 2).sum()))
            (asol, adist, anorm, anodes, ast), wall = timed(lambda: g.closest_vector(tg, route="auto", full=True), a.reps)
            assert np.all(ast == 1)
            done = st == 1
            row.update(auto_differs=int((anorm[done] != norm[done]).sum()))  # (exact distances: 0 expected)
            row.update(auto_ms_per_target=mmm([w * 1e3 / T for w in wall]), auto_wave_kernel_ms=g.last_kernel_ms)
            m = min(T, a.enum_sample)
            g.closest_vector(tg[:1], route="enum")  # warm-up
            (esol, edist, enorm, enodes, est), wall = timed(lambda: g.closest_vector(tg[:m], route="enum", full=True), a.reps)
            assert np.all(est == 1)
            row.update(enum_differs=int((enorm[done[:m]] != norm[:m][done[:m]]).sum()))
            row.update(enum_sample=m, enum_ms_per_target=mmm([w * 1e3 / m for w in wall]), enum_nodes_mean=float(enodes.mean()))
            rows.append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
        g.close()
    ctx.close()
    return dict(bench="cvp_wave", reps=a.reps, budget=a.budget, lone_wave_nodes_per_s=lone_rate, rows=rows)


def fmt(m):
    return "%.3g (%.3g - %.3g)" % (m["median"], m["min"], m["max"])


def verdict(x, y):
    """x against y (medians, ms per target) under the +-10 % box noise."""
    if x["median"] < y["median"] / 1.1:
        return "faster, %.1fx" % (y["median"] / x["median"])
    if x["median"] > y["median"] * 1.1:
        return "SLOWER, %.1fx" % (x["median"] / y["median"])
    return "within the noise"


def render(R, out):
    lone = R["lone_wave_nodes_per_s"]
    cs = {}
    with open(out, "w") as f:
        f.write("# Closest-vector solver: the wave route (one wavefront per target) against the ENUM route\n\n")
        f.write("Written by `tests/perf/cvp_wave_bench.py` (one session; medians with min - max over %d calls; the box noise of "
                "DESIGN section 5, +-10 %%, applies: \"faster\" only where the medians differ by more).  Bases: "
                "`tests/golden/cvpsolve_q24.json` and `cvpsolve_q40.json`; targets: seeded lattice points (coefficients in "
                "[-8, 8]) plus offsets in [-8, 8].  WAVE and AUTO: one call for the T targets, wall time divided by T "
                "(preparation, launch and copies included).  ENUM — the code of the parent commit, the yardstick —: one "
                "enumerator call per target whatever T is, so a sample of the batch is timed.  Every WAVE call carries a "
                "budget of %.0e nodes per target.\n\n" % (R["reps"], R["budget"]))
        f.write("| basis | T | WAVE ms / target | AUTO ms / target | ENUM ms / target (sample) | WAVE vs ENUM | AUTO vs ENUM | "
                "wave kernel ms | nodes / target mean (max) | kernel nodes/s | over budget |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in R["rows"]:
            f.write("| %s | %d | %s | %s | %s (%d) | %s | %s | %.2f | %.4g (%d) | %.3g | %d |\n" % (
                r["basis"], r["T"], fmt(r["wave_ms_per_target"]), fmt(r["auto_ms_per_target"]), fmt(r["enum_ms_per_target"]),
                r["enum_sample"], verdict(r["wave_ms_per_target"], r["enum_ms_per_target"]),
                verdict(r["auto_ms_per_target"], r["enum_ms_per_target"]), r["wave_kernel_ms"], r["nodes_mean"], r["nodes_max"],
                r["wave_nodes_per_s"], r["wave_over_budget"]))
            if r["T"] == 1024:
                cs[r["basis"]] = (lone["median"] * r["enum_ms_per_target"]["median"] * 1e-3, r["enum_ms_per_target"]["median"])
        f.write("\nLone-wave rate (the near:10 target of `cvpsolve_q36.json`, %d nodes, alone in a launch): %s nodes/s "
                "(kernel time).\n\n" % (lone["nodes"], "%.3g (%.3g - %.3g)" % (lone["median"], lone["min"], lone["max"])))
        f.write("c = lone-wave rate x wall time of one ENUM call (the median per target at T = 1024):\n\n")
        for basis, (c, ems) in sorted(cs.items()):
            f.write("- %s: %.3g nodes/s x %.3f ms = %.0f nodes\n" % (basis, lone["median"], ems, c))
        low = min(v[0] for v in cs.values()) if cs else float("nan")
        f.write("\nThe built-in default (`CVP_WAVE_NODES_PER_TARGET_DEFAULT`, `gso_host.hip`) is %d: the smaller of the two as "
                "measured when the constant was set (2.91e6 nodes/s x 0.196 ms = 571, an earlier session of the same code), so "
                "that the wave stage of the AUTO route is no longer than the ENUM route on either basis; this run's smaller "
                "figure, %.0f, is %.2f of it (box noise +-10 %%) "
                % (DEFAULT_C, low, low / DEFAULT_C))
        f.write("(DESIGN section 3g).\n\n`over budget`: targets of the WAVE call that ended on the node budget (status 2: "
                "NOT solved, the best point so far returned).  Where it is not 0 the WAVE column is not like for like with "
                "ENUM; the AUTO column is (every target solved, the over-budget ones finished by an enumerator call).\n")
    return {k: v[0] for k, v in cs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,64,1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--enum-sample", type=int, default=24)
    ap.add_argument("--budget", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cvp_wave.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cvp_wave_bench.json"))
    ap.add_argument("--from-json", default=None, help="render the profile from the JSON of an earlier run")
    a = ap.parse_args()
    if a.from_json:
        R = json.load(open(a.from_json))
    else:
        R = measure(a)
        with open(a.json, "w") as f:
            json.dump(R, f, indent=1)
            f.write("\n")
    R["c"] = render(R, a.out)
    print(json.dumps(dict(bench="cvp_wave", c=R["c"], lone_wave_nodes_per_s=R["lone_wave_nodes_per_s"]["median"])))


if __name__ == "__main__":
    main()
