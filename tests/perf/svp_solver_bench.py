"""The shortest-vector solver's numbers (profiles/svp_solver.md, written by this script):

  * batches of LLL-reduced q-ary lattices (q = 2039, k = d / 2) at d = 32, 40, 48: the WAVE route's wall and kernel
    time per lattice and its nodes/s (fphip_shortest_vector, one launch per batch);
  * the ENUM route on lattices of the same batches, per lattice (one enumerator call each: independent of the batch
    size, so a sample of the batch is timed);
  * the reference's one-core milliseconds recorded in tests/golden/svpsolve_*.json (another machine's core);
  * the AUTO threshold: the Gaussian-heuristic node estimate (radius min(r_00, GH^2), what the AUTO route computes) at which the
    WAVE time per lattice at the largest batch equals the ENUM time per lattice, interpolated over the dimensions in
    log-log.

A lone wavefront walks a few million nodes a second, so a configuration whose WAVE launch is predicted (from the batch
of 16 of the same dimension) to run longer than --cap seconds is not launched and says so in the table.

    python tests/perf/svp_solver_bench.py [--dims 32,40,48] [--batches 256,1024] [--enum-sample 24] [--cap 150]
                                          [--out profiles/svp_solver.md]
    python tests/perf/svp_solver_bench.py --from-json profiles/svp_solver_bench.json     # render a recorded run again
"""
import argparse
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
Q = 2039  # a prime of 11 bits


def qary(d, seed):
    k = d // 2
    rng = np.random.default_rng(100000 * d + seed)
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, Q, size=(k, d - k))
    b[k:, k:] = Q * np.eye(d - k, dtype=np.int64)
    return b


def gh_nodes(rd):
    """The enumerator's Gaussian-heuristic node estimate (estimate_levels, enum_host.hip) at the radius the AUTO route
    uses: min(r_00, GH^2), GH the Gaussian-heuristic length of the lattice."""
    d, tot, sumlog = len(rd), 0.0, 0.0
    gh2 = math.exp((2.0 / d) * (math.lgamma(0.5 * d + 1.0) - 0.5 * d * math.log(math.pi) + 0.5 * sum(math.log(v) for v in rd)))
    r2 = min(rd[0], gh2)
    for k in range(d - 1, -1, -1):
        sumlog += 0.5 * math.log(rd[k])
        n = d - k
        tot += math.exp(math.log(0.5) + 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1.0) + 0.5 * n * math.log(r2) - sumlog)
    return tot


def reduced_batch(ctx, d, B):
    from fplll_amd.gso import MatGSOBatch
    g = MatGSOBatch(ctx, B, d, d)
    g.set_basis(np.stack([qary(d, s) for s in range(B)]))
    st, _ = g.lll()
    assert np.all(st == 1)
    assert np.all(g.update_gso() == 1)
    est = []
    for k in range(min(B, 64)):
        r, e = np.diag(g.get_r_matrix(k)), g.row_expo(k)
        est.append(gh_nodes(np.ldexp(r, (2 * e).astype(np.int32))))
    return g, float(np.exp(np.mean(np.log(est)))), float(max(est))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="32,40,48")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--enum-sample", type=int, default=24)
    ap.add_argument("--cap", type=float, default=150.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svp_solver.md"))
    ap.add_argument("--from-json", default=None, help="render the profile from the JSON line of an earlier run")
    a = ap.parse_args()
    if a.from_json:
        rows = json.load(open(a.from_json))["rows"]
        thr, how = render(rows, a.out)
    else:
        rows = measure(a)
        thr, how = render(rows, a.out)
    print(json.dumps(dict(bench="svp_solver", rows=rows, threshold=thr, threshold_note=how)))


def measure(a):
    import fplll_amd
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    cus = 256
    rows = []
    for d in [int(v) for v in a.dims.split(",")]:
        slots = cus * min(8, (160 * 1024) // (4 * 8 * (d * (d + 1) // 2 + 2 + max(d * (d - 1) // 2, 2)))) * 4
        t16 = None
        for B in [16] + [int(v) for v in a.batches.split(",")]:
            g, est, est_max = reduced_batch(ctx, d, B)
            row = dict(d=d, batch=B, gh_estimate=est, gh_estimate_max=est_max)
            rounds = -(-B // slots)
            if t16 is None and est_max / 2.5e6 > a.cap:  # (a lone wave walks about 2.5e6 nodes a second)
                row["wave"] = "not launched: the largest estimate, %.3g nodes, is %.0f s of one wave" % (est_max, est_max / 2.5e6)
                t16 = est_max / 2.5e6
            elif t16 is not None and t16 * rounds * 1.5 > a.cap:
                row["wave"] = "not launched: predicted %.0f s (batch of 16: %.1f s)" % (t16 * rounds * 1.5, t16)
            else:
                t0 = time.perf_counter()
                sol, vec, norm, nodes, st = g.shortest_vector(route="wave")
                wall = time.perf_counter() - t0
                assert np.all(st == 1)
                kms = g.last_kernel_ms
                row.update(wave_wall_ms_per_lattice=wall * 1e3 / B, wave_kernel_ms_per_lattice=kms / B, wave_kernel_ms=kms,
                           wave_nodes=int(nodes.sum()), wave_nodes_per_s=float(nodes.sum()) / (kms * 1e-3),
                           wave_nodes_per_lattice=float(nodes.mean()), wave_nodes_max=int(nodes.max()))
                if B == 16:
                    t16 = kms * 1e-3
            m = min(B, a.enum_sample)
            g.shortest_vector(first=0, count=1, route="enum")  # warm-up
            t0 = time.perf_counter()
            es = g.shortest_vector(first=0, count=m, route="enum")
            ewall = time.perf_counter() - t0
            assert np.all(es[4] == 1)
            if "wave" not in row:
                assert np.array_equal(es[2], norm[:m]), "the routes disagree on a norm"
            row.update(enum_sample=m, enum_wall_ms_per_lattice=ewall * 1e3 / m, enum_nodes_per_lattice=float(es[3].mean()))
            g.close()
            rows.append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    return rows


def render(rows, out):
    per_dim = {}
    for r in rows:  # (ascending batches: the largest batch launched per dimension stays)
        if "wave" not in r:
            per_dim[r["d"]] = r
    # the threshold: where wave ms per lattice (largest batch launched) = enum ms per lattice, log-log over the dimensions
    pts = sorted((r["gh_estimate"], r["wave_wall_ms_per_lattice"] / r["enum_wall_ms_per_lattice"]) for r in per_dim.values())
    thr, how = None, ""
    for (e0, q0), (e1, q1) in zip(pts, pts[1:]):
        if (q0 - 1.0) * (q1 - 1.0) <= 0 and q0 != q1:
            t = (0.0 - math.log(q0)) / (math.log(q1) - math.log(q0))
            thr = math.exp(math.log(e0) + t * (math.log(e1) - math.log(e0)))
            how = "interpolated between the estimates %.3g and %.3g" % (e0, e1)
    if thr is None and pts:
        if all(q < 1.0 for _, q in pts):
            how = "WAVE is faster per lattice at every dimension measured: the crossing lies above the estimate %.3g" % pts[-1][0]
        else:
            how = "WAVE is slower per lattice at every dimension measured: the crossing lies below the estimate %.3g" % pts[0][0]
    fixtures = []
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "svpsolve_q*.json"))):
        fx = json.load(open(p))
        fixtures.append((os.path.basename(p), fx["d"], fx["fast"]["ref_ms"], fx["proved"]["ref_ms"]))
    with open(out, "w") as f:
        f.write("# Shortest-vector solver: WAVE route against ENUM route\n\n")
        f.write("Written by `tests/perf/svp_solver_bench.py` (one run; the box noise of DESIGN section 5, +-10 %, applies to every "
                "time).  LLL-reduced q-ary lattices (q = 2039, k = d / 2, seeds 0 .. batch - 1).  `gh estimate`: geometric mean of "
                "the Gaussian-heuristic node estimate at radius min(r_00, GH^2) over (at most 64 of) the lattices, the quantity the AUTO route "
                "compares with its threshold.  WAVE: one launch per batch, times divided by the batch.  ENUM: one enumerator call "
                "per lattice, mean over a sample of the same batch (independent of the batch size).\n\n")
        f.write("| d | batch | gh estimate | WAVE wall ms / lattice | WAVE kernel ms / lattice | WAVE kernel ms | WAVE nodes / lattice "
                "(max) | WAVE nodes/s | ENUM wall ms / lattice (sample) | ENUM nodes / lattice |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "wave" in r:
                f.write("| %d | %d | %.3g | %s | | | | | %.3f (%d) | %.3g |\n" % (r["d"], r["batch"], r["gh_estimate"], r["wave"],
                                                                                r["enum_wall_ms_per_lattice"], r["enum_sample"],
                                                                                r["enum_nodes_per_lattice"]))
            else:
                f.write("| %d | %d | %.3g | %.3f | %.3f | %.1f | %.3g (%.3g) | %.3g | %.3f (%d) | %.3g |\n" % (
                    r["d"], r["batch"], r["gh_estimate"], r["wave_wall_ms_per_lattice"], r["wave_kernel_ms_per_lattice"],
                    r["wave_kernel_ms"], r["wave_nodes_per_lattice"], r["wave_nodes_max"], r["wave_nodes_per_s"],
                    r["enum_wall_ms_per_lattice"], r["enum_sample"], r["enum_nodes_per_lattice"]))
        f.write("\n")
        for d, r in sorted(per_dim.items()):
            q = r["wave_wall_ms_per_lattice"] / r["enum_wall_ms_per_lattice"]
            f.write("- d = %d, batch %d: WAVE %.3f ms per lattice against ENUM %.3f ms: WAVE %s.\n" % (
                d, r["batch"], r["wave_wall_ms_per_lattice"], r["enum_wall_ms_per_lattice"],
                "is %.1f times faster" % (1 / q) if q < 1 else "does NOT beat ENUM, it is %.1f times slower" % q))
        f.write("- The WAVE kernel's time is that of its slowest lattice (one lone wavefront walks 2.5 to 3 million nodes a "
                "second, whatever the batch): the nodes/s column grows with the batch because more waves run side by side, and a "
                "batch of 16 is slower per lattice than ENUM already at d = 32.\n")
        f.write("\nAUTO threshold (node estimate at which the two times per lattice are equal, largest batch launched per "
                "dimension): %s%s.\n\n" % ("%.3g, " % thr if thr else "", how))
        f.write("The reference on one core (recorded in the fixtures on another machine, `shortest_vector` alone):\n\n"
                "| fixture | d | SVPM_FAST ms | SVPM_PROVED ms |\n|---|---|---|---|\n")
        for name, d, fm, pm in fixtures:
            f.write("| %s | %d | %.1f | %.1f |\n" % (name, d, fm, pm))
    return thr, how


if __name__ == "__main__":
    main()
