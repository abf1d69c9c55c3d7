"""The N-shortest-vectors solver's numbers (profiles/svp_best.md and profiles/svp_best_bench.json, written by this
script):

  * batches of LLL-reduced q-ary lattices (q = 2039, k = d / 2, the lattices of svp_solver_bench.py) at d = 24 and 32:
    fphip_shortest_vectors for K = 1, 8, 64 at the default bound and at 1.5 N0 (N0 the norm of the lattice's shortest
    row), the WAVE route's wall and kernel time per lattice (one launch per batch) against the ENUM route's (one
    enumerator call per lattice: independent of the batch size, so a sample of the batch is timed);
  * the baseline of the K = 1 default-bound line: fphip_shortest_vector(route=wave) on the same lattices — the code path
    this solver leaves untouched — and the ratio of the two kernel times;
  * the node estimate the AUTO route compares with FPHIP_SVP_WAVE_MAX_NODES (fphip_enum_gh_nodes at radius B0), as a
    geometric mean over (at most 64 of) the lattices, next to the WAVE / ENUM ratio: where the two cross for K = 8, 64.

    python tests/perf/svp_best_bench.py [--dims 24,32] [--batch 1024] [--enum-sample 24] [--repeats 3]
                                        [--out profiles/svp_best.md] [--json profiles/svp_best_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from svp_solver_bench import qary  # noqa: E402


def gh_nodes_at(rd, r2):
    """The enumerator's Gaussian-heuristic node estimate (estimate_levels, enum_host.hip) at the squared radius r2."""
    d, tot, sumlog = len(rd), 0.0, 0.0
    for k in range(d - 1, -1, -1):
        sumlog += 0.5 * math.log(rd[k])
        n = d - k
        tot += math.exp(math.log(0.5) + 0.5 * n * math.log(math.pi) - math.lgamma(0.5 * n + 1.0) + 0.5 * n * math.log(r2) - sumlog)
    return tot


def timed(fn, repeats):
    """(best wall seconds, the last result) of `repeats` calls after one warm-up."""
    fn()
    best, out = None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best, out


def measure(a):
    import fplll_amd
    from fplll_amd.gso import MatGSOBatch
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    rows = []
    B = a.batch
    for d in [int(v) for v in a.dims.split(",")]:
        g = MatGSOBatch(ctx, B, d, d)
        g.set_basis(np.stack([qary(d, s) for s in range(B)]))
        st, _ = g.lll()
        assert np.all(st == 1) and np.all(g.update_gso() == 1)
        b = g.get_basis()
        N0 = (b.astype(object) ** 2).sum(axis=2).min(axis=1).astype(np.int64)  # (LLL-reduced q-ary: every row is useful)
        rds = []
        for k in range(min(B, 64)):
            r, e = np.diag(g.get_r_matrix(k)), g.row_expo(k)
            rds.append(np.ldexp(r, (2 * e).astype(np.int32)))
        # the baseline: the one-vector solver on the same lattices
        kms = []
        wall, base = timed(lambda: (g.shortest_vector(route="wave"), kms.append(g.last_kernel_ms))[0], a.repeats)
        assert np.all(base[4] == 1)
        base_row = dict(d=d, batch=B, what="shortest_vector(route=wave)", wall_ms_per_lattice=wall * 1e3 / B,
                        kernel_ms_per_lattice=min(kms[1:]) / B, nodes_per_lattice=float(base[3].mean()))
        rows.append(base_row)
        print("# %s" % json.dumps(base_row), file=sys.stderr, flush=True)
        for factor in (1.0, 1.5):
            bound = None if factor == 1.0 else (N0 * 3) // 2
            radius = N0.astype(float) * factor
            est = float(np.exp(np.mean([math.log(gh_nodes_at(rd, radius[k])) for k, rd in enumerate(rds)])))
            for K in (1, 8, 64):
                kms = []
                wall, out = timed(lambda: (g.shortest_vectors(K, bound_sq=bound, route="wave"), kms.append(g.last_kernel_ms))[0], a.repeats)
                found, sol, vec, norm, nodes, st = out
                assert np.all(st == 1) and np.all(found >= 1)
                m = min(B, a.enum_sample)
                ewall, eo = timed(lambda: g.shortest_vectors(K, first=0, count=m, bound_sq=None if bound is None else bound[:m],
                                                             route="enum"), 1)
                assert np.all(eo[5] == 1) and np.array_equal(eo[3], norm[:m]) and np.array_equal(eo[0], found[:m]), "the routes disagree"
                row = dict(d=d, batch=B, what="shortest_vectors", K=K, bound="N0" if bound is None else "1.5 N0", gh_estimate=est,
                           wave_wall_ms_per_lattice=wall * 1e3 / B, wave_kernel_ms_per_lattice=min(kms[1:]) / B,
                           wave_nodes_per_lattice=float(nodes.mean()), found_mean=float(found.mean()),
                           enum_sample=m, enum_wall_ms_per_lattice=ewall * 1e3 / m, enum_nodes_per_lattice=float(eo[4].mean()))
                if K == 1 and bound is None:
                    assert np.array_equal(norm[:, 0], base[2]), "K = 1 disagrees with shortest_vector"
                    row["kernel_ratio_to_shortest_vector"] = row["wave_kernel_ms_per_lattice"] / base_row["kernel_ms_per_lattice"]
                    row["nodes_ratio_to_shortest_vector"] = row["wave_nodes_per_lattice"] / base_row["nodes_per_lattice"]
                rows.append(row)
                print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
        g.close()
    ctx.close()
    return rows


def crossing(rows, K):
    """Where WAVE ms per lattice = ENUM ms per lattice along the node estimate, every sign change (the estimate does not
    order the ratio monotonically across bounds: under a large bound ENUM pays for every candidate its callback sees)."""
    pts = sorted((r["gh_estimate"], r["wave_wall_ms_per_lattice"] / r["enum_wall_ms_per_lattice"])
                 for r in rows if r.get("K") == K)
    found = []
    for (e0, q0), (e1, q1) in zip(pts, pts[1:]):
        if (q0 - 1.0) * (q1 - 1.0) <= 0 and q0 != q1:
            t = (0.0 - math.log(q0)) / (math.log(q1) - math.log(q0))
            found.append("%.3g (log-log between the estimates %.3g, WAVE / ENUM %.2f, and %.3g, %.2f)" % (
                math.exp(math.log(e0) + t * (math.log(e1) - math.log(e0))), e0, q0, e1, q1))
    if found:
        return "K = %d: the two times are equal at an estimate of %s" % (K, "; and again at ".join(found))
    if all(q < 1.0 for _, q in pts):
        return "K = %d: WAVE is faster at every point measured (estimates %.3g .. %.3g): the runs did not bracket the crossing, it lies above" % (
            K, pts[0][0], pts[-1][0])
    return "K = %d: WAVE is slower at every point measured (estimates %.3g .. %.3g): the runs did not bracket the crossing, it lies below" % (
        K, pts[0][0], pts[-1][0])


def render(rows, out):
    with open(out, "w") as f:
        f.write("# N shortest vectors per lattice: WAVE route against ENUM route\n\n")
        f.write("Written by `tests/perf/svp_best_bench.py`: one box, this change's session, one run (the box noise of DESIGN "
                "section 5, +-10 %%, applies to every time).  LLL-reduced q-ary lattices (q = 2039, k = d / 2, seeds 0 .. batch - 1), "
                "batch %d.  `bound`: N0 = the default (the norm of the lattice's shortest row), 1.5 N0 = a per-lattice `bound_sq`.  "
                "`gh estimate`: geometric mean over (at most 64 of) the lattices of the Gaussian-heuristic node estimate at radius "
                "B0, what the AUTO route compares with FPHIP_SVP_WAVE_MAX_NODES for K > 1 or a caller's bound.  WAVE: one launch per "
                "batch, best of the repeats, times divided by the batch.  ENUM: one enumerator call per lattice, mean over a sample.\n\n" % rows[0]["batch"])
        f.write("| d | K | bound | gh estimate | found (mean) | WAVE wall ms / lattice | WAVE kernel ms / lattice | WAVE nodes / lattice | "
                "ENUM wall ms / lattice (sample) | ENUM nodes / lattice | WAVE / ENUM |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if r["what"] != "shortest_vectors":
                continue
            f.write("| %d | %d | %s | %.3g | %.1f | %.4f | %.4f | %.3g | %.3f (%d) | %.3g | %.2f |\n" % (
                r["d"], r["K"], r["bound"], r["gh_estimate"], r["found_mean"], r["wave_wall_ms_per_lattice"],
                r["wave_kernel_ms_per_lattice"], r["wave_nodes_per_lattice"], r["enum_wall_ms_per_lattice"], r["enum_sample"],
                r["enum_nodes_per_lattice"], r["wave_wall_ms_per_lattice"] / r["enum_wall_ms_per_lattice"]))
        f.write("\nThe baseline of the K = 1 default-bound line, `fphip_shortest_vector(route=wave)` on the same lattices (its code "
                "path is not touched by this solver):\n\n| d | batch | shortest_vector kernel ms / lattice | nodes / lattice | "
                "shortest_vectors K = 1 kernel ms / lattice | nodes / lattice | kernel time ratio | node ratio |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            if "kernel_ratio_to_shortest_vector" in r:
                base = [x for x in rows if x["what"] != "shortest_vectors" and x["d"] == r["d"]][0]
                f.write("| %d | %d | %.4f | %.3g | %.4f | %.3g | %.3f | %.3f |\n" % (
                    r["d"], r["batch"], base["kernel_ms_per_lattice"], base["nodes_per_lattice"], r["wave_kernel_ms_per_lattice"],
                    r["wave_nodes_per_lattice"], r["kernel_ratio_to_shortest_vector"], r["nodes_ratio_to_shortest_vector"]))
        f.write("\nThe K = 1 walk starts at the radius N0 (1 + 2^-30), inclusive, where `fphip_shortest_vector` starts at N0 - 1 with "
                "the shortest row seeded: the node ratio is the cost of that start, the kernel time ratio follows it.\n\n")
        f.write("Where WAVE and ENUM cross (the AUTO default FPHIP_SVP_WAVE_MAX_NODES = 2e5 is kept):\n\n")
        for K in (8, 64):
            f.write("- %s.\n" % crossing(rows, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="24,32")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--enum-sample", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svp_best.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "svp_best_bench.json"))
    ap.add_argument("--from-json", default=None, help="render the profile from the JSON of an earlier run")
    a = ap.parse_args()
    rows = json.load(open(a.from_json))["rows"] if a.from_json else measure(a)
    render(rows, a.out)
    res = dict(bench="svp_best", rows=rows, crossing={str(K): crossing(rows, K) for K in (8, 64)})
    if not a.from_json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
