"""The form solver's numbers (profiles/svp_gram.md and profiles/svp_gram_bench.json, written by this script):

  * batches of LLL-reduced q-ary lattices (q = 2039, k = d / 2, the lattices of svp_solver_bench.py) at d = 24 and 32,
    given as FORMS (G = B B^T): fphip_gram_shortest_vectors for K = 1, 8, 64 at the default bound, the WAVE route's
    kernel and wall time per form (one launch per batch);
  * next to each, svp_best_kernel's kernel time per lattice on the SAME lattices given as bases, in the same session:
    once with n = d columns and once with the basis padded with zero columns to n = 256 (the same Gram matrix, the same
    tree; the form's evaluator does not see n);
  * the ENUM route's wall time per form (one enumerator call per form: independent of the batch size, so a sample of
    the batch is timed), and the node estimate the AUTO route compares with FPHIP_SVP_WAVE_MAX_NODES.

    python tests/perf/svp_gram_bench.py [--dims 24,32] [--batch 1024] [--enum-sample 24] [--repeats 3]
                                        [--out profiles/svp_gram.md] [--json profiles/svp_gram_bench.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from svp_best_bench import crossing, gh_nodes_at, timed  # noqa: E402
from svp_solver_bench import qary  # noqa: E402


def measure(a):
    import fplll_amd
    from fplll_amd.gram import MatGSOGramBatch
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
        wide = np.zeros((B, d, 256), dtype=np.int64)
        wide[:, :, :d] = b
        gw = MatGSOBatch(ctx, B, d, 256)
        gw.set_basis(wide)
        G = np.einsum("bij,bkj->bik", b, b)  # (entries below 2039^2 * 32: int64 holds them)
        m = MatGSOGramBatch(ctx, G)
        assert np.all(m.update() == 1)
        r_all = m.r
        N0 = np.array([int(min(np.diag(G[k]))) for k in range(B)], dtype=float)
        est = float(np.exp(np.mean([math.log(gh_nodes_at(np.diag(r_all[k]), N0[k])) for k in range(min(B, 64))])))
        for K in (1, 8, 64):
            kms = []
            wall, out = timed(lambda: (m.shortest_vectors(K, route="wave"), kms.append(m.last_kernel_ms))[0], a.repeats)
            found, sol, norm, nodes, st = out
            assert np.all(st == 1) and np.all(found >= 1)
            kb = []
            _, ob = timed(lambda: (g.shortest_vectors(K, route="wave"), kb.append(g.last_kernel_ms))[0], a.repeats)
            kw = []
            _, ow = timed(lambda: (gw.shortest_vectors(K, route="wave"), kw.append(gw.last_kernel_ms))[0], a.repeats)
            # (the answers are compared by their norms; the node counts are recorded next to each other — on these
            #  lattices they came out equal in every row, mu / r of the form and of the basis being the same doubles)
            assert np.array_equal(ob[3], norm) and np.array_equal(ow[3], norm), "the form and the basis solver disagree"
            ne = min(B, a.enum_sample)
            ewall, eo = timed(lambda: m.shortest_vectors(K, first=0, count=ne, route="enum"), 1)
            assert np.all(eo[4] == 1) and np.array_equal(eo[2], norm[:ne]) and np.array_equal(eo[0], found[:ne]), "the routes disagree"
            row = dict(d=d, batch=B, what="shortest_vectors", K=K, bound="B0", gh_estimate=est,
                       wave_wall_ms_per_lattice=wall * 1e3 / B, wave_kernel_ms_per_lattice=min(kms[1:]) / B,
                       wave_nodes_per_lattice=float(nodes.mean()), found_mean=float(found.mean()),
                       basis_kernel_ms_per_lattice=min(kb[1:]) / B, basis_nodes_per_lattice=float(ob[4].mean()),
                       basis256_kernel_ms_per_lattice=min(kw[1:]) / B,
                       enum_sample=ne, enum_wall_ms_per_lattice=ewall * 1e3 / ne, enum_nodes_per_lattice=float(eo[3].mean()))
            rows.append(row)
            print("# %s" % json.dumps(row), file=sys.stderr, flush=True)
        m.close()
        g.close()
        gw.close()
    ctx.close()
    return rows


def render(rows, out):
    with open(out, "w") as f:
        f.write("# N shortest vectors of quadratic forms: svp_gram_kernel against svp_best_kernel and the ENUM route\n\n")
        f.write("Written by `tests/perf/svp_gram_bench.py`: one box, this change's session, one run (the box noise of DESIGN "
                "section 5, +-10 %%, applies to every time).  LLL-reduced q-ary lattices (q = 2039, k = d / 2, seeds 0 .. batch - 1), "
                "batch %d, given as forms G = B B^T at the default bound (B0 = the smallest diagonal entry).  `basis n = d` and "
                "`basis n = 256`: `svp_best_kernel` on the same lattices given as bases, with d columns and padded with zero "
                "columns to 256 (the same Gram matrix; the form's evaluator does not see n).  WAVE: one launch per batch, best "
                "of the repeats, times divided by the batch.  ENUM: one enumerator call per form, mean over a sample.  `gh "
                "estimate`: geometric mean over (at most 64 of) the forms of the Gaussian-heuristic node estimate at radius B0, "
                "what the AUTO route compares with FPHIP_SVP_WAVE_MAX_NODES.\n\n" % rows[0]["batch"])
        f.write("| d | K | gh estimate | found (mean) | form kernel ms / form | form wall ms / form | form nodes / form | "
                "basis n = d kernel ms / lattice | basis n = 256 kernel ms / lattice | form / basis n = d | form / basis n = 256 | "
                "ENUM wall ms / form (sample) | WAVE / ENUM |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d | %d | %.3g | %.1f | %.4f | %.4f | %.3g | %.4f | %.4f | %.2f | %.2f | %.3f (%d) | %.2f |\n" % (
                r["d"], r["K"], r["gh_estimate"], r["found_mean"], r["wave_kernel_ms_per_lattice"], r["wave_wall_ms_per_lattice"],
                r["wave_nodes_per_lattice"], r["basis_kernel_ms_per_lattice"], r["basis256_kernel_ms_per_lattice"],
                r["wave_kernel_ms_per_lattice"] / r["basis_kernel_ms_per_lattice"],
                r["wave_kernel_ms_per_lattice"] / r["basis256_kernel_ms_per_lattice"],
                r["enum_wall_ms_per_lattice"], r["enum_sample"], r["wave_wall_ms_per_lattice"] / r["enum_wall_ms_per_lattice"]))
        f.write("\nWhere WAVE and ENUM cross for forms (the AUTO default FPHIP_SVP_WAVE_MAX_NODES = 2e5 is the basis solver's "
                "and is NOT retuned for forms in this change; two estimates per K are too few points for a new value):\n\n")
        for K in (1, 8, 64):
            f.write("- %s.\n" % crossing(rows, K))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="24,32")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--enum-sample", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svp_gram.md"))
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "svp_gram_bench.json"))
    ap.add_argument("--from-json", default=None, help="render the profile from the JSON of an earlier run")
    a = ap.parse_args()
    rows = json.load(open(a.from_json))["rows"] if a.from_json else measure(a)
    render(rows, a.out)
    res = dict(bench="svp_gram", rows=rows, crossing={str(K): crossing(rows, K) for K in (1, 8, 64)})
    if not a.from_json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
