"""The closest-vector solver's numbers (profiles/cvp_solver.md):

  * the preparation kernel (fphip_cvp_prepare) over T = 4096 targets against the d = 40 solver fixture's basis and a
    72 x 72 q-ary basis: kernel time (HIP events) and the algorithmic bytes per second — per target and pass, the
    wave-uniform operands the loops read (d n + d (d - 1) + d doubles of basis, mu and r; n d int64 of the basis in
    the subtraction) plus its own vectors — over that time;
  * wall time per closest_vector call on the five known-answer cases and the d = 40 fixture's targets, next to the
    reference's time recorded in the fixture (one core of ANOTHER machine);
  * nodes/s of the recorded closest-vector runs above 64 rows (cvpw_d96_k0, cvpw_d136_k0, cvpw_d72_real) at their fixed
    radius, next to a shortest-vector call (no target) on the same block and radius.

Median of the timed repeats after warm-up calls.  One JSON line on stdout.

    python tests/perf/cvp_solver_bench.py [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

os.environ.setdefault("FPHIP_CVP_WIDE", "1")  # closest-vector calls above 64 rows are opt-in
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cvp_solver_cases as S  # noqa: E402
import wide_cvp_cases as W  # noqa: E402


def targets_around(b, seed, count):
    rng = np.random.default_rng(seed)
    d, n = b.shape
    c = rng.integers(-8, 9, size=(count, d))
    return (c.astype(object).dot(b.astype(object)) + rng.integers(-6, 7, size=(count, n)).astype(object)).astype(np.int64)


def prepare_rows(ctx, a):
    from fplll_amd.gso import MatGSOBatch, lll_reduction
    rows = []
    b40 = S.basis_of(S.load("cvpsolve_q40.json"))
    rng = np.random.default_rng(72)
    b72 = np.zeros((72, 72), dtype=np.int64)
    b72[:36, :36] = np.eye(36, dtype=np.int64)
    b72[:36, 36:] = rng.integers(0, 2039, size=(36, 36))
    b72[36:, 36:] = 2039 * np.eye(36, dtype=np.int64)
    b72, _, status, _ = lll_reduction(ctx, b72, with_u=False)
    assert status == 1
    for name, b in (("q40 (40 x 40)", b40), ("q-ary 72 x 72", b72)):
        d, n = b.shape
        T = 4096
        tg = targets_around(b, 5, T)
        g = MatGSOBatch(ctx, 1, d, n)
        g.set_basis(b)
        assert g.update_gso()[0] == 1
        mu, rd = S.true_values(g.get_mu_matrix(0), g.get_r_matrix(0), g.row_expo(0))
        passes = int(S.prepare(b, mu, rd, tg[:64])["passes"].max())
        ms = []
        for i in range(a.warmup + a.repeats):
            coef, tc, desc, st = g.cvp_prepare(tg)
            assert np.all(st == 1)
            if i >= a.warmup:
                ms.append(g.last_kernel_ms)
        g.close()
        per_pass = 8 * (d * n + d * (d - 1) + d) + 8 * n * d + 8 * (3 * n + 4 * d)
        byts = T * passes * per_pass
        m = statistics.median(ms)
        rows.append(dict(basis=name, T=T, passes=passes, kernel_ms=m, ms_min=min(ms), ms_max=max(ms),
                         algorithmic_bytes=byts, bytes_per_s=byts / (m * 1e-3), targets_per_s=T / (m * 1e-3)))
        print("# %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def solver_rows(ctx, a):
    from fplll_amd.cvp import closest_vector
    rows = []

    def timed(b, t, reduce):
        w = []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            closest_vector(ctx, b, t, reduce=reduce)
            if i >= a.warmup:
                w.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(w)

    for c in S.load("kat_cvp.json")["cases"]:
        rows.append(dict(case=c["name"], d=c["d"], wall_ms=timed(c["basis"], c["target"], True), includes="lll_reduction",
                         ref_ms=None))
    fx = S.load("cvpsolve_q40.json")
    b = S.basis_of(fx)
    for k, t in enumerate(fx["targets"]):
        rows.append(dict(case="cvpsolve_q40 " + t["kind"], d=40, wall_ms=timed(b, S.targets_of(fx)[k], False),
                         includes="closest_vector only", ref_ms=t["ref_ms"]))
    for r in rows:
        print("# %s" % json.dumps(r), file=sys.stderr, flush=True)
    return rows


def wide_rows(ctx, a):
    from fplll_amd.enumeration import FastEvaluator, enumerate_block
    rows = []
    for name in ("cvpw_d96_k0", "cvpw_d136_k0", "cvpw_d72_real"):
        f = W.fixture(name)
        for mode, target in (("cvp", f["target"]), ("svp", None)):
            wall, nodes = [], 0
            for i in range(a.warmup + a.repeats):
                res = enumerate_block(ctx, f["mut"], f["rdiag"], f["pruning"], f["maxdist"], FastEvaluator(10**9, 0),
                                      target=target)
                if target is not None:
                    assert [int(v) for v in res.nodes] == f["nodes"]
                nodes = sum(int(v) for v in res.nodes if int(v) < 2**63)
                if i >= a.warmup:
                    wall.append(res.stats.wall_ms)
            m = statistics.median(wall)
            rows.append(dict(block=name, mode=mode, nodes=nodes, wall_ms=m, ms_min=min(wall), ms_max=max(wall),
                             nodes_per_s=nodes / (m * 1e-3), ns_per_node=m * 1e6 / max(nodes, 1)))
            print("# %s" % json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import fplll_amd
    ctx = fplll_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    out = dict(bench="cvp_solver", repeats=a.repeats, warmup=a.warmup, prepare=prepare_rows(ctx, a),
               solver=solver_rows(ctx, a), wide=wide_rows(ctx, a))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
