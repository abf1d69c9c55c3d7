"""Batched LLL of quadratic forms against the basis kernel on the bases behind the same forms: B distinct
gen_intrel-style lattices per dimension (rows (x_i | e_i), x_i of `bits` bits: ZZ_mat::gen_intrel), the form is
A A^T.  Per dimension: reductions per second of lll_gram_kernel (fphip_gram_lll) and of lll_kernel (fphip_gso_lll) —
kernel time, one warm-up and `reps` timed repetitions each, median and spread — and, when
oracle/_ref/lll_gram_ref_driver is present, the reference's MatGSOGram LLL on one core for the first forms (its
ref_ms field; the reduced forms are checked against the device's).

    python tests/perf/lll_gram_bench.py [batch=1024] [bits=20] [reps=5] [ncheck=2] [d ...=80 120]
"""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fplll_amd
from fplll_amd.gram import MatGSOGramBatch
from fplll_amd.gso import MatGSOBatch


def intrel(rng, d, bits):
    a = np.zeros((d, d + 1), dtype=np.int64)
    a[:, 0] = rng.integers(1, 1 << bits, size=d)
    a[:, 1:] = np.eye(d, dtype=np.int64)
    return a


def timed(run, reps):
    run()  # warm-up
    ms = sorted(run() for _ in range(reps))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ncheck = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    dims = [int(x) for x in sys.argv[5:]] or [80, 120]
    ctx = fplll_amd.Context(0)
    for d in dims:
        rng = np.random.default_rng(d)
        bs = np.stack([intrel(rng, d, bits) for _ in range(B)])
        gs = np.einsum("bik,bjk->bij", bs, bs)
        m = MatGSOGramBatch(ctx, gs)
        res = {}

        def run_gram():
            m.set_gram(gs)
            st, info = m.lll()
            assert np.all(st == 1), np.unique(st, return_counts=True)
            res["info"] = info
            return m.last_kernel_ms
        med, lo, hi = timed(run_gram, reps)
        gout, info = m.gram(), res["info"]
        print("d=%d B=%d bits=%d  Gram kernel:  median %.1f ms (min %.1f, max %.1f) -> %.0f reductions/s; swaps mean %.0f, "
              "iterations mean %.0f" % (d, B, bits, med, lo, hi, B / (med * 1e-3), info[:, 1].mean(), info[:, 3].mean()),
              flush=True)
        m.close()
        g = MatGSOBatch(ctx, B, d, d + 1)

        def run_basis():
            g.set_basis(bs)
            st, binfo = g.lll()
            assert np.all(st == 1), np.unique(st, return_counts=True)
            res["binfo"] = binfo
            return g.last_kernel_ms
        bmed, blo, bhi = timed(run_basis, reps)
        bout = g.get_basis(0, B)
        g.close()
        same = int(np.sum([np.array_equal(bout[k].dot(bout[k].T), gout[k]) for k in range(B)]))
        print("d=%d B=%d bits=%d  basis kernel: median %.1f ms (min %.1f, max %.1f) -> %.0f reductions/s; swaps mean %.0f; "
              "Gram / basis time = %.2f; %d of %d reduced bases have the reduced form as their Gram matrix"
              % (d, B, bits, bmed, blo, bhi, B / (bmed * 1e-3), res["binfo"][:, 1].mean(), med / bmed, same, B), flush=True)
        drv = os.path.join(ROOT, "oracle", "_ref", "lll_gram_ref_driver")
        if os.path.exists(drv) and ncheck > 0:
            ref_ms = []
            for k in range(ncheck):
                txt = "[" + "\n".join("[" + " ".join(str(int(x)) for x in row) + "]" for row in bs[k]) + "]\n"
                r = subprocess.run([drv, "bench", "0.99", "0.51", "0", "A"], input=txt, capture_output=True, text=True,
                                   timeout=600, check=True)
                j = json.loads(r.stdout)
                assert np.array_equal(np.array(j["G_out"], dtype=np.int64), gout[k]), "form %d differs from the reference" % k
                ref_ms.append(j["ref_ms"])
            print("d=%d  reference MatGSOGram LLL (1 core): %.2f ms per form -> %.0f reductions/s; outputs identical on %d "
                  "checked; Gram kernel / reference = %.1fx" % (d, np.mean(ref_ms), 1e3 / np.mean(ref_ms), ncheck,
                                                                 (B / (med * 1e-3)) * np.mean(ref_ms) * 1e-3), flush=True)
    ctx.close()


main()
