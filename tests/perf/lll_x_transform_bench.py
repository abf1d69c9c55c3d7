#!/usr/bin/env python
"""What carrying the transformation matrix u costs lll_ex (fphip_gso_enable_transform under fphip_gso_lll_ex): B raw
d-dimensional q-ary lattices, LLLReduction::lll in double-double (precision 106) and in plain double in tree order
(53), one launch each, run `reps` times without u (lll_x_kernel) and `reps` times with it (lll_x_u_kernel),
alternating; kernel times from last_kernel_ms (HIP events).  The runs with u must return the statuses and the bases of
the runs without, and u b_in = b_out is checked in exact integers on the first and the last lattice.  One JSON line.
A library without the feature (the parent commit's: lll_ex refuses a tracked u) gives the plain figures alone.
usage: lll_x_transform_bench.py [reps] [d] [B] [precision ...]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import fplll_amd  # noqa: E402
from fplll_amd.gso import MatGSOBatch  # noqa: E402


def qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b


def exact(u, b):
    return np.asarray(u).astype(object).dot(np.asarray(b).astype(object))


def carries_u(ctx):
    g = MatGSOBatch(ctx, 1, 4, 4)
    try:
        g.set_basis(np.array([[[5, 1, 0, 0], [0, 7, 1, 0], [0, 0, 9, 1], [3, 0, 0, 11]]], dtype=np.int64))
        g.enable_transform()
        g.lll_ex(53)
        return True
    except fplll_amd.HipError:
        return False
    finally:
        g.close()


def measure(reps=3, d=80, B=1024, precisions=(106, 53)):
    ctx = fplll_amd.Context(0)
    has_u = carries_u(ctx)
    rng = np.random.default_rng(0)
    bs = np.stack([qary(rng, d, d // 2, 1048583) for _ in range(B)])
    res = {"d": d, "batch": B, "reps": reps, "carries_u": has_u}
    for prec in precisions:
        r = {"plain_ms": [], "with_u_ms": []}
        ref = None
        for rep in range(reps):
            for with_u in ((False, True) if has_u else (False,)):
                g = MatGSOBatch(ctx, B, d, d)
                g.set_basis(bs)
                if with_u:
                    g.enable_transform()
                st, info = g.lll_ex(prec)
                r["with_u_ms" if with_u else "plain_ms"].append(round(g.last_kernel_ms, 1))
                out = g.get_basis(0, B)
                ref = (st, out) if ref is None else ref
                assert np.array_equal(st, ref[0]) and np.array_equal(out, ref[1]), \
                    "the run with u must return the statuses and the bases of the run without"
                if with_u:
                    for L in (0, B - 1):
                        assert np.array_equal(exact(g.get_transform(L, 1)[0], bs[L]), out[L].astype(object)), L
                r["status_1"] = int(np.count_nonzero(st == 1))
                r["swaps_mean"] = round(float(info[:, 1].mean()), 1)
                g.close()
        p = float(np.median(r["plain_ms"]))
        r["plain_lattices_per_s"] = round(B / (p * 1e-3), 1)
        if r["with_u_ms"]:
            w = float(np.median(r["with_u_ms"]))
            r["with_u_lattices_per_s"] = round(B / (w * 1e-3), 1)
            r["with_u_over_plain"] = round(w / p, 4)
        res[str(prec)] = r
    ctx.close()
    return res


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    print(json.dumps(measure(*a[:3], **({"precisions": tuple(a[3:])} if len(a) > 3 else {}))))
