#!/usr/bin/env python
"""What tracking the transformation matrix u costs the device BKZ drivers (FPHIP_BKZ_TRANSFORM): the workloads of
bkz_bench.py (B q-ary lattices, device LLL then BKZ-beta with empty strategies) and bkzs_bench.py (B copies of a
bkzs_* fixture, BKZ with strategies), each run `reps` times without u (bkz_kernel / bkzs_kernel) and with it
(bkz_kernel_u / bkzs_kernel_u), alternating; kernel times by HIP events.  The runs with u are checked by
u b_in = b_out on lattice 0.  One JSON line.
usage: bkz_transform_bench.py [reps] [d beta B] [Bs fixture-substring]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import conftest as C  # noqa: E402
import fplll_amd  # noqa: E402
from fplll_amd.gso import MatGSOBatch  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
d, beta, B = (int(x) for x in sys.argv[2:5]) if len(sys.argv) > 4 else (60, 16, 512)
Bs = int(sys.argv[5]) if len(sys.argv) > 5 else 1024
which = sys.argv[6] if len(sys.argv) > 6 else "pre_gh"


def qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b


def exact(u, b):
    return np.asarray(u).astype(object).dot(np.asarray(b).astype(object))


ctx = fplll_amd.Context(0)
res = {"reps": reps, "bkz": {"d": d, "beta": beta, "batch": B, "plain_ms": [], "with_u_ms": []},
       "bkzs": {"batch": Bs, "plain_ms": [], "with_u_ms": []}}

# ---- empty strategies: LLL once (without u), then BKZ from the same reduced bases every time
rng = np.random.default_rng(0)
g = MatGSOBatch(ctx, B, d, d)
g.set_basis(np.stack([qary(rng, d, d // 2, 1048583) for _ in range(B)]))
assert np.all(g.lll()[0] == 1)
b_lll = g.get_basis()
g.close()
ref = None
for rep in range(reps):
    for with_u in (False, True):
        g = MatGSOBatch(ctx, B, d, d)
        g.set_basis(b_lll)
        if with_u:
            g.enable_transform()
        st, info = g.bkz(beta, transform=with_u)
        assert np.all(st == 1)
        res["bkz"]["with_u_ms" if with_u else "plain_ms"].append(round(g.last_kernel_ms, 2))
        out = g.get_basis()
        ref = out if ref is None else ref
        assert np.array_equal(out, ref), "the run with u must return the basis of the run without"
        if with_u:
            assert np.array_equal(exact(g.get_transform(0, 1)[0], b_lll[0]), out[0].astype(object))
            res["bkz"]["insertions"] = g.bkz_insert_stats()
        g.close()

# ---- with strategies
f = C.load_bkz_fixture([p for p in C.bkz_strategy_fixtures() if which in p][0])
res["bkzs"]["fixture"] = f["name"]
for rep in range(reps):
    for with_u in (False, True):
        g = MatGSOBatch(ctx, Bs, f["d"], f["n"])
        g.set_basis(np.stack([f["b_in"]] * Bs))
        if with_u:
            g.enable_transform()
        rnd, draws = C.gmp_streams_native(Bs, f["rng_seed"])
        st, info = g.bkz_strategies(f["block_size"], f["strategies"], rnd, f["delta"], f["eta"], max_loops=f["max_loops"],
                                    gh_bnd=bool(f["flags"] & 0x80), bounded_lll=bool(f["flags"] & 0x10),
                                    gh_factor=f["gh_factor"], transform=with_u)
        assert np.all(st == f["status"])
        res["bkzs"]["with_u_ms" if with_u else "plain_ms"].append(round(g.last_kernel_ms, 2))
        out = g.get_basis(0, 1)[0]
        assert np.array_equal(out, f["b_out"])
        if with_u:
            assert np.array_equal(exact(g.get_transform(0, 1)[0], f["b_in"]), out.astype(object))
            res["bkzs"]["insertions"] = g.bkz_insert_stats()
        g.close()
for k in ("bkz", "bkzs"):
    p, w = np.median(res[k]["plain_ms"]), np.median(res[k]["with_u_ms"])
    res[k]["cost_of_u_percent"] = round(100.0 * (w - p) / p, 2)
print(json.dumps(res))
ctx.close()
