#!/usr/bin/env python
"""What carrying the transformation matrix u costs the batched HLLL (fphip_hh_enable_transform): the workload of
README's HLLL line (B raw 80-dimensional q-ary lattices, HLLLReduction::hlll in double, one launch — bench.py's
hlll_batch), run `reps` times without u (hlll_kernel) and `reps` times with it (hlll_u_kernel), alternating; kernel
times from last_kernel_ms (HIP events).  The runs with u must return the basis of the runs without, and
u b_in = b_out is checked in exact integers on the first and the last lattice.  One JSON line.
A library without the feature (the parent commit's) gives the plain figures alone.
usage: hlll_transform_bench.py [reps] [d] [B]"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import fplll_amd  # noqa: E402
from fplll_amd.householder import MatHouseholderBatch  # noqa: E402


def qary(rng, d, k, q):
    b = np.zeros((d, d), dtype=np.int64)
    b[:k, :k] = np.eye(k, dtype=np.int64)
    b[:k, k:] = rng.integers(0, q, size=(k, d - k))
    b[k:, k:] = q * np.eye(d - k, dtype=np.int64)
    return b


def exact(u, b):
    return np.asarray(u).astype(object).dot(np.asarray(b).astype(object))


def measure(reps=3, d=80, B=1024):
    ctx = fplll_amd.Context(0)
    has_u = hasattr(ctx.lib, "fphip_hh_enable_transform")
    rng = np.random.default_rng(0)
    bs = np.stack([qary(rng, d, d // 2, 1048583) for _ in range(B)])
    res = {"d": d, "batch": B, "reps": reps, "plain_ms": [], "with_u_ms": []}
    ref = None
    for rep in range(reps):
        for with_u in ((False, True) if has_u else (False,)):
            h = MatHouseholderBatch(ctx, B, d, d, row_expo=True)
            h.set_basis(bs)
            if with_u:
                h.enable_transform()
            st, info = h.hlll()
            assert np.all(st == 1), np.unique(st, return_counts=True)
            res["with_u_ms" if with_u else "plain_ms"].append(round(h.last_kernel_ms, 1))
            out = h.get_basis(0, B)
            ref = out if ref is None else ref
            assert np.array_equal(out, ref), "the run with u must return the basis of the run without"
            if with_u:
                for L in (0, B - 1):
                    assert np.array_equal(exact(h.get_transform(L, 1)[0], bs[L]), out[L].astype(object)), L
            res["swaps_mean"] = round(float(info[:, 0].mean()), 1)
            h.close()
    p = float(np.median(res["plain_ms"]))
    res["plain_lattices_per_s"] = round(B / (p * 1e-3), 1)
    if res["with_u_ms"]:
        w = float(np.median(res["with_u_ms"]))
        res["with_u_lattices_per_s"] = round(B / (w * 1e-3), 1)
        res["with_u_over_plain"] = round(w / p, 4)
    ctx.close()
    return res


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:4]]
    print(json.dumps(measure(*a)))
