"""List mode against the callback path on the same trees (results: profiles/enum_list.md).

  python tests/perf/enum_list_bench.py [--reps 3] [--md]

Blocks: the Leech basis of the reference's test_list_cvp at radius^2 32.5, without a target (98 280 records) and
around the origin (196 561), and the 40-row pruned block of tests/golden/enum_d40_lin20_fixed.json at 1.95 times its
radius (about 10^5 records).

  list      fphip_enum_list: wall time of the call (buffers, walk, copy, sort), kernel time, records/s, nodes/s
  callback  the path a caller had before: fphip_enum_run with a callback that returns the bound unchanged.  The
            callback is C (compiled here with the host compiler), not Python: the interpreter's cost per candidate
            is not part of the old path.

One JSON line per (block, mode), the best of --reps runs; --md prints the table of the profile."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CB_SRC = r"""
#include <stdint.h>
struct keep { double bound; uint64_t calls; double last; };
double keep_cb(void *user, double dist, const double *sol)
{
  struct keep *k = (struct keep *)user;
  k->calls++;
  k->last = dist + sol[0];
  return k->bound;
}
"""


class Keep(ctypes.Structure):
    _fields_ = [("bound", ctypes.c_double), ("calls", ctypes.c_uint64), ("last", ctypes.c_double)]


def blocks():
    import conftest as C
    import list_helpers as H
    mut, rdiag = H.block_of(H.leech_basis())
    f = C.load_fixture(os.path.join(C.GOLDEN, "enum_d40_lin20_fixed.json"))
    return [("leech24 r2=32.5", mut, rdiag, None, 32.5, None),
            ("leech24 r2=32.5 target 0", mut, rdiag, None, 32.5, np.zeros(24)),
            ("d40_lin20 x1.95", f["mut"], f["rdiag"], f["pruning"], f["maxdist"] * 1.95, None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--md", action="store_true")
    a = ap.parse_args()
    import fplll_amd
    from fplll_amd import _lib
    from fplll_amd.enumeration import list_block
    ctx = fplll_amd.Context(0)
    lib = ctx.lib
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "cb.c"), "w") as fh:
        fh.write(CB_SRC)
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", os.path.join(tmp, "cb.so"), os.path.join(tmp, "cb.c")])
    cb = ctypes.cast(ctypes.CDLL(os.path.join(tmp, "cb.so")).keep_cb, _lib.SOL_CB)
    rows = []
    for name, mut, rdiag, pruning, R, target in blocks():
        mut = np.ascontiguousarray(mut, dtype=np.float64)
        rdiag = np.ascontiguousarray(rdiag, dtype=np.float64)
        d = len(rdiag)
        pr = None if pruning is None else np.ascontiguousarray(pruning, dtype=np.float64)
        best = {}
        for rep in range(a.reps + 1):  # (the first run warms the context: buffers, code objects)
            res = list_block(ctx, mut, rdiag, pr, R, target=target, cap=1 << 18)
            got = dict(records=res.count, nodes=res.total_nodes, wall_ms=res.stats.wall_ms, kernel_ms=res.stats.kernel_ms)
            keep = Keep(R, 0, 0.0)
            opts = _lib.EnumOpts()
            if target is not None:
                opts.target = target.ctypes.data
            nodes = np.zeros(d + 1, dtype=np.uint64)
            stats = _lib.EnumStats()
            rc = lib.fphip_enum_run(ctx.handle, d, ctypes.c_double(R), mut.ctypes.data_as(ctypes.c_void_p),
                                    rdiag.ctypes.data_as(ctypes.c_void_p),
                                    None if pr is None else pr.ctypes.data_as(ctypes.c_void_p), ctypes.byref(opts), cb,
                                    _lib.SUBSOL_CB(), ctypes.byref(keep), nodes.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(stats))
            assert rc == 0, ctx.last_error()
            old = dict(records=int(keep.calls), nodes=int(stats.total_nodes), wall_ms=stats.wall_ms,
                       kernel_ms=stats.kernel_ms)
            assert old["records"] == got["records"] and old["nodes"] == got["nodes"], (old, got)
            if rep == 0:
                continue
            for mode, r in (("list", got), ("callback", old)):
                if mode not in best or r["wall_ms"] < best[mode]["wall_ms"]:
                    best[mode] = r
        for mode in ("list", "callback"):
            r = dict(block=name, mode=mode, **best[mode])
            r["records_per_s"] = r["records"] / (r["wall_ms"] * 1e-3)
            r["nodes_per_s_kernel"] = r["nodes"] / (r["kernel_ms"] * 1e-3)
            rows.append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    if a.md:
        print("\n| block | mode | records | nodes | wall ms | kernel ms | records/s (wall) | nodes/s (kernels) |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %s | %d | %d | %.2f | %.2f | %.3g | %.3g |" % (r["block"], r["mode"], r["records"], r["nodes"],
                                                                      r["wall_ms"], r["kernel_ms"], r["records_per_s"],
                                                                      r["nodes_per_s_kernel"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
