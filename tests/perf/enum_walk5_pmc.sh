#!/bin/bash
# Counters-only PMC passes (no tracing in the same run) over the enumeration-only bench, one step each; per pass the
# counters summed over the dispatches of the walk kernels of every generation (enum_phase_kernel, enum_walk_kernel,
# enum_walk4_kernel, enum_walk5_kernel) and the per-node figures (counter / nodes of the step).
# enum_walk4_pmc.sh with the fifth generation's kernel name summed as well (enum_walk5_kernel, enum_walk5.hip): the same
# counter sets (passes 1-3 of enum_lds_pmc.sh), the same summary, counters only, no tracing of any kind beside --pmc.
# A script of its own so that the older one stays what the earlier profiles were collected with.  A change to the
# counter sets belongs in all three.
#   tests/perf/enum_walk5_pmc.sh [OUT]     (run from the checkout whose bench.py and library are measured)
# Passes 1 and 2: the instruction mix; pass 3: the LDS unit.  Every pass runs under its own time limit, and nothing is
# started behind a pass that failed.
export TMPDIR=${TMPDIR:-/tmp}
OUT=${1:-$TMPDIR/enum_walk5_pmc}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
B="python bench.py --no-cpu --no-gso --no-tour --no-pmc --no-batch --steps 1 --warmup 0"
P1="SQ_BUSY_CYCLES SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAVES SQ_WAVE_CYCLES"
P2="SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM SQ_INST_CYCLES_SALU SQ_INSTS_SMEM SQ_INSTS_BRANCH"
P3="SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES"
n=0
for P in "$P1" "$P2" "$P3"; do
  n=$((n + 1))
  rm -rf "$OUT/pmc$n"; mkdir -p "$OUT/pmc$n"
  timeout -k 10 300 rocprofv3 --pmc $P -f csv -d "$OUT/pmc$n" -- $B > "$OUT/pmc$n.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass $n failed ($rc)"; tail -n 30 "$OUT/pmc$n.log"; exit $rc
  fi
  echo "pass $n done"
done
python - "$OUT" <<'PY' | tee "$OUT/summary.txt"
import csv, glob, collections, json, os, sys
out = sys.argv[1]
KERNELS = ("enum_phase_kernel", "enum_walk_kernel", "enum_walk4_kernel", "enum_walk5_kernel")
for p in ("pmc1", "pmc2", "pmc3"):
    if not os.path.exists("%s/%s.log" % (out, p)):
        continue
    acc = collections.defaultdict(float)
    for f in glob.glob("%s/%s/**/*counter_collection.csv" % (out, p), recursive=True):
        for r in csv.DictReader(open(f)):
            if any(k in r["Kernel_Name"] for k in KERNELS):
                acc[r["Counter_Name"]] += float(r["Counter_Value"])
    l = [x for x in open("%s/%s.log" % (out, p)) if x.startswith("{")]
    if l:
        d = json.loads(l[-1])
        nodes = d["value"] * d["ms_per_step"] / 1e3
        print(p, json.dumps({"counters": dict(sorted(acc.items())), "nodes_per_step": nodes,
                             "per_node": {k: v / nodes for k, v in sorted(acc.items())}}))
    else:
        print(p, dict(acc))
        print(open("%s/%s.log" % (out, p)).read()[-800:])
PY
