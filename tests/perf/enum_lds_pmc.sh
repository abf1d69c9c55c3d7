#!/bin/bash
# PMC passes, counters only, over the enumeration-only bench (1 step each); summary per pass, summed over the walk
# kernels' dispatches, with the per-node figures (counter / nodes of the step).
#   tests/perf/enum_lds_pmc.sh [TREE [OUT]]   (enum_pmc.sh's two passes plus the LDS unit's)
# TREE: the checkout whose bench.py and library run (default: the one this script lies in — a parent commit's export
# for a before / after pair); OUT: where the passes and summary.txt go (default: enum_pmc under $TMPDIR).
# Passes 1 and 2: the instruction mix.  Passes 3 and 4: the LDS unit (issue stalls, busy cycles, bank conflicts) — of
# the names below only those the device offers (rocprofv3 --list-avail) are asked for.
# Every pass runs under its own time limit, and nothing is started behind a pass that failed.
HERE=$(cd "$(dirname "$0")/../.." && pwd)
R=$(cd "${1:-$HERE}" && pwd)
export TMPDIR=${TMPDIR:-/tmp}
OUT=${2:-$TMPDIR/enum_pmc}
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
B="python $R/bench.py --no-cpu --no-gso --no-tour --no-pmc --no-batch --steps 1 --warmup 0"
avail=$(timeout -k 10 120 rocprofv3 --list-avail 2>&1)
# (a listing without a counter every pass has used so far is no listing: then all names are asked for)
grep -qw SQ_INSTS_LDS <<<"$avail" || avail=
pick() { for c in "$@"; do { [ -z "$avail" ] || grep -qw "$c" <<<"$avail"; } && printf '%s ' "$c"; done; }
P1="SQ_BUSY_CYCLES SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAVES SQ_WAVE_CYCLES"
P2="SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM SQ_INST_CYCLES_SALU SQ_INSTS_SMEM SQ_INSTS_BRANCH"
P3=$(pick SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES)
P4=$(pick SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_INSTS_LDS SQ_WAVE_CYCLES)
echo "pass 3: $P3"; echo "pass 4: $P4"
n=0
for P in "$P1" "$P2" "$P3" "$P4"; do
  n=$((n + 1))
  [ -n "$P" ] || continue
  rm -rf "$OUT/pmc$n"; mkdir -p "$OUT/pmc$n"
  (cd "$R" && timeout -k 10 420 rocprofv3 --kernel-trace --pmc $P -f csv -d "$OUT/pmc$n" -- $B) > "$OUT/pmc$n.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass $n failed ($rc)"; tail -n 30 "$OUT/pmc$n.log"; exit $rc
  fi
done
python - "$OUT" <<'PY' | tee "$OUT/summary.txt"
import csv, glob, collections, json, os, sys
out = sys.argv[1]
for p in ("pmc1", "pmc2", "pmc3", "pmc4"):
    if not os.path.exists("%s/%s.log" % (out, p)):
        continue
    acc = collections.defaultdict(float)
    for f in glob.glob("%s/%s/**/*counter_collection.csv" % (out, p), recursive=True):
        for r in csv.DictReader(open(f)):
            if "enum_phase_kernel" in r["Kernel_Name"] or "enum_walk_kernel" in r["Kernel_Name"]:
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
