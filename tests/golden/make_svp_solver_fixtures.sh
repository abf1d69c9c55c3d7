#!/bin/bash
# Regenerates tests/golden/svpsolve_*.json with the REAL reference: lll_reduction + shortest_vector (SVPM_FAST and
# SVPM_PROVED) recorded by tests/native/shortest_vector_ref_driver.cpp — build line in its header, the binary goes to
# oracle/_ref/.  What the fixtures are for: tests/test_svp_solver_cpu.py (their conditions) and
# tests/test_svp_solver_gpu.py.  The reference's own example_svp_in / example_svp_out pair (data files of its test
# suite, 20 x 21) is copied next to them; svp_rank_defect.json is the 4 x 4 matrix of its test_rank_defect, as data.
set -e
cd "$(dirname "$0")/../.."
D=oracle/_ref/shortest_vector_ref_driver
G=tests/golden
REF=${REF:?set REF to the source tree of fplll (the variable of oracle/Makefile)}
#  d seed qbits   (q-ary, q a prime of 11 bits: entries below 2^11), two seeds per dimension, counted up from 1.  A seed
# is replaced by the next one where the FAST and the PROVED norm differ (the driver exits with status 3), and where the
# reference's FAST call takes 100 ms or more on one core: the lone wavefront of a one-lattice test walks such a tree
# about fifteen times slower than that core, and a test has a few seconds.
for d in 24 32 40; do
  found=0
  seed=1
  while [ $found -lt 2 ]; do
    f=$G/svpsolve_q${d}_s${seed}.json
    if $D $d $seed 11 > $f && python3 -c "import json, sys; sys.exit(0 if json.load(open('$f'))['fast']['ref_ms'] < 100 else 1)"; then
      found=$((found + 1))
    else
      rm -f $f
    fi
    seed=$((seed + 1))
  done
done
cp $REF/tests/lattices/example_svp_in $G/example_svp_in.txt
cp $REF/tests/lattices/example_svp_out $G/example_svp_out.txt
chmod 644 $G/example_svp_in.txt $G/example_svp_out.txt
cat > $G/svp_rank_defect.json <<'JSON'
{"desc": "the matrix of test_rank_defect (the reference's tests/test_svp.cpp): LLL-reduce, then shortest_vector must succeed",
 "basis": [[75, 44, -5, -16], [29, 7, -52, 134], [-89, 108, 56, 29], [-94, 55, -194, -20]]}
JSON
# The families of tests/solver_families.py (reduced in exact arithmetic, not by the reference): one knapsack, one
# cut_rows and one scaled_root member, given to the driver as files; FAST and PROVED recorded as they come — on the
# scaled root lattice the FAST method, which decides in floating point, returns a vector that is not the shortest.
for name in knap_d20_b40 cut_scaled root_e8_s29_x2_0; do
  t=$(mktemp)
  python3 -c "import sys; sys.path.insert(0, 'tests'); import solver_families as F; print('[' + ' '.join('[' + ' '.join(str(v) for v in r) + ']' for r in F.basis('$name')) + ']')" > $t
  $D --file $t > $G/svpsolve_fam_$name.json
  rm -f $t
done
