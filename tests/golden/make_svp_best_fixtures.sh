#!/bin/bash
# Regenerates tests/golden/svpbest_*.json with the REAL reference: Enumeration under a FastEvaluator with
# EVALSTRATEGY_BEST_N_SOLUTIONS (what its shortest_vectors(max_sols) runs), recorded by
# tests/native/shortest_vectors_ref_driver.cpp — build line in its header, the binary goes to oracle/_ref/.  The bases
# are those of the recorded shortest-vector fixtures (tests/golden/svpsolve_*.json), as they stand:
#   svpsolve_q24_s1 at 3181 (26 vectors within it: a table of 64 never fills) and at 3817 (233: it fills and shrinks),
#   svpsolve_q32_s2 at 5620 (24 vectors within it),
# each for max_sols = 8 and 64.  What the fixtures are for: tests/test_svp_best_cpu.py (the recorded norms are those of
# the recorded coefficients and the model's) and tests/test_svp_best_gpu.py (both routes return them).
set -e
cd "$(dirname "$0")/../.."
D=oracle/_ref/shortest_vectors_ref_driver
G=tests/golden
for case in "svpsolve_q24_s1 3181" "svpsolve_q24_s1 3817" "svpsolve_q32_s2 5620"; do
  set -- $case
  t=$(mktemp)
  python3 -c "import json; b = json.load(open('$G/$1.json'))['basis']; print('[' + ' '.join('[' + ' '.join(str(v) for v in r) + ']' for r in b) + ']')" > $t
  for k in 8 64; do
    $D $t $1 $2 $k > $G/svpbest_${1#svpsolve_}_b$2_k$k.json
  done
  rm -f $t
done
