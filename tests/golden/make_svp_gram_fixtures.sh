#!/bin/bash
# Regenerates tests/golden/svpgram_*.json with the REAL reference: LLL over MatGSOGram, symmetrize_g, shortest_vector
# and shortest_vectors(max_sols) with SVPM_FAST, recorded by tests/native/svp_gram_ref_driver.cpp — build line in its
# header, the binary goes to oracle/_ref/.  The forms:
#   dim7, dim4     the reference's own test forms (its tests/lattices/grammatrix_dimension7 and _dimension4; REF below
#                  is its source tree), with the coefficient vectors it holds as their answers ("ref_out");
#   nobasis        G_in of tests/golden/lllgram_form_nobasis.json: B B^T of no integer B;
#   q24            B B^T of the basis of tests/golden/svpsolve_q24_s1.json,
# each for max_sols = 8 and 64.  What the fixtures are for: tests/test_svp_gram_cpu.py (the recorded coefficients have the
# recorded norms under the recorded form, the norms are the exact enumeration's) and tests/test_svp_gram_gpu.py (both
# routes return them).
set -e
cd "$(dirname "$0")/../.."
REF=${REF:-/root/reference}
D=oracle/_ref/svp_gram_ref_driver
G=tests/golden
fmt="import sys, json; print('[' + ' '.join('[' + ' '.join(str(v) for v in r) + ']' for r in json.load(sys.stdin)) + ']')"
t=$(mktemp)
for k in 8 64; do
  for dim in 7 4; do
    $D $REF/tests/lattices/grammatrix_dimension$dim dim$dim $k > $t
    python3 - $t $REF/tests/lattices/grammatrix_dimension${dim}_out > $G/svpgram_dim${dim}_k$k.json <<'PY'
import sys
body = open(sys.argv[1]).read().rstrip()
out = [int(v) for v in open(sys.argv[2]).read().replace("[", " ").replace("]", " ").split()]
assert body.endswith("}")
print(body[:-1] + ',\n"ref_out":[' + ",".join(str(v) for v in out) + "]}")
PY
  done
  python3 -c "import json; print(json.dumps(json.load(open('$G/lllgram_form_nobasis.json'))['G_in']))" | python3 -c "$fmt" > $t
  $D $t nobasis $k > $G/svpgram_nobasis_k$k.json
  python3 -c "import json; b = json.load(open('$G/svpsolve_q24_s1.json'))['basis']; print(json.dumps([[sum(x * y for x, y in zip(r, s)) for s in b] for r in b]))" | python3 -c "$fmt" > $t
  $D $t q24 $k > $G/svpgram_q24_k$k.json
done
rm -f $t
