#!/bin/bash
# Regenerates tests/golden/lllgram_*.json(.gz) with the REAL reference: LLLReduction<Z_NR<long>, FP_NR<double>> over
# MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM), recorded by tests/native/lll_gram_ref_driver.cpp
# — build line in its header, the binary goes to oracle/_ref/.  What the fixtures are for: tests/test_lll_gram_cpu.py
# (the model of tests/gram_lll_model.py reproduces them; their own conditions) and tests/test_lll_gram_gpu.py.
# The conditions of tests/test_lll_gram_cpu.py are checked on every fixture right after recording.
set -e
cd "$(dirname "$0")/../.."
REF=${REF:-/root/reference}  # fplll's source tree (the variable of oracle/Makefile): its tests/lattices
R=oracle/_ref
D=$R/lll_gram_ref_driver
G=tests/golden
L=$REF/tests/lattices
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
# (forms of 10 rows and more are stored gzipped: mu and r as hexadecimal doubles are most of a file)
run() {
  name=$1; shift
  $D "$name" "$@" > $G/lllgram_$name.json
  if [ "$(grep -m1 '"d":' $G/lllgram_$name.json | tr -dc 0-9)" -ge 10 ]; then gzip -9nf $G/lllgram_$name.json; fi
}

# ---- the inputs of the reference's own tests/test_lll_gram.cpp (those that fit Z_NR<long>)
run example2 0.99 0.51 0 A < $L/example2_in
run cvp_lattice 0.99 0.51 0 A < $L/example_cvp_in_lattice
run cvp_lattice2 0.99 0.51 0 A < $L/example_cvp_in_lattice2
run cvp_lattice3 0.99 0.51 0 A < $L/example_cvp_in_lattice3
run cvp_lattice4 0.99 0.51 0 A < $L/example_cvp_in_lattice4
run cvp_lattice5 0.99 0.51 0 A < $L/example_cvp_in_lattice5
run intrel_40_10 0.99 0.51 0 intrel 40 10 1
run intrel_50_20 0.99 0.51 0 intrel 50 20 1
# ---- LLL_SIEGEL (4); LLL_EARLY_RED (2), which the reference switches off on an integer Gram matrix
run cvp_lattice4_siegel 0.99 0.51 4 A < $L/example_cvp_in_lattice4
run cvp_lattice4_early 0.99 0.51 2 A < $L/example_cvp_in_lattice4

# ---- inputs made here: rank deficit, a form that is no B B^T, the edges, the width classes
python - "$T" "$R" <<'EOF'
import sys
import numpy as np
T, R = sys.argv[1], sys.argv[2]

def fmt(m):
    return "[" + "\n".join("[" + " ".join(str(int(x)) for x in row) + "]" for row in m) + "]\n"

rng = np.random.default_rng(20260)
# rank deficit: a repeated row (3 = 1) and a row that is an integer combination of others (6 = 2*0 - 2 + 4)
a = rng.integers(-40, 41, size=(8, 10))
a[3] = a[1]
a[6] = 2 * a[0] - a[2] + a[4]
open(T + "/rankdef.A", "w").write(fmt(a))

# a form that is B B^T of no integer B: positive definite, odd determinant that is no square
def det(m):  # Bareiss, exact
    m = [[int(x) for x in row] for row in m]
    n, prev, sign = len(m), 1, 1
    for k in range(n - 1):
        if m[k][k] == 0:
            p = next((i for i in range(k + 1, n) if m[i][k]), None)
            if p is None:
                return 0
            m[k], m[p] = m[p], m[k]
            sign = -sign
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                m[i][j] = (m[i][j] * m[k][k] - m[i][k] * m[k][j]) // prev
        prev = m[k][k]
    return sign * m[-1][-1]

import math
while True:
    d = 7
    g = np.diag(rng.integers(500, 4000, size=d) * 2 + 1)
    p = rng.integers(-300, 301, size=(d, d))
    p = np.tril(p, -1)
    g = g + p + p.T
    # unreduce it: a unimodular lower-triangular change of variables
    u = np.tril(rng.integers(-5, 6, size=(d, d)), -1) + np.eye(d, dtype=np.int64)
    dt = det(g)
    if all(det(g[:k, :k]) > 0 for k in range(1, d + 1)) and dt % 2 == 1 and math.isqrt(dt) ** 2 != dt:
        g = u @ g @ u.T
        break
open(T + "/form.G", "w").write(fmt(g))

open(T + "/d1.G", "w").write(fmt([[7]]))
open(T + "/d2.G", "w").write(fmt([[10, 23], [23, 54]]))
open(T + "/d3.A", "w").write(fmt([[12, 5, -7, 3], [25, 9, -13, 7], [-31, -16, 22, -8]]))

# width classes: wide_basis(d) of tests/lll_gram_cases.py, a recipe in integer arithmetic (no fixture stores it)
sys.path.insert(0, "tests")
import lll_gram_cases as S
for d in (64, 65, 128, 129, 192, 193, 256):
    open(T + "/w%d.A" % d, "w").write(fmt(S.wide_basis(d)))
EOF
run rankdef 0.99 0.51 0 A < $T/rankdef.A
run form_nobasis 0.99 0.51 0 G < $T/form.G
run d1 0.99 0.51 0 G < $T/d1.G
run d2 0.99 0.51 0 G < $T/d2.G
run d3 0.99 0.51 0 A < $T/d3.A
# ... recorded in full, checked (the run succeeded and swapped, u G_in u^T == G_out), then stored compactly: u, the
# counters, the diagonal of r and the SHA-256 of G_in, G_out, mu and r (compact() of tests/lll_gram_cases.py: written
# out these seven records are 2.5 MB gzipped, nearly all of it the mantissas of mu and r)
for d in 64 65 128 129 192 193 256; do
  $D w$d 0.99 0.51 0 A < $T/w$d.A > $T/w$d.json
done
python - "$T" <<'EOF'
import gzip, json, sys
import numpy as np
sys.path.insert(0, "tests")
import lll_gram_cases as S
for d in (64, 65, 128, 129, 192, 193, 256):
    f = json.load(open("%s/w%d.json" % (sys.argv[1], d)))
    u, gin = np.array(f["u"], dtype=object), np.array(f["G_in"], dtype=object)
    assert f["status"] == 0 and f["n_swaps"] > 0 and f["gso_rows"] == d
    assert (u.dot(gin).dot(u.T) == np.array(f["G_out"], dtype=object)).all()
    with gzip.GzipFile("tests/golden/lllgram_w%d.json.gz" % d, "wb", 9, mtime=0) as fh:
        fh.write(json.dumps(S.compact(f), separators=(",", ":")).encode())
EOF
python -m pytest -q tests/test_lll_gram_cpu.py -k conditions
