"""Forms on which a candidate's partial sums y_j = sum_i x_i g_ij leave the 63 bits while x G x^T fits: what the 128-bit
evaluator of svp_gram.hip is for, and what an overflow-checked 64-bit evaluator gives up on (status -2).  Shared by
tests/test_svp_gram_cpu.py and tests/test_svp_gram_gpu.py.

The forms are Gram matrices of bases that are NOT size-reduced (mu up to 3): a short vector is then a combination of
long rows with coefficients of several units, and the prefixes of its sums are several times the largest entry.  Every
entry is a small integer times a power of two, so mu and r_ii are exact doubles whatever computes them.

  CASES: name -> (G, bound_sq, K)
  partial_bits(G, xs) -> (bit length of the largest |prefix of y_j|, of the largest |x_j y_j|) over the vectors xs
"""
import numpy as np

import list_helpers as H


def skew2():
    """2^56 [[49, 35], [35, 26]] (rows (7, 0) and (5, 1), mu = 5 / 7), every vector with a value below 2^63."""
    s2 = 2**56
    return [[49 * s2, 35 * s2], [35 * s2, 26 * s2]], 2**63 - 1, 64


def skew8(K):
    """An LLL-reduced 8 x 8 basis R with entries in [-6, 6], rows b_i + 3 b_{i-1} / b_i - 2 b_{i-1} in turn, its Gram
    matrix scaled by the largest power of two that keeps the entries within int64; the bound 110 times the scale."""
    R = H.lll_exact(np.random.default_rng(8).integers(-6, 7, size=(8, 8)).tolist())
    U = [[int(i == j) for j in range(8)] for i in range(8)]
    for i in range(1, 8):
        U[i][i - 1] = 3 if i % 2 else -2
    B = [[sum(U[i][k] * R[k][j] for k in range(8)) for j in range(8)] for i in range(8)]
    G0 = [[sum(a * b for a, b in zip(r1, r2)) for r2 in B] for r1 in B]
    e = (2**63 - 1) // max(abs(v) for row in G0 for v in row)
    s2 = 1 << (e.bit_length() - 1)
    return [[v * s2 for v in row] for row in G0], 110 * s2, K


CASES = {"skew2": skew2, "skew8_k4": lambda: skew8(4), "skew8_k64": lambda: skew8(64)}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def partial_bits(G, xs):
    big = term = 0
    d = len(G)
    for x in xs:
        for j in range(d):
            acc = 0
            for i in range(d):
                acc += int(x[i]) * int(G[i][j])
                big = max(big, abs(acc))
            term = max(term, abs(int(x[j]) * acc))
    return big.bit_length(), term.bit_length()
