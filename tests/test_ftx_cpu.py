"""fplll_amd/csrc/ftx.h — the double-double and quad-double arithmetic of the extended-precision kernels (the device
stand-ins for the reference's FP_NR<dd_real> / FP_NR<qd_real>: libqd is absent, parity with it is unpinned) — compiled
FOR THE HOST (tests/native/ftx_host.cpp: the header's arithmetic is plain C++) and checked against mpmath on the
operand classes of tests/ftx_cases.py (random, 62-bit integers, cancellation, equal operands, plain doubles, far-apart
magnitudes, interior gaps, binade boundaries, extreme exponents): every operation to a few units of 2^-104 / 2^-205
of the result (of the larger operand for the "sloppy" additions), nint / rnd_we / the comparisons exactly, and every
result normalised.  The GPU suite runs the same list on the device and compares it bit for bit with this build
(tests/test_ftx_gpu.py); the exact R-factor used there (the Cholesky factor of the integer Gram matrix) is pinned here
against the reference's 106-bit MPFR run."""
import gzip
import json
import os

import numpy as np
import pytest

import conftest as C
import ftx_cases as F

mp = pytest.importorskip("mpmath")


@pytest.fixture(scope="module")
def ftx(tmp_path_factory):
    return F.host_harness(tmp_path_factory.mktemp("ftx"))


@pytest.mark.parametrize("comps,base,eps_bits", [(4, 0, 205), (2, 10, 104)])
def test_extended_arithmetic_against_mpmath(ftx, comps, base, eps_bits):
    """add, sub, mul, div, sqrt, mul by a double (1 / 1 / 4 / 8 / 4 / 4 units of 2^-eps_bits), nint, le / gt, rnd_we
    over all operand classes, with the normalisation invariant on every result (`base`, the harness's op offset of the
    type, and `eps_bits` are kept as parameters only because they are part of the case ids this test has had since
    before the operand classes moved to ftx_cases.py; they are checked against that module's constants): no zero component followed by a non-zero one and |x[k+1]| <= ulp(x[k]) — the weak form; half an ulp does
    not hold in general (a cancelling quad-double sum can leave |x[2]| at 1.1 half-ulps of x[1]), so the components
    above half an ulp are counted, not refused."""
    assert F.EPS_BITS[comps] == eps_bits and base == (10 if comps == 2 else 0)
    for label, op, a, b, verify in F.checks(comps):
        line = verify(ftx(comps, op, a, b))
        C.note(lambda: ("%s %s" % ("qd" if comps == 4 else "dd", line),))


def test_quad_double_nint_is_exact(ftx):
    """nint by parts on another seed: an integer, within 1/2 of the operand — and THE nearest one with halves going
    up (libqd's rule), on integral and tied leading components and beyond 2^52"""
    mp.mp.prec = F.PREC
    q = F.nint_cases(3, 4, 600)
    out = ftx(4, 5, q, q)
    for i in range(len(q)):
        x, got = F.val(q[i]), F.val(out[i])
        assert got == mp.floor(got) and abs(got - x) <= mp.mpf(1) / 2, (list(q[i]), list(out[i]))
        assert got == F.nint_exact(x), (list(q[i]), list(out[i]))


def test_operand_classes_are_what_they_say():
    """the generator itself: deterministic, normalised (except the gaps), and every class present with its property"""
    a, b, cls = F.arith_cases(2024, 4, 2048)
    a2, b2, _ = F.arith_cases(2024, 4, 2048)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    assert set(cls) == set(F.CLASSES)
    idx = {c: [i for i, x in enumerate(cls) if x == c] for c in F.CLASSES}
    nogap = [i for i, x in enumerate(cls) if x != "gap"]
    for x in (a, b):
        bad, above = F.normalisation(x[nogap], 4)
        assert not bad and above == 0
        assert np.all(x[idx["gap"], 1] == 0) and np.all(x[idx["gap"], 2] != 0)
        assert np.all(x[idx["plain"], 1:] == 0)
        assert np.all(x[idx["int62"], 2:] == 0) and np.all(x[idx["int62"], 1] == np.round(x[idx["int62"], 1]))
        assert np.all(x[idx["random"], 3] != 0)
    assert np.array_equal(a[idx["equal"]], b[idx["equal"]])
    e = np.frexp(a[idx["scaled"], 0])[1]
    assert np.all(np.abs(e) >= 160) and (e > 0).any() and (e < 0).any()
    mp.mp.prec = F.PREC
    for i in idx["cancel"][:40]:
        x, y = F.val(a[i]), F.val(b[i])
        assert mp.mpf(2) ** -192 < abs(x + y) / abs(x) < mp.mpf(2) ** -19
    q = F.nint_cases(2034, 4, 600)
    assert np.count_nonzero(np.abs(q[:, 0]) >= 2.0 ** 52) > 100
    assert np.count_nonzero(np.abs(q[:, 0] - np.floor(q[:, 0])) == 0.5) > 50


@pytest.mark.parametrize("name", ["q40", "q72"])
def test_cholesky_of_the_exact_gram_matrix_is_the_reference_r_factor(name):
    """The R-factor reference of the quad-double device test: the lower Cholesky factor of the exact integer Gram
    matrix, at 700 bits.  The reference's MatHouseholder run in MPFR at 106 bits (hhmp106_*.json.gz) carries ~2^-102
    of its own error: agreement to 2^-100 of the row norm, entry by entry and sign by sign (the diagonal is positive
    in both), pins the construction and the sign convention.  (Measured: 2^-103.0 on q40, 2^-101.8 on q72.)"""
    mp.mp.prec = 700
    with gzip.open(os.path.join(C.GOLDEN, "hhmp106_%s.json.gz" % name), "rt") as f:
        j = json.load(f)
    d, n = j["d"], j["n"]
    b = np.array(j["b"], dtype=np.int64).reshape(d, n)
    L = F.cholesky_rfactor(b)
    want = iter(j["R"])
    worst = mp.mpf(0)
    for i in range(d):
        ref = [mp.mpf(next(want)) for _ in range(i + 1)]
        rown = mp.sqrt(mp.fsum(t * t for t in ref))
        assert ref[i] > 0 and L[i][i] > 0
        worst = max(worst, max(abs(x - y) for x, y in zip(L[i], ref)) / rown)
    C.note(lambda: ("Cholesky of the exact Gram matrix vs MPFR-106 on %s: 2^%.1f of the row norm"
                    % (name, float(mp.log(worst, 2))),))
    assert worst <= mp.mpf(2) ** -100
