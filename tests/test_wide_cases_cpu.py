"""The inputs of tests/test_width_classes_gpu.py are what tests/wide_cases.py says they are, and its exact checkers
tell right from wrong — shown with the C oracle alone, without a GPU.

Inputs: every lattice gives LLL and HLLL at least 10 swaps (status 1), BKZ changes every BKZ input within 2e6 nodes, the
last chunk carries at least a quarter of every row's squared norm in the short-wide family and DECIDES the run (zeroing
it changes the swap count or the transformation on the other columns), the tall family's exchanges and the rows the
reduction changes reach the last chunk of rows.
Checkers: they accept the oracle's outputs and reject three doctored ones — a row replaced by twice itself (lattice),
two reduced rows exchanged (Lovasz), a multiple of an earlier row added to a row (size reduction)."""
import numpy as np
import pytest

import wide_cases as W

mp = pytest.importorskip("mpmath")

MIN_SWAPS = 10
MAX_NODES = 2 * 10 ** 6
ALL_SHORT = W.SHORT_WIDE + W.SHORT_WIDE_BKZS
_id = lambda s: "%dx%d" % s  # noqa: E731


def test_width_classes_of_the_shapes():
    assert [W.nq_of(d, n) for d, n in W.SHORT_WIDE] == [2, 3, 3, 4, 4]
    assert [W.nq_of(d, n) for d, n in W.SHORT_WIDE_BKZS] == [2, 3, 4] and W.SHORT_WIDE_BKZS[1:] == W.SHORT_WIDE_BKZ
    assert [W.nq_of(*W.tall_base(nq).shape) for nq in (3, 4)] == [3, 4]
    assert W.tall_base(3).shape == (180, 180) and W.tall_base(4).shape == (200, 200)
    # the builders are deterministic, and the lattices of a batch differ
    assert np.array_equal(W.short_wide(20, 193, 2), W.short_wide(20, 193, 2))
    assert np.array_equal(W.tall(3, 5), W.tall(3, 5))


@pytest.mark.parametrize("shape", ALL_SHORT, ids=_id)
def test_short_wide_inputs(shape):
    d, n = shape
    lo = W.last_chunk(d, n)
    bs = W.short_wide_batch(d, n)
    assert len(bs) == 5 and len({b.tobytes() for b in bs}) == 5
    paths = set()
    for b in bs:
        assert b.shape == (d, n) and np.array_equal(b[:, :d], np.eye(d, dtype=np.int64))
        assert W.last_chunk_share(b).min() >= 0.25
        st, info, out = W.oracle_lll(b)
        hst, hinfo, hout = W.oracle_hlll(b)
        assert st == 1 and hst == 1
        assert info[1] >= MIN_SWAPS and hinfo[0] >= MIN_SWAPS
        for flags in (2, 6):
            assert W.oracle_lll(b, flags)[0] == 1
        paths.add((info[1], hinfo[0]))
        # sensitivity: without the last chunk the run is another one
        zst, zinfo, zout = W.oracle_lll(W.without_last_chunk(b))
        assert zst == 1
        assert zinfo[1] != info[1] or not np.array_equal(zout[:, :lo], out[:, :lo])
        hz = W.oracle_hlll(W.without_last_chunk(b))
        assert hz[1][0] != hinfo[0] or not np.array_equal(hz[2][:, :lo], hout[:, :lo])
    assert len(paths) > 1   # the waves of a launch take different decision paths


@pytest.mark.parametrize("nq", [3, 4])
def test_tall_inputs(nq):
    lo = 64 * (nq - 1)
    bs = W.tall_batch(nq)
    assert len(bs) == 3 and len({b.tobytes() for b in bs}) == 3
    for seed, b in zip(W.TALL_SEEDS[nq], bs):
        ex = W.tall_exchanges(nq, seed)
        assert len(ex) == 24 and sum(i >= lo for i in ex) >= 4 and all(0 <= i < b.shape[0] - 1 for i in ex)
        assert W.same_lattice_square(W.tall_base(nq), b)
        st, info, out = W.oracle_lll(b)
        hst, hinfo, hout = W.oracle_hlll(b)
        assert st == 1 and hst == 1
        assert info[1] >= MIN_SWAPS and hinfo[0] >= MIN_SWAPS
        for flags in (2, 6):
            assert W.oracle_lll(b, flags)[0] == 1
        assert (out[lo:] != b[lo:]).any() and (hout[lo:] != b[lo:]).any()


@pytest.mark.parametrize("shape", W.SHORT_WIDE_BKZS, ids=_id)
def test_short_wide_bkz_inputs(shape):
    for b in W.short_wide_batch(*shape):
        lll = W.oracle_lll(b)[2]
        st, tours, nodes, out = W.oracle_bkz(lll, 12)
        assert st == 1 and tours >= 1 and 0 < nodes < MAX_NODES
        assert not np.array_equal(out, lll)
        for which in ("rerand", "pre_gh"):
            st, nodes, calls, rerand, out = W.oracle_bkzs(lll, 36, which)
            assert st in (1, 8) and 0 < nodes < MAX_NODES
            assert not np.array_equal(out, lll)


@pytest.mark.parametrize("nq", [3, 4])
def test_tall_bkz_inputs(nq):
    lo = 64 * (nq - 1)
    rerand = 0
    for b in W.tall_batch(nq):
        lll = W.oracle_lll(b)[2]
        st, tours, nodes, out = W.oracle_bkz(lll, 10, 1)
        assert st in (1, 8) and tours == 1 and 0 < nodes < MAX_NODES
        assert (out[lo:] != lll[lo:]).any()
        for which in ("rerand", "pre_gh"):
            st, nodes, calls, rr, out = W.oracle_bkzs(lll, 30, which)
            assert st in (1, 8) and 0 < nodes < MAX_NODES
            assert (out[lo:] != lll[lo:]).any()
            rerand += rr
    assert rerand > 0   # the generator streams are in use


# ---- the checkers ------------------------------------------------------------------------------------------------------
def _doctored(out, g, delta=0.99):
    """(twice a row, two rows exchanged so that Lovasz fails for certain, a row plus 3 times an earlier one).
    Exchanging rows i - 1, i turns s = r(i,i) + mu(i,i-1)^2 r(i-1,i-1) into the new r(i-1,i-1) and Lovasz' condition at i
    into r(i-1,i-1) <= delta s: it fails exactly where the reduced basis had s > r(i-1,i-1) / delta, so the pair with the
    largest s / r(i-1,i-1) is taken (and has to have that much: a reduced basis whose profile never rises would
    need another doctoring).  The conditions before i - 1 read rows that did not move, so the FIRST failure is at i or
    at i - 1 (_at)."""
    d = out.shape[0]
    twice = out.copy()
    twice[d // 2] *= 2
    s = lambda k: (g.r[k] + g.mu[k][k - 1] ** 2 * g.r[k - 1]) / g.r[k - 1]  # noqa: E731
    i = max(range(1, d), key=s)
    assert s(i) * g.num(delta) > 1
    swapped = out.copy()
    swapped[[i - 1, i]] = swapped[[i, i - 1]]
    added = out.copy()
    added[d - 1] += 3 * added[d // 3]
    return twice, (swapped, i), (added, d - 1)


def _at(i):
    return (("lovasz", i - 1), ("lovasz", i))


@pytest.mark.parametrize("shape", W.SHORT_WIDE, ids=_id)
def test_checkers_on_the_short_wide_family(shape):
    for b in W.short_wide_batch(*shape)[:2]:
        for out, viol in ((W.oracle_lll(b)[2], W.lll_violation), (W.oracle_hlll(b)[2], W.hlll_violation)):
            g = W.exact_gso(out)
            assert W.same_lattice(b, out)
            assert viol(g) is None
            twice, (swapped, i), (added, row) = _doctored(out, g)
            assert not W.same_lattice(b, twice)
            assert W.same_lattice(b, swapped) and viol(W.exact_gso(swapped), which=("lovasz",)) in _at(i)
            assert viol(W.exact_gso(swapped)) is not None
            assert W.same_lattice(b, added) and viol(W.exact_gso(added))[:2] == ("size", row)
    # one entry off by one: U is no longer integral, or no longer fits every column
    off = out.copy()
    off[1, shape[1] - 1] += 1
    assert not W.same_lattice(b, off)


@pytest.mark.parametrize("nq", [3, 4])
def test_checkers_on_the_tall_family(nq):
    b = W.tall_batch(nq)[1]
    out, hout = W.oracle_lll(b)[2], W.oracle_hlll(b)[2]
    g = W.exact_gso(out, True)
    assert W.same_lattice_square(b, out) and W.same_lattice_square(W.tall_base(nq), out)
    assert W.same_lattice_square(b, hout)
    assert W.lll_violation(g) is None and W.hlll_violation(W.exact_gso(hout, True)) is None
    # (an LLL-reduced basis is HLLL-reduced for the same delta and eta, whatever theta: one doctoring serves both)
    assert W.hlll_violation(g) is None
    twice, (swapped, i), (added, row) = _doctored(out, g)
    assert not W.same_lattice_square(b, twice)
    assert W.same_lattice_square(b, swapped) and W.same_lattice_square(b, added)
    gs, ga = W.exact_gso(swapped, True), W.exact_gso(added, True)
    for viol in (W.lll_violation, W.hlll_violation):
        assert viol(gs, which=("lovasz",)) in _at(i) and viol(gs) is not None
        assert viol(ga)[:2] == ("size", row)
    off = out.copy()
    off[1, 0] += 1
    assert not W.same_lattice_square(b, off)


def test_predicates_have_no_slack():
    """eta and delta are taken at the exact value of the double: a 2 x 2 basis with mu = 51/100 exactly is size-reduced
    for eta = 0.51 (that double lies 9e-18 above 51/100) and is NOT for the next double down; Lovasz likewise at
    equality."""
    from fractions import Fraction
    assert Fraction(0.51) > Fraction(51, 100) > Fraction(float(np.nextafter(0.51, 0.0)))
    g = W.exact_gso(np.array([[100, 0], [51, 1000]]))
    assert W.lll_violation(g, 0.99, 0.51) is None
    assert W.lll_violation(g, 0.99, float(np.nextafter(0.51, 0.0))) == ("size", 1, 0)
    # r(1,1) = (delta - mu^2) r(0,0) exactly, with delta = 3/4 and mu = 1/2: 10000 / 2 = 5000 = 50^2 + 50^2
    g = W.exact_gso(np.array([[100, 0, 0], [50, 50, 50]]))
    assert W.lll_violation(g, 0.75, 0.51) is None
    assert W.lll_violation(g, float(np.nextafter(0.75, 1.0)), 0.51) == ("lovasz", 1)
    assert W.hlll_violation(g, 0.75, 0.51, 0.0) is None
    assert W.hlll_violation(g, float(np.nextafter(0.75, 1.0)), 0.51, 0.0) == ("lovasz", 1)
    # |R(1,0)| <= eta R(0,0) + theta R(1,1): mu = 3/5 against eta = 1/2 needs theta R(1,1) >= R(0,0) / 10
    g = W.exact_gso(np.array([[10, 0], [6, 8]]))
    assert W.hlll_violation(g, 0.5, 0.5, 0.125) is None          # 1/8 . 8 = 1 = 10 / 10
    assert W.hlll_violation(g, 0.5, 0.5, float(np.nextafter(0.125, 0.0))) == ("size", 1, 0)


def test_fixed_point_cholesky_is_ftx_cases_cholesky():
    """wide_cases.cholesky_fixed against ftx_cases.cholesky_rfactor at 300 bits on 100 rows of a tall output: the two
    agree to 2^-250 of the row norm — the mpmath run rounds every quotient at 300 bits and the conditioning of the
    factor (its diagonal spans 2^4) amplifies that by far less than the 50 bits left for it — and the error helpers
    built on it read 0 for the exact factor itself and 2^-53-ish for its rounding to doubles."""
    import ftx_cases as F
    out = W.oracle_lll(W.tall_batch(4)[0])[2][:100]
    L = W.cholesky_fixed(out, 300)
    L0 = F.cholesky_rfactor(out, 300)
    mp.mp.prec = 400
    worst = max(abs(L[i][j] - L0[i][j]) / mp.sqrt(mp.fsum(t * t for t in L0[i]))
                for i in range(len(L)) for j in range(i + 1))
    assert worst <= mp.mpf(2) ** -250, W.log2(worst)
    R = np.zeros((100, 200))
    for i in range(100):
        for j in range(i + 1):
            R[i, j] = float(L0[i][j])
    err = W.r_factor_error(out, [R], np.zeros(100, dtype=np.int64))
    assert mp.mpf(2) ** -60 < err <= mp.mpf(2) ** -53
    lo = np.zeros_like(R)
    for i in range(100):
        for j in range(i + 1):
            lo[i, j] = float(L0[i][j] - mp.mpf(float(R[i, j])))
    assert W.r_factor_error(out, [R, lo], np.zeros(100, dtype=np.int64)) <= mp.mpf(2) ** -105


def test_reference_arithmetic_on_a_short_wide_basis():
    """wide_cases.reference_gso_error — Gram-Schmidt by the reference's recurrence with every operation rounded to 53 /
    106 bits — on a reduced 24 x 256 basis: inside the project's gates (2^-40, 2^-92), the 106-bit run 2^40 better, and
    no better than the width allows.  (On the tall bases it is the yardstick where those gates cannot be met.)"""
    out = W.oracle_lll(W.short_wide(24, 256, 0))[2]
    e53, e106 = W.reference_gso_error(out, 53), W.reference_gso_error(out, 106)
    for k in (0, 1):
        assert mp.mpf(2) ** -54 < e53[k] <= mp.mpf(2) ** -40
        assert mp.mpf(2) ** -107 < e106[k] <= mp.mpf(2) ** -92
        assert e106[k] * 2 ** 40 <= e53[k]
